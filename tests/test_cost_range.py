"""GPU: the semi-global, banded, two-piece and banded two-piece batch kernels (csrc/nw_batch_semi.hip,
nw_batch_banded.hip, nw_batch_dual.hip, nw_batch_dual_banded.hip with nw_batch_dual_dev.h and
BandRange of nw_batch_dev.h) over the gap costs their argument checks accept, at tests/test_batch.py's
shapes plus what only values can get wrong.

The families' own device tests draw (ge, go) from (-1, -11), (-2, -3), (-3, 0), (-2, -11) and two-piece
costs with |v| <= 24.  Here (inputs and their conditions: tests/test_cost_range_host.py, which pins
the checkers on them):
  * ge = 0 with and without an opening (every run value ties with its extension; several equal end
    cells), ge = +1, +-4095, gap_open at the last value the range bound takes (-87 to -89 million
    beside a "minus infinity" of -2^29) next to ge = -1, -4095 and +4095;
  * two-piece costs whose piece-2 values drift by +4094, -8190 and +8190 a step, zero pieces, both
    openings at the edge of the bound with the pieces crossing at 50 and at 40, one opening at the
    edge and dominated;
  * bands 0, 3, 64 and a covering one; under (4095, 0) the checker's paths follow a band edge for 62
    to 298 vertices, under (4095, -11) they cross the band from edge to edge and either edge, moved
    by one diagonal, changes the score;
  * `ends` 0, 3, 12, 15, 6, 9: end cells strictly inside the last row and the last column at the
    go-edge, three and more equal end cells under (0, 0);
  * pairs of one to five columns on one worker in the list's order (59 to 63 lanes of the strip past
    n1), 200 pairs through each family's one-thread-per-ticket walk, chunks of more than 64 pairs.
Checkers: tests/nw_semi.py, nw_banded.py, nw_gotoh2.py, nw_banded2.py; every comparison is of integers
and bytes, exact.  A condition that makes a case mean something is asserted from the checker before
the device's result is looked at.
"""
import numpy as np
import pytest

import nw_banded as nb
import nw_banded2 as b2
import nwhip
import test_cost_range_host as h
from test_batch_semi import hit_rows
from test_scheme_range import chunks_of, same_ops

pytestmark = pytest.mark.gpu

K9, K10 = range(h.N_COSTS), range(h.N_PIECES)
kw = h.kw


@pytest.fixture(scope="module")
def ctx():
    c = nwhip.Context(0)
    yield c
    c.close()


def device_order(ctx, pairs, call):
    """One worker's call on device tensors, the pairs in the list's own order (the device entries
    do not sort): call(d_s1, d_off1, d_s2, d_off2, max_n2) -> tensor."""
    import torch
    d = [torch.from_numpy(x).cuda() for x in nwhip.batch_csr(pairs)]
    got = call(d[0], d[1], d[2], d[3], max(b.size for _, b in pairs))
    torch.cuda.synchronize()
    assert ctx.status() == nwhip.NW_OK
    return got.cpu().numpy()


def with_other(mat):
    return nwhip.SubMatrix(mat.letters, mat.scores, other=1)


def same_bytes(pairs, ops, want_ops, what):
    assert len(ops) == len(want_ops)
    for (a, b), x, y in zip(pairs, ops, want_ops):
        assert x.size == y.size and x.tobytes() == y.tobytes(), (a.size, b.size, what)   # ops and n_ops


# ================================================================== semi-global
def semi_conditions(k, ends, want, pairs):
    if k == 0 and ends:
        assert h.end_ties_decide(want, pairs) >= 3
    if k in h.GO_EDGE and ends:
        assert h.interior_ends(want, pairs, ends) >= 1


@pytest.mark.parametrize("k", K9)
def test_semi_hits(k):
    pairs, mat = h.pairs_of("score"), h.matrix()
    ge, go = h.costs("score")[k]
    for ends in h.SCORE_ENDS:
        semi_conditions(k, ends, h.semi_want("score", "M20", ge, go, ends, False), pairs)
        want = h.semi_hits("score", "M20", ge, go, ends)
        got, st = nwhip.score_batch_semi(pairs, mat, ge, go, ends, return_stats=True)
        np.testing.assert_array_equal(hit_rows(got), want, err_msg=f"ends {ends}")
        assert (got["begin_i"] == -1).all() and (got["begin_j"] == -1).all() and (got["reserved"] == 0).all()
        assert st.chunks == 1
        got, st = nwhip.score_batch_semi(pairs, mat, ge, go, ends, waves=3, return_stats=True)
        np.testing.assert_array_equal(hit_rows(got), want, err_msg=f"ends {ends}, 3 workers")
        assert st.waves == 3
        if ends == 0:
            np.testing.assert_array_equal(got["score"], nwhip.score_batch_matrix(pairs, mat, ge, go))


@pytest.mark.parametrize("k", [1, 6])
def test_semi_hits_edge_matrix(k):
    """EDGE20: with ge = 0 the table bytes are the entries themselves, 127 and -128 in every byte of
    a profile dword; with ge = -1 they leave int8 and the kernel's wide form runs, at the go-edge."""
    pairs, mat = h.pairs_of("score"), h.matrix("EDGE20")
    ge, go = h.costs("score", "EDGE20")[k]
    assert ((mat.scores - 2 * ge).max() > 127) == (k == 6)
    for ends in h.SCORE_ENDS:
        want = h.semi_hits("score", "EDGE20", ge, go, ends)
        np.testing.assert_array_equal(hit_rows(nwhip.score_batch_semi(pairs, mat, ge, go, ends)), want)
    for ends in h.OPS_ENDS:
        semi_align_and_check(h.pairs_of("score"), "score", "EDGE20", ge, go, ends)


def semi_align_and_check(pairs, batch, name, ge, go, ends, **k):
    mat = h.matrix(name)
    want = h.semi_want(batch, name, ge, go, ends)
    hits, ops, st = nwhip.align_batch_semi(pairs, mat, ge, go, ends, **k)
    np.testing.assert_array_equal(hit_rows(hits), np.array([w.hit for w in want], np.int32), err_msg=f"ends {ends}")
    assert [(int(x["begin_i"]), int(x["begin_j"])) for x in hits] == [w.begin for w in want]
    assert (hits["reserved"] == 0).all()
    same_bytes(pairs, ops, [w.ops for w in want], (ge, go, ends))
    for (a, b), x, o in zip(pairs, hits, ops):
        begin = (int(x["begin_i"]), int(x["begin_j"]))
        assert nwhip.ops_score_matrix(a, b, o, mat, ge, go, begin=begin) == x["score"]
    got = nwhip.score_batch_semi(pairs, mat, ge, go, ends, waves=k.get("waves", 0))
    np.testing.assert_array_equal(hit_rows(got), hit_rows(hits))
    return hits, ops, st, want


@pytest.mark.parametrize("k", K9)
def test_semi_ops(k):
    pairs = h.pairs_of("ops")
    ge, go = h.costs("ops")[k]
    for ends in h.OPS_ENDS:
        want = h.semi_want("ops", "M20", ge, go, ends)
        if k == 0:
            h.ties_decide(want)
        if k in h.GO_EDGE:
            assert h.interior_ends(want, pairs, ends) >= 1
        _, _, st, _ = semi_align_and_check(pairs, "ops", "M20", ge, go, ends)
        assert st.chunks == 1


@pytest.mark.parametrize("k", K9)
def test_semi_tiny_pairs_on_one_worker(ctx, k):
    """59 to 63 lanes of every pair's one strip hold columns past n1, of column n1's letter; under a
    free end of s1 and an extension that costs nothing they outscore the pair's own end cell."""
    pairs = list(h.pairs_of("tiny"))
    assert h.longest("tiny") == (5, 5)
    ge, go = h.costs("tiny")[k]
    if k in (0, 2, 3, 8):
        assert sum(h.semi_idle_lanes_outscore(pairs, "M20", ge, go, ends) for ends in (3, 15, 6)) >= 1
    if k in h.GO_EDGE:
        assert h.status_of(nwhip.score_batch_semi, pairs, h.matrix(), ge, go - 1, 3) == nwhip.NW_ERR_ARG
    full = with_other(h.matrix())
    for ends in h.SCORE_ENDS:
        want = h.semi_hits("tiny", "M20", ge, go, ends)
        got = device_order(ctx, pairs, lambda *d: ctx.score_batch_semi(*d, full, ge, go, ends, waves=1))
        np.testing.assert_array_equal(got[:, :3], want, err_msg=f"ends {ends}")
        assert (got[:, 3:5] == -1).all() and (got[:, 5:] == 0).all()
        semi_align_and_check(pairs, "tiny", "M20", ge, go, ends, waves=1)


# ================================================================== banded
def banded_align_and_check(pairs, batch, name, ge, go, w, **k):
    mat = h.matrix(name)
    want = h.banded_want(batch, name, ge, go, w)
    sc, ops, st = nwhip.align_batch_banded(pairs, mat, ge, go, w, **k)
    np.testing.assert_array_equal(sc, h.scores_of(want), err_msg=f"w {w}")
    same_bytes(pairs, ops, [x.ops for x in want], (ge, go, w))
    for (a, b), s, o in zip(pairs, sc, ops):
        assert nwhip.ops_score_matrix(a, b, o, mat, ge, go) == s
    np.testing.assert_array_equal(nwhip.score_batch_banded(pairs, mat, ge, go, w, waves=k.get("waves", 0)), sc)
    return sc, ops, st


@pytest.mark.parametrize("k", K9)
def test_banded_scores(k):
    pairs, mat = h.pairs_of("score"), h.matrix()
    ge, go = h.costs("score")[k]
    for w in h.BANDS:
        want = h.scores_of(h.banded_want("score", "M20", ge, go, w))
        got = nwhip.score_batch_banded(pairs, mat, ge, go, w)
        np.testing.assert_array_equal(got, want, err_msg=f"w {w}")
        got, st = nwhip.score_batch_banded(pairs, mat, ge, go, w, waves=3, return_stats=True)
        np.testing.assert_array_equal(got, want, err_msg=f"w {w}, 3 workers")
        assert st.waves == 3
    np.testing.assert_array_equal(got, nwhip.score_batch_matrix(pairs, mat, ge, go))   # (w = COVER)


@pytest.mark.parametrize("k", K9)
def test_banded_ops(k):
    pairs, mat = h.pairs_of("band_ops"), h.matrix()
    ge, go = h.costs("band_ops")[k]
    for w in h.BANDS:
        want = h.banded_want("band_ops", "M20", ge, go, w)
        if k in h.HUGGING and w in (3, 64):
            h.band_edge_decides("band_ops", want, w)
        if k == 0 and w == 3:
            h.ties_decide(want)
        sc, ops, _ = banded_align_and_check(pairs, "band_ops", "M20", ge, go, w)
    # the covering band: byte for byte the matrix family
    sc0, ops0, st0 = nwhip.align_batch_matrix(pairs, mat, ge, go)
    np.testing.assert_array_equal(sc, sc0)
    same_bytes(pairs, ops, ops0, "covering")


@pytest.mark.parametrize("w", [0, 3, 64])
def test_banded_paths_that_cross_the_band(w):
    pairs, m = h.pairs_of("band_ops"), h.matrix()
    ge, go = h.ZIGZAG
    if w == 3:
        h.both_edges_decide(lambda a, b, dlo, dhi: nb.score(a, b, m.scores, m.index, ge, go, dlo=dlo, dhi=dhi),
                            lambda a, b: nb.walk(a, b, m.scores, m.index, ge, go, 3), 3)
    banded_align_and_check(pairs, "band_ops", "M20", ge, go, w)


@pytest.mark.parametrize("k", [1, 6])
def test_banded_edge_matrix(k):
    pairs = h.pairs_of("score")
    ge, go = h.costs("score", "EDGE20")[k]
    for w in (0, 3, 64):
        banded_align_and_check(pairs, "score", "EDGE20", ge, go, w)


@pytest.mark.parametrize("k", K9)
def test_banded_tiny_pairs_on_one_worker(ctx, k):
    pairs = list(h.pairs_of("tiny"))
    ge, go = h.costs("tiny")[k]
    full = with_other(h.matrix())
    for w in h.TINY_BANDS:
        want = h.scores_of(h.banded_want("tiny", "M20", ge, go, w))
        got = device_order(ctx, pairs, lambda *d: ctx.score_batch_banded(*d, full, ge, go, w, waves=1))
        np.testing.assert_array_equal(got, want, err_msg=f"w {w}")
        banded_align_and_check(pairs, "tiny", "M20", ge, go, w, waves=1)


# ================================================================== two pieces, with and without a band
def dual_align_and_check(pairs, batch, name, pc, w=None, **k):
    mat = h.matrix(name)
    want = h.dual_want(batch, name, pc, w)
    align = nwhip.align_batch_dual if w is None else nwhip.align_batch_dual_banded
    score = nwhip.score_batch_dual if w is None else nwhip.score_batch_dual_banded
    sc, ops, st = align(pairs, mat, **kw(pc, w), **k)
    np.testing.assert_array_equal(sc, h.scores_of(want), err_msg=f"{pc} w {w}")
    same_bytes(pairs, ops, [x.ops for x in want], (pc, w))
    for (a, b), s, o in zip(pairs, sc, ops):
        assert nwhip.ops_score_dual(a, b, o, mat, **kw(pc)) == s
    np.testing.assert_array_equal(score(pairs, mat, waves=k.get("waves", 0), **kw(pc, w)), sc)
    return sc, ops, st


@pytest.mark.parametrize("k", K10)
def test_dual_scores(k):
    pairs, mat = h.pairs_of("dual_score"), h.matrix()
    pc = h.pieces("dual_score")[k]
    if k in h.CROSSING:
        h.both_pieces_count(k, pc)
    for w in [None] + h.BANDS:
        want = h.scores_of(h.dual_want("dual_score", "M20", pc, w))
        score = nwhip.score_batch_dual if w is None else nwhip.score_batch_dual_banded
        np.testing.assert_array_equal(score(pairs, mat, **kw(pc, w)), want, err_msg=f"w {w}")
        got, st = score(pairs, mat, waves=3, return_stats=True, **kw(pc, w))
        np.testing.assert_array_equal(got, want, err_msg=f"w {w}, 3 workers")
        assert st.waves == 3
    np.testing.assert_array_equal(got, h.scores_of(h.dual_want("dual_score", "M20", pc)))   # COVER is no band


@pytest.mark.parametrize("k", K10)
def test_dual_ops(k):
    pairs = h.pairs_of("ops")
    pc = h.pieces("ops")[k]
    if k == 5:
        h.ties_decide(h.dual_want("ops", "M20", pc))
    sc0, ops0, st0 = dual_align_and_check(pairs, "ops", "M20", pc)
    assert st0.chunks == 1
    for w in h.BANDS:
        sc, ops, st = dual_align_and_check(pairs, "ops", "M20", pc, w)
    # the covering band: byte for byte the unbanded family
    np.testing.assert_array_equal(sc, sc0)
    same_bytes(pairs, ops, ops0, "covering")
    assert st.dir_bytes == st0.dir_bytes


@pytest.mark.parametrize("w", [0, 3, 64])
@pytest.mark.parametrize("pc", [h.HUG_PIECES, h.ZIGZAG_PIECES, (0, 0, 0, 0)], ids=["hug", "zigzag", "zero"])
def test_dual_banded_paths_along_and_across_the_band(pc, w):
    pairs, m = h.pairs_of("band_ops"), h.matrix()
    want = h.dual_want("band_ops", "M20", pc, w)
    if pc == h.HUG_PIECES and w:
        h.band_edge_decides("band_ops", want, w)
    if pc == h.ZIGZAG_PIECES and w == 3:
        h.both_edges_decide(lambda a, b, dlo, dhi: b2.score(a, b, m.scores, m.index, pc, dlo=dlo, dhi=dhi),
                            lambda a, b: b2.walk(a, b, m.scores, m.index, pc, 3), 3)
    if pc == (0, 0, 0, 0) and w == 3:
        h.ties_decide(want)
    dual_align_and_check(pairs, "band_ops", "M20", pc, w)


@pytest.mark.parametrize("k", [4, 6])
def test_dual_edge_matrix(k):
    """EDGE20 under (-3, 0, 0, -2) (ge1 = 0: the table bytes are the entries, 127 and -128 among them)
    and under both openings at the edge beside ge1 = -1 (the wide form)."""
    pairs = h.pairs_of("score")
    pc = h.pieces("score", "EDGE20")[k]
    assert ((h.matrix("EDGE20").scores - 2 * pc[1]).max() > 127) == (k == 6)
    dual_align_and_check(pairs, "score", "EDGE20", pc)
    for w in (0, 3, 64):
        dual_align_and_check(pairs, "score", "EDGE20", pc, w)


@pytest.mark.parametrize("k", K10)
def test_dual_tiny_pairs_on_one_worker(ctx, k):
    pairs = list(h.pairs_of("tiny"))
    pc = h.pieces("tiny")[k]
    full = with_other(h.matrix())
    want = h.scores_of(h.dual_want("tiny", "M20", pc))
    got = device_order(ctx, pairs, lambda *d: ctx.score_batch_dual(*d, full, waves=1, **kw(pc)))
    np.testing.assert_array_equal(got, want)
    dual_align_and_check(pairs, "tiny", "M20", pc, waves=1)
    for w in h.TINY_BANDS:
        want = h.scores_of(h.dual_want("tiny", "M20", pc, w))
        got = device_order(ctx, pairs, lambda *d: ctx.score_batch_dual_banded(*d, full, waves=1, **kw(pc, w)))
        np.testing.assert_array_equal(got, want, err_msg=f"w {w}")
        dual_align_and_check(pairs, "tiny", "M20", pc, w, waves=1)


# ================================================================== 200 pairs through the four walks
def run_crowd(align, check, dir_bytes, hit_bytes=0):
    """align(pairs, **kw) -> (results, ops, stats); check(results, ops): against the checker.  The
    chunks are replayed from `dir_bytes` and the unchunked call's peak_bytes (tests/test_scheme_
    range.py chunks_of): at least three, one above 64 pairs."""
    pairs = h.crowd()
    live = [(a.size, b.size) for a, b in pairs if a.size and b.size]
    r0, ops0, st0 = align(pairs)
    assert st0.chunks == 1 and st0.pairs == 200
    assert st0.dir_bytes == sum(dir_bytes(n1, n2) for n1, n2 in live)
    check(r0, ops0)
    fixed = st0.peak_bytes - st0.dir_bytes - sum(n1 + n2 for n1, n2 in live)
    assert fixed > hit_bytes * 200
    mem = fixed + 80 * (dir_bytes(12, 12) + 24)
    want_chunks = chunks_of(pairs, dir_bytes, fixed, mem)
    assert len(want_chunks) >= 3 and max(want_chunks) > 64 and sum(want_chunks) == len(live)
    r, ops, st = align(pairs, mem_bytes=mem)
    assert st.chunks == len(want_chunks) and st.peak_bytes <= mem and st.dir_bytes == st0.dir_bytes
    np.testing.assert_array_equal(r, r0)
    same_ops(ops, ops0)


@pytest.mark.parametrize("cost,ends", h.CROWD_SEMI)
def test_200_pairs_semi(cost, ends):
    pairs, mat = h.crowd(), h.matrix()
    ge, go = cost
    want = h.semi_want("crowd", "M20", ge, go, ends)
    h.crowd_walks(want)

    def check(hits, ops):
        np.testing.assert_array_equal(hit_rows(hits), np.array([w.hit for w in want], np.int32))
        assert [(int(x["begin_i"]), int(x["begin_j"])) for x in hits] == [w.begin for w in want]
        same_bytes(pairs, ops, [w.ops for w in want], (cost, ends))
        np.testing.assert_array_equal(hit_rows(nwhip.score_batch_semi(pairs, mat, ge, go, ends, waves=3)), hit_rows(hits))

    run_crowd(lambda p, **k: nwhip.align_batch_semi(p, mat, ge, go, ends, **k), check, nwhip.batch_affine_dir_bytes, 32)


@pytest.mark.parametrize("cost,w", h.CROWD_BANDED)
def test_200_pairs_banded(cost, w):
    pairs, mat = h.crowd(), h.matrix()
    ge, go = cost
    want = h.banded_want("crowd", "M20", ge, go, w)
    h.crowd_walks(want)

    def check(sc, ops):
        np.testing.assert_array_equal(sc, h.scores_of(want))
        same_bytes(pairs, ops, [x.ops for x in want], (cost, w))
        np.testing.assert_array_equal(nwhip.score_batch_banded(pairs, mat, ge, go, w, waves=3), sc)

    run_crowd(lambda p, **k: nwhip.align_batch_banded(p, mat, ge, go, w, **k), check,
              lambda n1, n2: nwhip.batch_banded_dir_bytes(n1, n2, w))


@pytest.mark.parametrize("w", [None, h.CROWD_DUAL_BAND])
@pytest.mark.parametrize("pc", h.CROWD_DUAL, ids=str)
def test_200_pairs_dual(pc, w):
    pairs, mat = h.crowd(), h.matrix()
    want = h.dual_want("crowd", "M20", pc, w)
    h.crowd_walks(want)
    align = nwhip.align_batch_dual if w is None else nwhip.align_batch_dual_banded
    score = nwhip.score_batch_dual if w is None else nwhip.score_batch_dual_banded

    def check(sc, ops):
        np.testing.assert_array_equal(sc, h.scores_of(want))
        same_bytes(pairs, ops, [x.ops for x in want], (pc, w))
        np.testing.assert_array_equal(score(pairs, mat, waves=3, **kw(pc, w)), sc)

    run_crowd(lambda p, **k: align(p, mat, **kw(pc, w), **k), check,
              nwhip.batch_dual_dir_bytes if w is None else (lambda n1, n2: nwhip.batch_dual_banded_dir_bytes(n1, n2, w)))
