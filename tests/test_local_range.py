"""GPU: the batched local kernels (csrc/nw_batch_local.hip: nw_score_batch_local,
nw_align_batch_local, nw_score_batch_local_async) over the matrices and gap costs they
accept, at tests/test_batch_local.py's shapes plus what only values can get wrong.

tests/test_batch_local.py draws (ge, go) from four small pairs, matrix entries from
-8..11 and a negative expected score.  Here (inputs and their conditions: tests/
test_local_range_host.py, which pins the checker on them):
  * matrix entries 127 and -128 in every byte of a lane's profile dword, a matrix of
    positive entries only, entries of 0 on and off the diagonal, a matrix without a
    positive entry; a score above 2^15;
  * ge = 0 (with go = 0: every E and F ties with an H), ge = -4095, gap_open at the last
    value the range bound takes (about -87 to -89 million beside scores of thousands);
  * 97 to 258 equal maxima: two in one lane's columns on one row, in all three strips,
    down one column over four row blocks;
  * pairs of one to five columns on one worker under a matrix whose idle lanes win;
  * 200 pairs through nw_batch_local_walk (one thread per ticket) and chunks of more
    than 64 pairs.
Checker: tests/nw_local.py (fill, best, walk, path_score); every comparison is of
integers and bytes, exact.  A condition that makes a case mean something is asserted
from the checker before the device's result is looked at.
"""
import numpy as np
import pytest

import nwhip
import test_batch_local as tbl
import test_local_range_host as h
from test_scheme_range import chunks_of, same_ops

pytestmark = pytest.mark.gpu

WIDE = ["EDGE20", "POS20"]
EMPTY_ALIGNED = (0, 0, 0, 0, 0)


def rows_of(want):
    return np.array([hit for hit, _, _, _ in want], np.int32)


# ------------------------------------------------------------------ 1. hits over matrices x costs
@pytest.mark.parametrize("k", range(h.N_COSTS))
@pytest.mark.parametrize("name", WIDE)
def test_hits_over_matrices_and_costs(name, k):
    pairs, mat = h.score_batch(), h.matrix(name)
    ge, go = h.costs(name, pairs)[k]
    want = h.want_hits("score", name, ge, go)
    live = np.array([a.size > 0 and b.size > 0 for a, b in pairs])
    assert (want[~live] == 0).all() and (want[live, 0] > 0).sum() >= 30
    if name == "EDGE20":
        assert want[-1, 0] > 32767 and tuple(want[-1, 1:]) == (300, 300)
    else:
        # H is never floored: the best cell of every pair lies on the last row or column
        n1, n2 = np.array([a.size for a, _ in pairs]), np.array([b.size for _, b in pairs])
        assert (want[live, 0] > 0).all() and ((want[:, 1] == n2) | (want[:, 2] == n1))[live].all()
    got, st = nwhip.score_batch_local(pairs, mat, ge, go, return_stats=True)
    np.testing.assert_array_equal(tbl.hit_rows(got), want)
    assert (got["begin_i"] == -1).all() and (got["begin_j"] == -1).all() and (got["reserved"] == 0).all()
    assert st.chunks == 1 and st.waves >= 1
    got, st = nwhip.score_batch_local(pairs, mat, ge, go, waves=3, return_stats=True)
    np.testing.assert_array_equal(tbl.hit_rows(got), want)
    assert st.waves == 3


# ------------------------------------------------------------------ 2. ops over matrices x costs
@pytest.mark.parametrize("k", range(h.N_COSTS))
@pytest.mark.parametrize("name", WIDE)
def test_ops_over_matrices_and_costs(name, k):
    pairs, mat = h.ops_batch(), h.matrix(name)
    ge, go = h.costs(name, pairs)[k]
    want = h.want_alignments(pairs, name, ge, go)
    if name == "POS20":
        for (a, b), (hit, begin, ops, _) in zip(pairs, want):
            assert 0 in begin and (hit[1] == b.size or hit[2] == a.size) and hit[0] > 0
    else:
        assert want[-1][0][0] > 32767 and want[-1][2].size == 300
    if k in h.EDGE_COSTS:
        assert go < -86_000_000 and h.gap_ops(want) == 0 and sum(w[2].size for w in want) > 400
    if (ge, go) == (0, 0):
        lefts, ups = h.open_ties(want, ge, go)
        assert lefts >= 1 and ups >= 1
    if ge == 0:
        assert h.gap_ops(want) >= 10  # the gaps are walked, not only priced
    hits, ops, st = nwhip.align_batch_local(pairs, mat, ge, go)
    got = tbl.check_alignments(pairs, mat, ge, go, hits, ops)
    for (begin, end, o), (hit, wbegin, wops, _) in zip(got, want):
        assert begin == wbegin and end == hit[1:] and o.size == wops.size
    assert st.chunks == 1
    np.testing.assert_array_equal(tbl.hit_rows(nwhip.score_batch_local(pairs, mat, ge, go)), tbl.hit_rows(hits))


# ------------------------------------------------------------------ 3. zeros
@pytest.mark.parametrize("ge,go", h.ZERO_COSTS)
def test_zero_entries(ge, go):
    pairs = h.zero_pairs()
    assert [(a.size, b.size) for a, b in pairs] == h.ZERO_SHAPES
    want = h.want_alignments(pairs, "ZERO4", ge, go)
    assert all(hit[0] > 0 for hit, _, _, _ in want)
    assert h.zero_diagonal_stops(pairs, "ZERO4", want) >= (ge < 0)
    none = h.want_alignments(pairs, "NONPOS4", ge, go)
    n4 = h.matrix("NONPOS4")
    for (a, b), (hit, begin, ops, _) in zip(pairs, none):
        assert (h.sub_table(a, b, n4.scores, n4.index) == 0).sum() >= 5  # zero-scoring diagonal steps exist
        assert hit == (0, 0, 0) and begin == (0, 0) and ops.size == 0
    for waves in (0, 1):
        z4 = h.matrix("ZERO4")
        hits, ops, _ = nwhip.align_batch_local(pairs, z4, ge, go, waves=waves)
        tbl.check_alignments(pairs, z4, ge, go, hits, ops)
        np.testing.assert_array_equal(tbl.hit_rows(nwhip.score_batch_local(pairs, z4, ge, go, waves=waves)), rows_of(want))
        hits, ops, _ = nwhip.align_batch_local(pairs, n4, ge, go, waves=waves)
        tbl.check_alignments(pairs, n4, ge, go, hits, ops)
        for hit, o in zip(hits, ops):
            assert tuple(hit)[:5] == EMPTY_ALIGNED and o.size == 0
        got = nwhip.score_batch_local(pairs, n4, ge, go, waves=waves)
        assert (tbl.hit_rows(got) == 0).all() and (got["begin_i"] == -1).all()


# ------------------------------------------------------------------ 4. periodic ties
@pytest.mark.parametrize("waves", [0, 1])
def test_periodic_ties(waves):
    pairs, mat = h.periodic_pairs(), h.matrix("UNI4")
    ge, go = h.PERIODIC_COST
    firsts = []
    for name in h.PERIODIC:
        top, score = h.periodic_facts(name)  # (asserts the number of maxima and where they lie)
        firsts.append((score, *top[0]))
    assert firsts == [(30, 6, 6), (30, 6, 7), (30, 6, 6), (30, 7, 6), (1000, 200, 200), (1000, 200, 201)]
    hits, ops, _ = nwhip.align_batch_local(pairs, mat, ge, go, waves=waves)
    assert [tuple(r) for r in tbl.hit_rows(hits).tolist()] == firsts
    tbl.check_alignments(pairs, mat, ge, go, hits, ops)
    got = nwhip.score_batch_local(pairs, mat, ge, go, waves=waves)
    assert [tuple(r) for r in tbl.hit_rows(got).tolist()] == firsts


# ------------------------------------------------------------------ 5. tiny pairs, one worker
def device_order_hits(ctx, pairs, mat, ge, go):
    """One worker, the pairs in the list's own order (the device entry does not sort)."""
    import torch
    s1, off1, s2, off2 = nwhip.batch_csr(pairs)
    d = [torch.from_numpy(x).cuda() for x in (s1, off1, s2, off2)]
    got = ctx.score_batch_local(d[0], d[1], d[2], d[3], max(b.size for _, b in pairs), mat, ge, go, waves=1)
    torch.cuda.synchronize()
    assert ctx.status() == nwhip.NW_OK
    return got.cpu().numpy()


@pytest.mark.parametrize("edge", [False, True])
@pytest.mark.parametrize("name", WIDE)
def test_tiny_pairs_on_one_worker(name, edge):
    """59 to 63 lanes of every pair's one strip hold columns past n1, of column n1's letter:
    under POS20 their cells outscore the pair's own."""
    pairs = list(h.tiny_pairs())
    assert h.longest(pairs) == (5, 5)
    ge, go = (-h.CAP, h.edge_open(name, -h.CAP, (5, 5))) if edge else (-1, -11)
    if name == "POS20":
        assert h.idle_lanes_outscore(pairs, name, ge, go) >= 3
    if edge:
        assert h.status_of(nwhip.score_batch_local, pairs, h.matrix(name), ge, go - 1) == nwhip.NW_ERR_ARG
    want = h.want_hits("tiny", name, ge, go)
    assert (want[:, 0] > 0).sum() >= (7 if name == "POS20" else 2)
    mat = h.matrix(name)
    for waves in (1, 0):
        got, st = nwhip.score_batch_local(pairs, mat, ge, go, waves=waves, return_stats=True)
        np.testing.assert_array_equal(tbl.hit_rows(got), want)
        hits, ops, st = nwhip.align_batch_local(pairs, mat, ge, go, waves=waves)
        assert waves == 0 or st.waves == 1
        tbl.check_alignments(pairs, mat, ge, go, hits, ops)
    ctx = nwhip.Context(0)
    try:
        got = device_order_hits(ctx, pairs, nwhip.SubMatrix(mat.letters, mat.scores, other=1), ge, go)
    finally:
        ctx.close()
    np.testing.assert_array_equal(got[:, :3], want)
    assert (got[:, 3:5] == -1).all() and (got[:, 5:] == 0).all()


# ------------------------------------------------------------------ 6. 200 pairs through the local walk
def test_200_pairs_local():
    pairs, mat = h.crowd(), h.matrix("UNI4")
    ge, go = h.CROWD_COST
    want, order = h.crowd_facts()  # (asserts what the crowd is there for)
    live = [(pairs[k][0].size, pairs[k][1].size) for k in order]
    dir_bytes = nwhip.batch_affine_dir_bytes

    hits0, ops0, st0 = nwhip.align_batch_local(pairs, mat, ge, go)
    assert st0.chunks == 1 and st0.pairs == 200
    assert st0.dir_bytes == sum(dir_bytes(n1, n2) for n1, n2 in live)
    got = tbl.check_alignments(pairs, mat, ge, go, hits0, ops0)
    for (a, b), hit, o, (begin, end, wops), w in zip(pairs, hits0, ops0, got, want):
        assert o.size == w[2].size and begin == w[1]
        if a.size == 0 or b.size == 0:
            assert tuple(hit)[:5] == EMPTY_ALIGNED and o.size == 0
    again = nwhip.score_batch_local(pairs, mat, ge, go, waves=3)
    np.testing.assert_array_equal(tbl.hit_rows(again), tbl.hit_rows(hits0))

    # what one chunk held beside the direction bytes and the ops slots (the hits are in it: 32
    # bytes a pair, held for the whole call); then room for the ten long pairs and some fifty
    # short ones, or for eighty short ones -- tests/test_scheme_range.py check_crowd's sizes
    fixed = st0.peak_bytes - st0.dir_bytes - sum(n1 + n2 for n1, n2 in live)
    assert fixed > 32 * 200
    mem = fixed + 80 * (dir_bytes(12, 12) + 24)
    want_chunks = chunks_of(pairs, dir_bytes, fixed, mem)
    assert len(want_chunks) >= 3 and max(want_chunks) > 64 and sum(want_chunks) == len(live)
    hits, ops, st = nwhip.align_batch_local(pairs, mat, ge, go, mem_bytes=mem)
    assert st.chunks == len(want_chunks) and st.peak_bytes <= mem and st.dir_bytes == st0.dir_bytes
    np.testing.assert_array_equal(hits, hits0)
    same_ops(ops, ops0)
