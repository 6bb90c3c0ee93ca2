"""GPU: the batched (linear, affine, matrix), checkpointed and global-traceback kernels
over the range of scoring schemes they accept, at the smallest shapes that hold every
mechanism (tests/test_batch.py's pairs, tests/test_ckpt.py's seeds).

Every other device test of these kernels draws its scheme from four with |v| <= 2, a
negative gap and match > mismatch.  Here:
  * WIDE_SCHEMES (tests/test_scheme_range_host.py): the v_perm table bytes match - 2 gap
    and mismatch - 2 gap at 127 / 128 and -128 / -129, positive and zero gap, match <=
    mismatch, the largest values; the table-side ones a second time with the tables off;
  * values at the accepted edge: the scheme at the parameter limit 4095 in either sign,
    gap_open at the edge of the affine and the matrix range bound (-89 478 055 next to a
    -2^29 "minus infinity") for large pairs, for tiny ones whose last strip is 251 idle
    columns, for one 300-long run, next to the scheme limit and next to an int8 matrix;
  * 200 pairs through the walks: blocks 1 and 2 of a one-thread-per-pair kernel, chunks
    of more than 64 pairs.
Checkers: oracle.fill / oracle.score with nw_walk.walk; nw_gotoh; nw_gotoh_matrix --
pinned on these very inputs by the host module.  Every comparison is exact.
"""
import functools

import numpy as np
import pytest

import nw_gotoh
import nw_gotoh_matrix as gm
import nwhip
import oracle
import test_batch as tb
import test_batch_affine as tba
import test_batch_matrix as tbm
import test_ckpt as tc
from test_scheme_range_host import (AFFINE_EDGES, BIG, CAP, CAP_SCHEME, LIMIT, MATRIX_EDGES, MID, TINY, WIDE_SCHEMES,
                                    aff_sum, edge_matrix, lin_sum, rand_pair, status_of)

pytestmark = pytest.mark.gpu

OPENS = [-1, -11, -1000003]
# the side of int8 the first four schemes are there for: True = both table bytes fit
INT8_SIDE = {(125, -1, -1): True, (126, -1, -1): False, (1, -130, -1): True, (1, -131, -1): False}
LIMIT_SCHEMES = [CAP_SCHEME, (-CAP, CAP, CAP)]


def forms(scheme):
    """The flags to run a scheme with: the table-side ones also with the tables off."""
    m, mm, g = scheme
    fits = -128 <= m - 2 * g <= 127 and -128 <= mm - 2 * g <= 127
    if scheme in INT8_SIDE:
        assert fits == INT8_SIDE[scheme]
        assert 127 in (m - 2 * g, mm - 2 * g) or -128 in (m - 2 * g, mm - 2 * g) if fits else \
            128 in (m - 2 * g, mm - 2 * g) or -129 in (m - 2 * g, mm - 2 * g)
    return [0, nwhip.FLAG_NO_PROFILE] if fits else [0]


def same_ops(ops, ops0):
    assert len(ops) == len(ops0)
    for x, y in zip(ops, ops0):
        np.testing.assert_array_equal(x, y)


def device_order_scores(ctx, pairs, scheme, gap_open=None):
    """One worker, the pairs in the list's own order (the device entry does not sort)."""
    import torch
    s1, off1, s2, off2 = nwhip.batch_csr(pairs)
    d = [torch.from_numpy(x).cuda() for x in (s1, off1, s2, off2)]
    got = ctx.score_batch(d[0], d[1], d[2], d[3], max(b.size for _, b in pairs), scheme, waves=1, gap_open=gap_open)
    torch.cuda.synchronize()
    assert ctx.status() == nwhip.NW_OK
    return got.cpu().numpy()


@pytest.fixture(scope="module")
def ctx():
    c = nwhip.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ 2. linear batch
@pytest.mark.parametrize("scheme", WIDE_SCHEMES)
def test_linear_batch_scores(ctx, scheme):
    pairs, want = tb.score_pairs(), tb.score_want(4, scheme)
    for flags in forms(scheme):
        np.testing.assert_array_equal(nwhip.score_batch(pairs, scheme, flags=flags), want)
        got, st = nwhip.score_batch(pairs, scheme, waves=3, flags=flags, return_stats=True)
        np.testing.assert_array_equal(got, want)
        assert st.waves == 3
    # the device entry: the empty sides are the kernel's own here, not the host's
    np.testing.assert_array_equal(device_order_scores(ctx, pairs, scheme), want)


@pytest.mark.parametrize("scheme", WIDE_SCHEMES)
def test_linear_batch_ops(scheme):
    pairs = tb.ops_pairs()
    sc0, ops0, _ = nwhip.align_batch(pairs, scheme)
    tb.check_alignments(pairs, scheme, sc0, ops0)
    for flags in forms(scheme)[1:]:
        sc, ops, _ = nwhip.align_batch(pairs, scheme, flags=flags)
        np.testing.assert_array_equal(sc, sc0)
        same_ops(ops, ops0)


# ------------------------------------------------------------------ 2. affine batch
@pytest.mark.parametrize("go", OPENS)
@pytest.mark.parametrize("scheme", WIDE_SCHEMES)
def test_affine_batch_scores(ctx, scheme, go):
    pairs, want = tb.score_pairs(), tba.score_want(4, scheme, go)
    for flags in forms(scheme):
        np.testing.assert_array_equal(nwhip.score_batch_affine(pairs, scheme, go, flags=flags), want)
        np.testing.assert_array_equal(nwhip.score_batch_affine(pairs, scheme, go, waves=3, flags=flags), want)
    np.testing.assert_array_equal(device_order_scores(ctx, pairs, scheme, gap_open=go), want)


@pytest.mark.parametrize("go", OPENS)
@pytest.mark.parametrize("scheme", WIDE_SCHEMES)
def test_affine_batch_ops(scheme, go):
    pairs = tb.ops_pairs()
    sc0, ops0, _ = nwhip.align_batch_affine(pairs, scheme, go)
    tba.check_alignments(pairs, scheme, go, sc0, ops0)
    for flags in forms(scheme)[1:]:
        sc, ops, _ = nwhip.align_batch_affine(pairs, scheme, go, flags=flags)
        np.testing.assert_array_equal(sc, sc0)
        same_ops(ops, ops0)


# ------------------------------------------------------------------ 2. checkpoint sweep, alignment, traceback
CKPT_SHAPES = [(257, 513), (300, 200)]  # (n1, n2)


@pytest.mark.parametrize("scheme", WIDE_SCHEMES)
def test_checkpointed(ctx, scheme):
    """nw_score, nw_align_ckpt in blocks of 64 rows, and the sweep's rows 64, 128, .. themselves."""
    import torch
    for n1, n2 in CKPT_SHAPES:
        s1, s2 = tc.seqs(n1, n2, 4)
        t, want = tc.table(n1, n2, 4, scheme), tc.walked(n1, n2, 4, scheme)
        for flags in forms(scheme):
            assert nwhip.score_sweep(s1, s2, scheme, flags=flags).score == t[n2, n1]
            tc.check_align(s1, s2, scheme, want, int(t[n2, n1]), 64, flags=flags)
            if n2 == 513:
                tc.check_sweep(torch, ctx, s1, s2, t, 64, scheme, flags=flags)


@pytest.mark.parametrize("scheme", WIDE_SCHEMES + LIMIT_SCHEMES[1:])
def test_global_traceback(scheme):
    for n1, n2 in [(257, 513), (65, 63)]:
        s1, s2 = tc.seqs(n1, n2, 4)
        t, want = tc.table(n1, n2, 4, scheme), tc.walked(n1, n2, 4, scheme)
        al, ops, _ = nwhip.align(s1, s2, scheme)
        np.testing.assert_array_equal(ops, want)
        assert al.score == t[n2, n1] == nwhip.ops_score(s1, s2, ops, scheme)
        assert (al.begin_i, al.begin_j, al.end_i, al.end_j, al.n_ops) == (0, 0, n2, n1, want.size)


# ------------------------------------------------------------------ 3. the accepted edges
def tiny_pairs(alpha=4):
    """1 x 1 .. 5 x 5, a 5 x 5 pair last: of every pair's one strip at most two lanes hold columns."""
    return [rand_pair(10 + k, n1, n2, alpha) for k, (n1, n2) in enumerate(TINY + [(5, 5)])]


@pytest.mark.parametrize("scheme", LIMIT_SCHEMES)
def test_linear_at_the_scheme_limit(scheme):
    """513 x 130 and 257 x 65 under +-4095: the largest scheme there is (4096 is refused), the
    w form at 8190 per cell.  The range bound itself is 50 times away (the host module)."""
    pairs = [rand_pair(1, *BIG), rand_pair(2, *MID)]
    assert lin_sum(scheme, *BIG) < LIMIT and max(abs(v) for v in scheme) == CAP
    one_more = tuple(v + (1 if v > 0 else -1) for v in scheme)
    assert status_of(nwhip.score_batch, pairs, one_more) == nwhip.NW_ERR_ARG
    want = [oracle.score(a, b, scheme) for a, b in pairs]
    assert nwhip.score_batch(pairs, scheme).tolist() == want
    sc, ops, _ = nwhip.align_batch(pairs, scheme)
    tb.check_alignments(pairs, scheme, sc, ops)
    for (a, b), w, o in zip(pairs, want, ops):
        assert nwhip.score_sweep(a, b, scheme).score == w
        tc.check_align(a, b, scheme, o, w, 64)


@pytest.mark.parametrize("scheme", LIMIT_SCHEMES)
def test_linear_tiny_pairs_at_the_scheme_limit(ctx, scheme):
    """Pairs of one to five columns: 59 to 63 lanes of the strip hold columns past n1, whose
    cells must reach no real cell and no score -- also not the next pair's on the same worker."""
    pairs = tiny_pairs()
    want = [oracle.score(a, b, scheme) for a, b in pairs]
    for waves in (1, 0):
        assert nwhip.score_batch(pairs, scheme, waves=waves).tolist() == want
        sc, ops, st = nwhip.align_batch(pairs, scheme, waves=waves)
        assert waves == 0 or st.waves == 1
        tb.check_alignments(pairs, scheme, sc, ops)
    assert device_order_scores(ctx, pairs, scheme).tolist() == want


@pytest.mark.parametrize("case", ["go_at_the_edge", "scheme_at_its_limit"])
def test_affine_gap_open_at_the_edge(case):
    """3 |go| + (M + |ge|) * 645 one unit below 2^28: H', E' and F' down to 3 go = -2^28 + a
    little, next to the -2^29 they must beat in every maximum."""
    scheme, go, shape = AFFINE_EDGES[case]
    assert shape == BIG and aff_sum(scheme, go, *BIG) < LIMIT <= aff_sum(scheme, go - 1, *BIG)
    pairs = [rand_pair(1, *BIG), rand_pair(2, *MID)]
    assert status_of(nwhip.score_batch_affine, pairs, scheme, go - 1) == nwhip.NW_ERR_ARG
    assert status_of(nwhip.align_batch_affine, pairs, scheme, go - 1) == nwhip.NW_ERR_ARG
    want = [nw_gotoh.score(a, b, scheme, go) for a, b in pairs]
    for flags in forms(scheme):
        assert nwhip.score_batch_affine(pairs, scheme, go, flags=flags).tolist() == want
        assert nwhip.score_batch_affine(pairs, scheme, go, waves=1, flags=flags).tolist() == want
        sc, ops, _ = nwhip.align_batch_affine(pairs, scheme, go, flags=flags)
        tba.check_alignments(pairs, scheme, go, sc, ops)


def test_affine_tiny_pairs_with_gap_open_at_their_edge(ctx):
    """The batch's largest pair is 5 x 5: 3 |go| + 2 * 12 < 2^28.  Lanes past n1 as above."""
    scheme, go, shape = AFFINE_EDGES["go_at_the_edge_tiny"]
    assert shape == (5, 5) and aff_sum(scheme, go, 5, 5) < LIMIT <= aff_sum(scheme, go - 1, 5, 5)
    pairs = tiny_pairs()
    assert status_of(nwhip.score_batch_affine, pairs, scheme, go - 1) == nwhip.NW_ERR_ARG
    want = [nw_gotoh.score(a, b, scheme, go) for a, b in pairs]
    for waves in (1, 0):
        for flags in forms(scheme):
            assert nwhip.score_batch_affine(pairs, scheme, go, waves=waves, flags=flags).tolist() == want
            sc, ops, _ = nwhip.align_batch_affine(pairs, scheme, go, waves=waves, flags=flags)
            tba.check_alignments(pairs, scheme, go, sc, ops)
    assert device_order_scores(ctx, pairs, scheme, gap_open=go).tolist() == want


@pytest.mark.parametrize("tall", [False, True])
def test_affine_one_long_run_with_gap_open_at_the_edge(tall):
    """test_batch_affine.seam_pair() (600 against 300): with gap_open at this pair's edge the path
    is still ONE run of 300 gap ops, extended over the strip seams (wide) or the row blocks
    (tall) while E' / F' sit a third of the budget above the -2^29."""
    scheme, go, shape = AFFINE_EDGES["go_at_the_edge_seam"]
    a, b = tba.seam_pair()
    assert (a.size, b.size) == shape and aff_sum(scheme, go, *shape) < LIMIT <= aff_sum(scheme, go - 1, *shape)
    s1, s2 = (b, a) if tall else (a, b)
    op = 1 if tall else 2
    assert status_of(nwhip.align_batch_affine, [(s1, s2)], scheme, go - 1) == nwhip.NW_ERR_ARG
    want = nw_gotoh.walk(s1, s2, scheme, go)
    (start, length), = nw_gotoh.runs(want, op)
    assert length == 300 and nw_gotoh.runs(want, 3 - op) == [] and want.size == 600
    for waves in (0, 1):
        sc, ops, _ = nwhip.align_batch_affine([(s1, s2)], scheme, go, waves=waves)
        np.testing.assert_array_equal(ops[0], want)
        assert sc[0] == nw_gotoh.score(s1, s2, scheme, go) == nw_gotoh.path_score_affine(s1, s2, want, scheme, go)
        assert nwhip.score_batch_affine([(s1, s2)], scheme, go, waves=waves)[0] == sc[0]


@pytest.mark.parametrize("case", sorted(MATRIX_EDGES))
def test_matrix_at_the_edge(case):
    """matrix(20) (entries -8..12) with gap_open at the edge of its bound for 513 x 130, next
    to gap_extend -1 and next to -4095, where every table byte s - 2 ge is far outside int8
    and the kernel adds -2 ge itself."""
    ge, go, shape = MATRIX_EDGES[case]
    mat = tbm.matrix(20)
    np.testing.assert_array_equal(mat.scores, edge_matrix().scores)
    assert shape == BIG and aff_sum((0, 0, ge), go, *BIG, mat_abs=12) < LIMIT <= aff_sum((0, 0, ge), go - 1, *BIG, mat_abs=12)
    if case == "ge_at_its_limit":
        assert (mat.scores - 2 * ge).min() > 127
    pairs = [rand_pair(1, *BIG, 20), rand_pair(2, *MID, 20)]
    assert status_of(nwhip.score_batch_matrix, pairs, mat, ge, go - 1) == nwhip.NW_ERR_ARG
    assert status_of(nwhip.align_batch_matrix, pairs, mat, ge, go - 1) == nwhip.NW_ERR_ARG
    want = [gm.score(a, b, mat.scores, mat.index, ge, go) for a, b in pairs]
    assert nwhip.score_batch_matrix(pairs, mat, ge, go).tolist() == want
    assert nwhip.score_batch_matrix(pairs, mat, ge, go, waves=1).tolist() == want
    sc, ops, _ = nwhip.align_batch_matrix(pairs, mat, ge, go)
    tbm.check_alignments(pairs, mat, ge, go, sc, ops)


# ------------------------------------------------------------------ 4. more than 64 pairs through the walks
@functools.lru_cache(maxsize=None)
def crowd(alpha):
    """200 pairs, shuffled: 190 with both sides drawn from 0..12 and ten of about 300 x 70."""
    rng = np.random.default_rng(640 + alpha)
    sizes = [(int(rng.integers(0, 13)), int(rng.integers(0, 13))) for _ in range(190)]
    sizes += [(int(rng.integers(280, 321)), int(rng.integers(60, 81))) for _ in range(10)]
    pairs = [(tb._rand(rng, n1, alpha), tb._rand(rng, n2, alpha)) for n1, n2 in sizes]
    pairs = tuple(pairs[i] for i in rng.permutation(len(pairs)))
    live = sum(1 for a, b in pairs if a.size and b.size)
    # empty sides are there, and the pairs with cells fill blocks 0, 1 and 2 of a walk
    assert len(pairs) == 200 and 128 < live < 190
    assert any(a.size == 0 and b.size for a, b in pairs) and any(b.size == 0 and a.size for a, b in pairs)
    return pairs


def chunks_of(pairs, dir_bytes, fixed, mem):
    """Pairs per chunk: consecutive runs of the longest-first order (pairs with cells only) whose
    direction bytes and ops slots fit mem - fixed."""
    live = sorted(((a.size, b.size) for a, b in pairs if a.size and b.size), key=lambda s: -s[0] * s[1])
    out, cur = [], 0
    for n1, n2 in live:
        need = dir_bytes(n1, n2) + n1 + n2
        if not out or fixed + cur + need > mem:
            out.append(0)
            cur = 0
        out[-1] += 1
        cur += need
    return out


def check_crowd(pairs, align, score, check, dir_bytes):
    sc0, ops0, st0 = align(pairs)
    assert st0.chunks == 1 and st0.pairs == 200
    live = [(a.size, b.size) for a, b in pairs if a.size and b.size]
    assert st0.dir_bytes == sum(dir_bytes(n1, n2) for n1, n2 in live)
    check(pairs, sc0, ops0)
    np.testing.assert_array_equal(score(pairs, waves=3), sc0)
    # what one chunk held beside the direction bytes and the ops slots; then room for the ten
    # long pairs and some fifty short ones, or for eighty short ones
    fixed = st0.peak_bytes - st0.dir_bytes - sum(n1 + n2 for n1, n2 in live)
    assert fixed > 0
    mem = fixed + 80 * (dir_bytes(12, 12) + 24)
    want_chunks = chunks_of(pairs, dir_bytes, fixed, mem)
    assert len(want_chunks) >= 3 and max(want_chunks) > 64 and sum(want_chunks) == len(live)
    sc, ops, st = align(pairs, mem_bytes=mem)
    assert st.chunks == len(want_chunks) and st.peak_bytes <= mem and st.dir_bytes == st0.dir_bytes
    np.testing.assert_array_equal(sc, sc0)
    same_ops(ops, ops0)


def test_200_pairs_linear():
    scheme = (1, -1, -1)

    def check(pairs, sc, ops):
        full = [k for k, (a, b) in enumerate(pairs) if a.size and b.size]
        tb.check_alignments([pairs[k] for k in full], scheme, sc[full], [ops[k] for k in full])
        for k, (a, b) in enumerate(pairs):
            if k not in full:  # an empty side: all ups or all lefts
                n = max(a.size, b.size)
                assert sc[k] == scheme[2] * n and ops[k].tolist() == [1 if b.size else 2] * n
    check_crowd(crowd(4), lambda p, **kw: nwhip.align_batch(p, scheme, **kw),
                lambda p, **kw: nwhip.score_batch(p, scheme, **kw), check, nwhip.batch_dir_bytes)


def test_200_pairs_affine():
    scheme, go = (1, -1, -1), -3
    check_crowd(crowd(4), lambda p, **kw: nwhip.align_batch_affine(p, scheme, go, **kw),
                lambda p, **kw: nwhip.score_batch_affine(p, scheme, go, **kw),
                lambda p, sc, ops: tba.check_alignments(p, scheme, go, sc, ops), nwhip.batch_affine_dir_bytes)


def test_200_pairs_matrix():
    mat, ge, go = tbm.matrix(20), -1, -11
    check_crowd(crowd(20), lambda p, **kw: nwhip.align_batch_matrix(p, mat, ge, go, **kw),
                lambda p, **kw: nwhip.score_batch_matrix(p, mat, ge, go, **kw),
                lambda p, sc, ops: tbm.check_alignments(p, mat, ge, go, sc, ops), nwhip.batch_affine_dir_bytes)
