"""GPU: banded batched alignment (nw_score_batch_banded, nw_align_batch_banded,
nw_score_batch_banded_async; csrc/nw_batch_banded.hip).

Checker: the plain Python banded Gotoh of tests/nw_banded.py (held to the path definition by
tests/test_batch_banded_host.py); under a covering band also the matrix entries themselves.
All comparisons are exact; no pair is over 2048 on a side.

The grid is tests/test_batch.py's (one lane, a lane boundary, the strip seam, the row-block
boundary, empty sides).  On that grid NO pair is square, and a band that widens by |n2 - n1|
almost never shuts the optimum out: with the checker alone, 0 or 1 of its 43 scores differ
from the global ones at w = 0, 1, 3 for every alphabet and cost used here.  So the grid is
run together with SQUARE, near-square pairs of the same sizes, and it is on those that the
test first asserts that a small w changes most scores.

The directed cases plant the optimum: `zigzag` builds a pair whose best path makes a run of g
lefts, follows diagonal -g, makes 2g ups, follows diagonal +g and returns with g lefts.  At w
= g the path fits exactly and touches both edges of the band; at w = g - 1 it does not fit.
Each case first asserts from the checker alone that moving dlo by one, and dhi by one,
changes the score -- inwards at w = g, outwards at w = g - 1 -- so a kernel whose band is one
diagonal too narrow or too wide on either side cannot pass.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import nw_banded as nb
import nw_gotoh_matrix as gm
import nwhip
from conftest import ROOT, bdna_path, read_bdna
from test_batch import OPS_N1, OPS_N2, _rand, score_pairs
from test_batch_matrix_host import random_matrix

pytestmark = pytest.mark.gpu

I32_MIN = np.iinfo(np.int32).min
COST = [(-1, -11), (-3, 0), (-2, -3), (-2, -11)]  # (ge, go): the local tests'
BANDS = [0, 1, 3, 31, 32, 63, 64, 65, 200, 10 ** 6]
SQUARE = [(5, 5), (63, 63), (64, 64), (65, 65), (130, 130), (255, 255), (256, 256), (257, 257), (257, 256),
          (130, 129), (64, 65)]


@functools.lru_cache(maxsize=None)
def matrix(alpha):
    """Seeded, asymmetric, entries in -8..12, over the bytes 1..alpha."""
    return random_matrix(np.random.default_rng(500 + alpha), alpha)


@functools.lru_cache(maxsize=None)
def related_matrix(alpha=8):
    """5 on the diagonal and an asymmetric -4 / -3 off it.  The planted pairs draw what both
    sequences share from the letters 1..4, what only s1 has from 5 and 6 and what only s2 has
    from 7 and 8: an unshared stretch can only be mismatched or skipped, and skipping (-1 a
    letter) is cheaper than a mismatch (-3 at best for a letter of each), so the planted path is the
    optimum."""
    sc = np.random.default_rng(47).integers(-4, -2, (alpha, alpha))
    sc[np.arange(alpha), np.arange(alpha)] = 5
    return nwhip.SubMatrix(list(range(1, alpha + 1)), sc)


@functools.lru_cache(maxsize=None)
def grid_pairs(alpha):
    rng = np.random.default_rng(900 + alpha)
    return score_pairs(alpha) + tuple((_rand(rng, a, alpha), _rand(rng, b, alpha)) for a, b in SQUARE)


@functools.lru_cache(maxsize=None)
def grid_want(alpha, ge, go, w):
    m = matrix(alpha)
    return np.array([nb.score(a, b, m.scores, m.index, ge, go, w) for a, b in grid_pairs(alpha)], np.int32)


def check_alignments(pairs, mat, ge, go, w, scores, ops):
    for (a, b), sc, o in zip(pairs, scores, ops):
        tables = nb.fill(a, b, mat.scores, mat.index, ge, go, w)
        assert sc == tables[0][-1, -1], (a.size, b.size, w)
        np.testing.assert_array_equal(o, nb.walk(a, b, mat.scores, mat.index, ge, go, w, tables=tables),
                                      err_msg=f"{a.size} x {b.size} ge {ge} go {go} w {w}")
        assert nwhip.ops_score_matrix(a, b, o, mat, ge, go) == sc
        dlo, dhi = nb.limits(a.size, b.size, w)
        assert all(nb.in_band(i, j, dlo, dhi) for i, j in nb.path_vertices(o))


# ------------------------------------------------------------------ the grid
@pytest.mark.parametrize("ge,go", COST)
@pytest.mark.parametrize("alpha", [4, 20, 32])
def test_scores_over_the_grid_and_the_bands(alpha, ge, go):
    pairs, mat = grid_pairs(alpha), matrix(alpha)
    nsq = len(SQUARE)
    glob = np.array([gm.score(a, b, mat.scores, mat.index, ge, go) for a, b in pairs], np.int32)
    for w in (0, 1, 3):  # the band matters: most of the square pairs' scores are not the global ones
        assert (grid_want(alpha, ge, go, w)[-nsq:] != glob[-nsq:]).sum() > nsq // 2, w
    np.testing.assert_array_equal(grid_want(alpha, ge, go, 10 ** 6), glob)
    for w in BANDS:
        want = grid_want(alpha, ge, go, w)
        got, st = nwhip.score_batch_banded(pairs, mat, ge, go, w, return_stats=True)
        np.testing.assert_array_equal(got, want, err_msg=f"w {w}")
        assert st.pairs == len(pairs) and st.chunks == 1 and st.fill_ms > 0
        got, st = nwhip.score_batch_banded(pairs, mat, ge, go, w, waves=3, return_stats=True)
        np.testing.assert_array_equal(got, want, err_msg=f"w {w}, 3 workers")
        assert st.waves == 3


# ------------------------------------------------------------------ a covering band
@pytest.mark.parametrize("ge,go", [(-1, -11), (-2, -3)])
def test_covering_band_is_the_matrix_entries_byte_for_byte(ge, go):
    pairs, mat = grid_pairs(20), matrix(20)
    sc0, ops0, st0 = nwhip.align_batch_matrix(pairs, mat, ge, go)
    sc, ops, st = nwhip.align_batch_banded(pairs, mat, ge, go, 10 ** 6)
    np.testing.assert_array_equal(sc, sc0)
    assert len(ops) == len(ops0)
    for (a, b), x, y in zip(pairs, ops, ops0):
        np.testing.assert_array_equal(x, y, err_msg=f"{a.size} x {b.size}")
    assert st.dir_bytes == st0.dir_bytes
    np.testing.assert_array_equal(nwhip.score_batch_banded(pairs, mat, ge, go, 10 ** 6),
                                  nwhip.score_batch_matrix(pairs, mat, ge, go))
    # the smallest covering band of the longest pair, too
    sc, ops, _ = nwhip.align_batch_banded(pairs, mat, ge, go, 513)
    np.testing.assert_array_equal(sc, sc0)
    for x, y in zip(ops, ops0):
        np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------ ops
@functools.lru_cache(maxsize=None)
def ops_pairs20():
    rng = np.random.default_rng(78)
    sizes = [(a, b) for a in OPS_N1 for b in OPS_N2] + [(200, 200), (256, 257), (600, 601)]
    return tuple((_rand(rng, a, 20), _rand(rng, b, 20)) for a, b in sizes)


@pytest.mark.parametrize("w", [0, 2, 40, 700])
def test_ops_are_the_checkers_walks(w):
    pairs, mat = ops_pairs20(), matrix(20)
    ge, go = -1, -11
    sc, ops, st = nwhip.align_batch_banded(pairs, mat, ge, go, w)
    check_alignments(pairs, mat, ge, go, w, sc, ops)
    assert st.chunks == 1 and st.walk_ms > 0
    assert st.dir_bytes == sum(nwhip.batch_banded_dir_bytes(a.size, b.size, w) for a, b in pairs)
    np.testing.assert_array_equal(nwhip.score_batch_banded(pairs, mat, ge, go, w), sc)


# ------------------------------------------------------------------ planted paths
def _only(rng, n, first):
    """n letters drawn from `first` and `first + 1`."""
    return (rng.integers(0, 2, n) + first).astype(np.int8)


def zigzag(seed, x, g, y, z, v):
    """(a, b): the best path runs x on the diagonal, g lefts, y along diagonal -g, 2g ups, z
    along diagonal +g, g lefts, v on the diagonal.  n1 = n2 = x + y + z + v + 2g."""
    rng = np.random.default_rng(seed)
    X, Y, Z, V = (_rand(rng, n, 4) for n in (x, y, z, v))
    I1, I2, I3 = _only(rng, g, 5), _only(rng, 2 * g, 7), _only(rng, g, 5)
    return np.concatenate([X, I1, Y, Z, I3, V]), np.concatenate([X, Y, I2, Z, V])


def assert_both_edges_matter(a, b, mat, ge, go, w, step):
    """From the checker alone: moving dlo by `step` towards (+1 at the fitting band) or away
    from (-1 at the band one short) the diagonal changes the score, and dhi likewise."""
    dlo, dhi = nb.limits(a.size, b.size, w)
    sc = nb.score(a, b, mat.scores, mat.index, ge, go, dlo=dlo, dhi=dhi)
    assert nb.score(a, b, mat.scores, mat.index, ge, go, dlo=dlo + step, dhi=dhi) != sc, ("dlo", a.size, b.size, w)
    assert nb.score(a, b, mat.scores, mat.index, ge, go, dlo=dlo, dhi=dhi - step) != sc, ("dhi", a.size, b.size, w)


def run_planted(pairs_w, mat, ge, go, waves=0, outwards=True):
    """pairs_w: [(a, b, g)]; each at w = g (edges inwards) and w = g - 1 (edges outwards)."""
    for a, b, g in pairs_w:
        assert_both_edges_matter(a, b, mat, ge, go, g, +1)
        if outwards:
            assert_both_edges_matter(a, b, mat, ge, go, g - 1, -1)
        for w in (g, g - 1):
            sc, ops, _ = nwhip.align_batch_banded([(a, b)], mat, ge, go, w, waves=waves)
            check_alignments([(a, b)], mat, ge, go, w, sc, ops)
            assert nwhip.score_batch_banded([(a, b)], mat, ge, go, w, waves=waves)[0] == sc[0]


# the edges run along the path's y and z segments: with x = 100 the dlo edge is followed over
# columns 100 + g .. 100 + g + y and the dhi edge over the columns after them, so both cross
# the seams 256 / 257 and 512 / 513 and every row residue mod 64; n1 >= 513: three strips
@pytest.mark.parametrize("g", [1, 2, 31, 32, 33, 63, 64, 65])
def test_both_band_edges_across_seams_and_row_blocks(g):
    mat = related_matrix()
    a, b = zigzag(300 + g, 100, g, 320, 330, 20)
    assert a.size == b.size >= 513 + 2 * g
    run_planted([(a, b, g)], mat, -1, -3)


def test_paths_that_hug_the_edges_and_long_runs_across_a_seam():
    """g = 300: runs of 300 lefts (columns 150 .. 450 over the seam 256 / 257) and of 600 ups
    inside the band; the path follows each edge for 300 cells."""
    mat = related_matrix()
    a, b = zigzag(77, 150, 300, 300, 300, 50)
    assert a.size == b.size == 1400
    want = nb.walk(a, b, mat.scores, mat.index, -1, -3, 300)
    assert gm.path_score(a, b, want, mat.scores, mat.index, -1, -3) == 5 * 800 - 3 * 3 - 1200
    v = nb.path_vertices(want)
    assert sum(i - j == -300 for i, j in v) > 300 and sum(i - j == 300 for i, j in v) > 300
    run_planted([(a, b, 300)], mat, -1, -3)


def test_edge_on_rows_63_64_65():
    """The dhi edge enters at row x + y + 2g of column x + g + y and the dlo edge at row x: with
    x = 63, 64, 65 and one lane's columns the first edge cells sit on the last rows of block 0
    and the first of block 1."""
    mat = related_matrix()
    run_planted([zigzag(500 + x, x, 3, 40, 40, 30) + (3,) for x in (63, 64, 65)], mat, -1, -3)
    run_planted([zigzag(510 + x, x - 7, 7, 20, 20, 10) + (7,) for x in (63, 64, 65)], mat, -2, -1)


@pytest.mark.parametrize("tall", [False, True])
def test_tall_and_wide_pairs_widened_by_delta(tall):
    """40 x 700 and 700 x 40: core(30) between two junk runs against core + 660 more.  The best
    path leaves the corner diagonal by g = 5 on one side at the start and on the other at the
    end, beyond the |delta| the band already grants.  (At w = 4 the two ends are not
    independent -- what the start is forced into changes what the end needs -- so the outward
    assertion is made at the fitting band only; w = 4 is compared all the same.)"""
    rng = np.random.default_rng(91)
    mat = related_matrix()
    core, j1, j2, r = _rand(rng, 30, 4), _only(rng, 5, 5), _only(rng, 5, 5), _only(rng, 670, 7)
    short, long_ = np.concatenate([j1, core, j2]), np.concatenate([core, r])
    a, b = (long_, short) if tall else (short, long_)
    assert sorted((a.size, b.size)) == [40, 700]
    run_planted([(a, b, 5)], mat, -1, -3, outwards=False)


def test_one_column_one_row_and_a_one_lane_last_strip():
    rng = np.random.default_rng(92)
    mat = matrix(20)
    pairs = [(_rand(rng, 1, 20), _rand(rng, 1, 20)), (_rand(rng, 1, 20), _rand(rng, 200, 20)),
             (_rand(rng, 200, 20), _rand(rng, 1, 20)), (_rand(rng, 257, 20), _rand(rng, 257, 20)),
             (_rand(rng, 513, 20), _rand(rng, 500, 20)), (_rand(rng, 260, 20), _rand(rng, 1, 20))]
    for w in (0, 1, 5, 64):
        sc, ops, _ = nwhip.align_batch_banded(pairs, mat, -1, -11, w)
        check_alignments(pairs, mat, -1, -11, w, sc, ops)
    # 257 columns, one lane in the last strip, and the path planted through it
    a, b = zigzag(94, 60, 4, 80, 80, 29)
    assert a.size == 257
    run_planted([(a, b, 4)], related_matrix(), -1, -3)


# ------------------------------------------------------------------ stale data
def test_short_narrow_pair_after_a_long_wide_one_on_one_worker():
    """waves = 1: the scratch holds the long pair's columns (every row written, wide band) when
    the short pair (narrow band, three strips) reads only its band's rows of it."""
    rng = np.random.default_rng(95)
    mat = related_matrix()
    long_ = (_rand(rng, 1100, 8), _rand(rng, 1000, 8))
    a, b = zigzag(96, 100, 2, 320, 330, 20)
    pairs = [long_, (a, b), (_rand(rng, 600, 8), _rand(rng, 590, 8))]
    for w in (2, 1, 0):
        sc, ops, st = nwhip.align_batch_banded(pairs, mat, -1, -3, w, waves=1)
        assert st.waves == 1
        check_alignments(pairs, mat, -1, -3, w, sc, ops)
        got = nwhip.score_batch_banded(pairs, mat, -1, -3, w, waves=1)
        np.testing.assert_array_equal(got, sc)
    # a covering band first, a narrow one after it, on the same context: the direction blocks,
    # the scratch and the profile are all reused
    sc, ops, _ = nwhip.align_batch_banded(pairs, mat, -1, -3, 10 ** 6, waves=1)
    check_alignments(pairs, mat, -1, -3, 10 ** 6, sc, ops)
    sc, ops, _ = nwhip.align_batch_banded(pairs[1:], mat, -1, -3, 2, waves=1)
    check_alignments(pairs[1:], mat, -1, -3, 2, sc, ops)


def test_strip_range_reaches_rows_the_strip_before_never_wrote():
    """1500 x 1500 at w = 2: strip p + 1 starts at row 256 (p + 1) - 3 while strip p stopped
    writing its right column 320 rows further down at the latest; the blocks strip p + 1 loads
    ahead lie beyond what strip p wrote, and below the band everything it reads must be -inf.
    Before it on the same worker a pair whose values would win: all matches, no gaps."""
    rng = np.random.default_rng(97)
    mat = related_matrix()
    same = _rand(rng, 1500, 4)
    a, b = zigzag(98, 400, 2, 500, 500, 96)
    assert a.size == 1500
    pairs = [(same, same.copy()), (a, b)]
    for w in (2, 1):
        sc, ops, st = nwhip.align_batch_banded(pairs, mat, -1, -3, w, waves=1)
        assert st.waves == 1 and sc[0] == 5 * 1500
        check_alignments(pairs, mat, -1, -3, w, sc, ops)
    assert_both_edges_matter(a, b, mat, -1, -3, 2, +1)
    assert_both_edges_matter(a, b, mat, -1, -3, 1, -1)


# ------------------------------------------------------------------ wide matrix, int8 span
@pytest.mark.parametrize("ge,go", [(-1, -11), (-64, -11), (0, -3), (1, -1)])
def test_full_int8_span(ge, go):
    """A matrix holding -128 and 127 (the matrix tests' case): the table byte s - 2 ge leaves
    int8 for three of the four gaps, and the kernel's wide form runs under the mask."""
    rng = np.random.default_rng(41)
    sc = rng.integers(-128, 128, (8, 8))
    sc[0, 1], sc[1, 0], sc[3, 3], sc[5, 2] = -128, 127, 127, -128
    mat = nwhip.SubMatrix(list(range(1, 9)), sc)
    pairs = [(_rand(rng, 257, 8), _rand(rng, 255, 8)), (_rand(rng, 513, 8), _rand(rng, 520, 8))]
    for w in (0, 3, 70):
        s, ops, _ = nwhip.align_batch_banded(pairs, mat, ge, go, w)
        check_alignments(pairs, mat, ge, go, w, s, ops)
        assert nwhip.score_batch_banded(pairs, mat, ge, go, w).tolist() == s.tolist()


# ------------------------------------------------------------------ chunks and memory
def test_chunks_replayed_from_the_dir_bytes():
    rng = np.random.default_rng(23)
    mat = matrix(20)
    pairs = [(_rand(rng, int(rng.integers(600, 641)), 20), _rand(rng, int(rng.integers(600, 640)), 20))
             for _ in range(30)]
    ge, go, w = -1, -11, 8
    sc0, ops0, st0 = nwhip.align_batch_banded(pairs, mat, ge, go, w)
    db = [nwhip.batch_banded_dir_bytes(a.size, b.size, w) for a, b in pairs]
    assert st0.chunks == 1 and st0.dir_bytes == sum(db)
    assert sum(db) < sum(nwhip.batch_affine_dir_bytes(a.size, b.size) for a, b in pairs)
    want = [nb.score(a, b, mat.scores, mat.index, ge, go, w) for a, b in pairs]
    assert sc0.tolist() == want
    # 11 pairs' worth of direction bytes for 30 pairs: three chunks at the least
    mem = 11 * max(db)
    sc, ops, st = nwhip.align_batch_banded(pairs, mat, ge, go, w, mem_bytes=mem)
    assert st.chunks >= 3 and st.peak_bytes <= mem and st.dir_bytes == st0.dir_bytes
    assert sc.tolist() == want
    for x, y in zip(ops, ops0):
        np.testing.assert_array_equal(x, y)
    check_alignments(pairs[:3], mat, ge, go, w, sc[:3], ops[:3])
    # below one pair's direction bytes: that pair does not fit
    with pytest.raises(nwhip.NwError) as e:
        nwhip.align_batch_banded(pairs, mat, ge, go, w, mem_bytes=min(db) - 1)
    assert e.value.status == nwhip.NW_ERR_OOM


def test_a_pair_the_matrix_entry_cannot_hold_fits_with_a_band():
    """2000 x 2000: 8 strips x 33 iterations x 8 KiB = 2.2 MB of directions for the whole table,
    8 x 8 x 8 KiB = 0.5 MB at w = 4.  With 1 MB the matrix entry answers NW_ERR_OOM and the
    banded one aligns the pair."""
    mat = related_matrix()
    a, b = zigzag(99, 600, 4, 500, 500, 392)
    assert a.size == b.size == 2000
    full, banded = nwhip.batch_affine_dir_bytes(2000, 2000), nwhip.batch_banded_dir_bytes(2000, 2000, 4)
    assert (full, banded) == (8 * 33 * 8192, 8 * 8 * 8192)
    mem = 1 << 20
    with pytest.raises(nwhip.NwError) as e:
        nwhip.align_batch_matrix([(a, b)], mat, -1, -3, mem_bytes=mem)
    assert e.value.status == nwhip.NW_ERR_OOM
    sc, ops, st = nwhip.align_batch_banded([(a, b)], mat, -1, -3, 4, mem_bytes=mem)
    assert st.dir_bytes == banded and st.peak_bytes <= mem
    check_alignments([(a, b)], mat, -1, -3, 4, sc, ops)
    with pytest.raises(nwhip.NwError) as e:
        nwhip.align_batch_banded([(a, b)], mat, -1, -3, 4, mem_bytes=banded - 1)
    assert e.value.status == nwhip.NW_ERR_OOM


# ------------------------------------------------------------------ device API
def test_context_score_batch_banded_on_a_stream():
    import torch
    ge, go, w = -2, -3, 3
    mat = nwhip.SubMatrix(matrix(20).letters, matrix(20).scores, other=1)
    # longest first, as the device entry asks; empty sides are answered by the kernel
    pairs = sorted(grid_pairs(20), key=lambda p: -p[0].size * p[1].size)
    assert sum(a.size == 0 or b.size == 0 for a, b in pairs) == 3
    want = np.array([nb.score(a, b, mat.scores, mat.index, ge, go, w) for a, b in pairs], np.int32)
    s1, off1, s2, off2 = nwhip.batch_csr(pairs)
    max_n2 = max(b.size for _, b in pairs)
    ctx = nwhip.Context(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = [torch.from_numpy(x).cuda() for x in (s1, off1, s2, off2)]
        got = ctx.score_batch_banded(d[0], d[1], d[2], d[3], max_n2, mat, ge, go, w, stream=stream)
        got2 = ctx.score_batch_banded(d[0], d[1], d[2], d[3], max_n2 + 70, mat, ge, go, w, stream=stream, waves=2)
        full = ctx.score_batch_matrix(d[0], d[1], d[2], d[3], max_n2, mat, ge, go, stream=stream)
        cover = ctx.score_batch_banded(d[0], d[1], d[2], d[3], max_n2, mat, ge, go, 10 ** 6, stream=stream)
        low = ctx.score_batch_banded(d[0], d[1], d[2], d[3], 65, mat, ge, go, w, stream=stream)
    stream.synchronize()
    assert ctx.status(stream) == nwhip.NW_OK
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(got2.cpu().numpy(), want)
    np.testing.assert_array_equal(cover.cpu().numpy(), full.cpu().numpy())
    # max_n2 below a pair's rows: that pair is refused (INT32_MIN), the others computed
    low = low.cpu().numpy()
    n2 = np.diff(off2)
    assert (n2 > 65).any()
    np.testing.assert_array_equal(low[n2 <= 65], want[n2 <= 65])
    assert (low[n2 > 65] == I32_MIN).all()
    with pytest.raises(ValueError):
        ctx.score_batch_banded(d[0], d[1], d[2], d[3], 65, matrix(20), ge, go, w, stream=stream)
    ctx.close()


def test_empty_sides():
    mat = matrix(4)
    ones, twos = (lambda n: np.full(n, 1, np.int8)), (lambda n: np.full(n, 2, np.int8))
    pairs = [(ones(0), twos(9)), (ones(9), twos(0)), (ones(0), twos(0)), (ones(3), twos(2))]
    for w in (0, 2):
        sc, ops, _ = nwhip.align_batch_banded(pairs, mat, -2, -5, w)
        assert sc[:3].tolist() == [-5 - 18, -5 - 18, 0]
        assert ops[0].tolist() == [1] * 9 and ops[1].tolist() == [2] * 9 and ops[2].size == 0
        check_alignments(pairs, mat, -2, -5, w, sc, ops)
        assert nwhip.score_batch_banded(pairs, mat, -2, -5, w).tolist() == sc.tolist()


# ------------------------------------------------------------------ CLI
MATRIX_TEXT = """# bytes 1..4 of the .bdna files and a wildcard; asymmetric
     0x01 0x02 0x03 0x04 *
0x01    5   -4   -3   -4   1
0x02   -2    5   -4   -1   1
0x03   -4   -4    6   -4   1
0x04   -3   -1   -4    5   1
*       0    0    0    0   1
"""


@pytest.mark.parametrize("extra", [[], ["--score-only"]])
@pytest.mark.parametrize("w", [0, 2, 100000])
def test_cli_batch_band(tmp_path, golden, extra, w):
    names = ["small", "debug", "t"]
    files = [(golden["pairs"][n]["argv1"], golden["pairs"][n]["argv2"]) for n in names]
    lst = tmp_path / "pairs.txt"
    lst.write_text("".join(f"{bdna_path(a)} {bdna_path(b)}\n" for a, b in files))
    mfile = tmp_path / "matrix.txt"
    mfile.write_text(MATRIX_TEXT)
    exe = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")
    r = subprocess.run([exe, "--batch", str(lst), "--scheme", "1,-1,-2", "--matrix", str(mfile), "--gap-open", "-11",
                        "--band", str(w)] + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    int(lines[0])  # the wall time, ms
    mat = nwhip.SubMatrix.from_text(str(mfile))
    pairs = [(read_bdna(a), read_bdna(b)) for a, b in files]
    want = [nb.score(a, b, mat.scores, mat.index, -2, -11, w) for a, b in pairs]
    assert lines[1:4] == [f"Score: {x}" for x in want]
