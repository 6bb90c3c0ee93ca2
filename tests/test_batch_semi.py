"""GPU: batched semi-global alignment -- Gotoh with a substitution matrix and free end gaps
per side (nw_score_batch_semi, nw_align_batch_semi, nw_score_batch_semi_async;
csrc/nw_batch_semi.hip).

Checker: the plain Python table, end cell and walk of tests/nw_semi.py (held to the path
definition by tests/test_batch_semi_host.py); with ends = 0 also the matrix entries
themselves, byte for byte.  All comparisons are of integers and bytes, exact.  The shapes
are tests/test_batch.py's -- one lane, a lane boundary, a strip seam (255 / 256 / 257
columns, three strips at 513), a row-block boundary (63 / 64 / 65 rows, three blocks at
130), empty sides -- plus constructions that put the end cell where a random pair never
does: in every strip, on the corner, in every row block of column n1, on a tie across two
strips, on a tie down a column, next to columns past n1 that would outscore it; walks that
run along a boundary that is not free; the 300-long runs over the seams.  Every
construction asserts its geometry from the checker before the library is called.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import nw_semi as ns
import nwhip
from conftest import ROOT
from test_batch import OPS_N1, OPS_N2, SCORE_N1, SCORE_N2, _rand
from test_batch_local import COST, matrix, mutate, planted

pytestmark = pytest.mark.gpu

I32_MIN = np.iinfo(np.int32).min
ENDS = [0, 3, 12, 9, 6, 15, 2, 8, 1, 4]


@functools.lru_cache(maxsize=None)
def grid_matrix(alpha):
    """Seeded and asymmetric over the bytes 1..alpha: 4..11 on the diagonal, -8..-1 off it --
    but -8 wherever one of the last two letters meets another letter: below every ge here,
    so a gap is always cheaper than aligning such a letter (score_pairs' end pieces)."""
    rng = np.random.default_rng(1200 + alpha)
    sc = rng.integers(-8, 0, (alpha, alpha))
    sc[alpha - 2:, :] = sc[:, alpha - 2:] = -8
    sc[np.arange(alpha), np.arange(alpha)] = rng.integers(4, 12, alpha)
    assert (sc != sc.T).any()
    return nwhip.SubMatrix(list(range(1, alpha + 1)), sc)


@functools.lru_cache(maxsize=None)
def score_pairs(alpha):
    """The cross product of the sizes plus the empty sides, shuffled.  Where both sides have
    60 letters, every free end has something to skip: the cores are drawn from the letters
    1 .. alpha - 2, s2's core is a mutated piece of s1's, s1 begins with 6 and ends with 4
    letters alpha - 1, s2 begins with 3 and ends with 7 letters alpha (under grid_matrix those
    letters cost more aligned than skipped by a gap, whatever stands against them)."""
    rng = np.random.default_rng(1100 + alpha)
    pairs = []
    for n1 in SCORE_N1:
        for n2 in SCORE_N2:
            if n1 >= 60 and n2 >= 60:
                a = _rand(rng, n1, alpha - 2)
                a[:6], a[-4:] = alpha - 1, alpha - 1
                seg = min(n1, n2) - 10
                at = int(rng.integers(6, n1 - 4 - seg + 1))
                b = np.full(n2, alpha, np.int8)
                b[3:3 + seg] = mutate(rng, a[at:at + seg], alpha - 2, subs=0.1)
                if n2 - 10 > seg:
                    b[3 + seg:n2 - 7] = _rand(rng, n2 - 10 - seg, alpha - 2)
                pairs.append((a, b))
            else:
                pairs.append((_rand(rng, n1, alpha), _rand(rng, n2, alpha)))
    pairs += [(_rand(rng, 0, alpha), _rand(rng, 7, alpha)), (_rand(rng, 7, alpha), _rand(rng, 0, alpha)),
              (_rand(rng, 0, alpha), _rand(rng, 0, alpha))]
    return tuple(pairs[i] for i in rng.permutation(len(pairs)))


def want_hit(a, b, mat, ge, go, ends):
    return ns.end_cell(ns.fill(a, b, mat.scores, mat.index, ge, go, ends)[0], ends)


@functools.lru_cache(maxsize=None)
def score_want(alpha, ge, go, ends):
    m = grid_matrix(alpha)
    return np.array([want_hit(a, b, m, ge, go, ends) for a, b in score_pairs(alpha)], np.int32)


def hit_rows(hits):
    return np.stack([hits["score"], hits["end_i"], hits["end_j"]], axis=1)


def check_alignments(pairs, mat, ge, go, ends, hits, ops):
    """Hits, begin cells and ops against the checker; returns the checker's (score, begin,
    end, ops) per pair."""
    out = []
    for (a, b), h, o in zip(pairs, hits, ops):
        tables = ns.fill(a, b, mat.scores, mat.index, ge, go, ends)
        sc, ei, ej = ns.end_cell(tables[0], ends)
        want, begin = ns.walk(a, b, mat.scores, mat.index, ge, go, ends, tables)
        what = f"{a.size} x {b.size} ge {ge} go {go} ends {ends}"
        assert (h["score"], h["end_i"], h["end_j"]) == (sc, ei, ej), what
        assert (h["begin_i"], h["begin_j"]) == begin, what
        assert (h["reserved"] == 0).all()
        np.testing.assert_array_equal(o, want, err_msg=what)
        assert o.size <= a.size + b.size
        assert nwhip.ops_score_matrix(a, b, o, mat, ge, go, begin=begin) == sc
        assert ns.path_score(a, b, o, begin, mat.scores, mat.index, ge, go) == (sc, (ei, ej))
        out.append((sc, begin, (ei, ej), want))
    return out


def align_and_check(pairs, mat, ge, go, ends, **kw):
    hits, ops, st = nwhip.align_batch_semi(pairs, mat, ge, go, ends, **kw)
    want = check_alignments(pairs, mat, ge, go, ends, hits, ops)
    # the score entry finds the same hits, and no begin cell
    got = nwhip.score_batch_semi(pairs, mat, ge, go, ends, waves=kw.get("waves", 0))
    np.testing.assert_array_equal(hit_rows(got), hit_rows(hits))
    assert (got["begin_i"] == -1).all() and (got["begin_j"] == -1).all() and (got["reserved"] == 0).all()
    return hits, ops, st, want


# ------------------------------------------------------------------ scores and end cells
@pytest.mark.parametrize("ends", ENDS)
@pytest.mark.parametrize("ge,go", COST)
@pytest.mark.parametrize("alpha", [4, 20, 32])
def test_hits_at_the_pairs_own_index(alpha, ge, go, ends):
    pairs, mat = score_pairs(alpha), grid_matrix(alpha)
    want = score_want(alpha, ge, go, ends)
    if ends != 0:  # the free ends matter on this batch -- judged on the checker's results alone
        assert 2 * (want != score_want(alpha, ge, go, 0)).any(axis=1).sum() > len(pairs)
    got, st = nwhip.score_batch_semi(pairs, mat, ge, go, ends, return_stats=True)
    np.testing.assert_array_equal(hit_rows(got), want)
    assert (got["begin_i"] == -1).all() and (got["begin_j"] == -1).all() and (got["reserved"] == 0).all()
    assert st.pairs == len(pairs) and st.cells == sum(a.size * b.size for a, b in pairs)
    assert st.chunks == 1 and 1 <= st.waves <= len(pairs) - 3 and st.fill_ms > 0
    # waves = 3: every worker sweeps a dozen pairs one after the other, so a best cell or a
    # call count that is not reset per strip and per pair fails here
    got, st = nwhip.score_batch_semi(pairs, mat, ge, go, ends, waves=3, return_stats=True)
    np.testing.assert_array_equal(hit_rows(got), want)
    assert st.waves == 3
    if ends == 0:
        want0 = nwhip.score_batch_matrix(pairs, mat, ge, go)
        np.testing.assert_array_equal(got["score"], want0)
        n1 = np.array([a.size for a, _ in pairs])
        n2 = np.array([b.size for _, b in pairs])
        np.testing.assert_array_equal(got["end_i"], n2)
        np.testing.assert_array_equal(got["end_j"], n1)


# ------------------------------------------------------------------ ops
@functools.lru_cache(maxsize=None)
def ops_pairs():
    """Over 20 letters: OPS_N1 x OPS_N2; where both sides have 60 letters a mutated segment of
    s1 stands in s2, so that the free ends have something to skip."""
    rng = np.random.default_rng(1000)
    pairs = []
    for n1 in OPS_N1:
        for n2 in OPS_N2:
            if n1 >= 60 and n2 >= 60:
                seg = min(n1, n2) * 2 // 3
                pairs.append(planted(rng, n1, n2, 20, int(rng.integers(0, n1 - seg + 1)), seg,
                                     int(rng.integers(0, n2 - seg + 1)), [("d", 3), ("i", 2)], 0.1))
            else:
                pairs.append((_rand(rng, n1, 20), _rand(rng, n2, 20)))
    pairs += [(_rand(rng, 0, 20), _rand(rng, 7, 20)), (_rand(rng, 7, 20), _rand(rng, 0, 20)),
              (_rand(rng, 0, 20), _rand(rng, 0, 20))]
    return tuple(pairs)


@pytest.mark.parametrize("ends", ENDS)
@pytest.mark.parametrize("ge,go", [(-1, -11), (-2, -3)])
def test_ops_are_the_walks_from_the_end_cell(ge, go, ends):
    pairs, mat = ops_pairs(), matrix(20)
    hits, ops, st, want = align_and_check(pairs, mat, ge, go, ends)
    assert st.chunks == 1
    assert st.dir_bytes == sum(nwhip.batch_affine_dir_bytes(a.size, b.size) for a, b in pairs)
    assert st.peak_bytes > st.dir_bytes and st.walk_ms > 0
    assert any((o == 1).any() and (o == 2).any() for _, _, _, o in want)
    if ends == 0:
        sc0, ops0, _ = nwhip.align_batch_matrix(pairs, mat, ge, go)
        np.testing.assert_array_equal(hits["score"], sc0)
        for (a, b), h, x, y in zip(pairs, hits, ops, ops0):
            assert x.tobytes() == y.tobytes()
            assert tuple(h)[1:5] == (b.size, a.size, 0, 0)
    else:
        base =[want_hit(a, b, mat, ge, go, 0) for a, b in pairs]
        differ = sum((sc, ei, ej) != g or begin != (0, 0) for (sc, begin, (ei, ej), _), g in zip(want, base))
        assert 2 * differ > len(pairs)
        if ends & 5:
            assert sum(begin != (0, 0) for _, begin, _, _ in want) >= 8
        if ends & 10:
            assert sum(end != (b.size, a.size) for (a, b), (_, _, end, _) in zip(pairs, want)) >= 8


def test_empty_sides_follow_the_definition():
    """The host answers them without a launch, ops included; alone in a batch nothing is
    launched at all."""
    mat = matrix(4)
    e = np.zeros(0, np.int8)
    pairs = [(e, _rand(np.random.default_rng(1), 7, 4)), (_rand(np.random.default_rng(2), 6, 4), e), (e, e)]
    for ends in range(16):
        for ge, go in COST:
            hits, ops, st, want = align_and_check(pairs, mat, ge, go, ends)
            assert st.chunks == 0 and st.dir_bytes == 0
            # 0 x 7: column 0 alone.  The end is (7, 0) unless bit 8 frees it: then (0, 0) wins
            sc, begin, end, o = want[0]
            assert end == ((0, 0) if ends & 8 else (7, 0))
            assert sc == (0 if ends & 12 else go + 7 * ge)
            assert o.tolist() == ([] if ends & 12 else [1] * 7)
            sc, begin, end, o = want[1]
            assert end == ((0, 0) if ends & 2 else (0, 6))
            assert sc == (0 if ends & 3 else go + 6 * ge)
            assert o.tolist() == ([] if ends & 3 else [2] * 6)
            assert want[2][:3] == (0, (0, 0), (0, 0))


# ------------------------------------------------------------------ directed geometry
@pytest.mark.parametrize("ge,go", COST)
@pytest.mark.parametrize("alpha", [4, 20])
def test_end_cell_in_every_strip_and_on_the_corner(alpha, ge, go):
    """s2 is a mutated copy of 130 letters of a 513-letter s1, all of s2 inside s1: the end
    cell is on row n2 in strip 0, in strip 1, on column 512 and on the corner (130, 513)."""
    rng = np.random.default_rng(1001 + alpha)
    mat = matrix(alpha)
    a = _rand(rng, 513, alpha)
    ats = [40, 300, 382, 383]
    pairs = [(a, mutate(rng, a[at:at + 130], alpha)) for at in ats]
    for (x, y), at in zip(pairs, ats):
        assert y.size == 130
        assert want_hit(x, y, mat, ge, go, 3)[1:] == (130, at + 130)
    hits, ops, _, want = align_and_check(pairs, mat, ge, go, 3)
    assert [w[2] for w in want] == [(130, 170), (130, 430), (130, 512), (130, 513)]
    assert [w[1] for w in want] == [(0, at) for at in ats]


@pytest.mark.parametrize("ge,go", COST)
@pytest.mark.parametrize("alpha", [4, 20])
def test_end_row_in_every_row_block_of_column_n1(alpha, ge, go):
    """s1 (5 letters: one lane and a bit; 257: a second strip) stands in a random s2 of 200 +
    n1 letters, all of s1 inside s2: the end cell is on column n1 in row block 0, 1, 2 and up."""
    rng = np.random.default_rng(1002 + alpha)
    mat = matrix(alpha)
    pairs, rows = [], []
    for n1 in (5, 257):
        for at in (30, 90, 150):
            a = _rand(rng, n1, alpha)
            b = _rand(rng, 200 + n1, alpha)
            b[at:at + n1] = a
            pairs.append((a, b))
            rows.append(at + n1)
    assert rows == [35, 95, 155, 287, 347, 407]
    for (a, b), r in zip(pairs, rows):
        assert want_hit(a, b, mat, ge, go, 12)[1:] == (r, a.size)
    hits, ops, _, want = align_and_check(pairs, mat, ge, go, 12)
    assert [w[2][0] for w in want] == rows
    assert [w[1] for w in want] == [(r - a.size, 0) for (a, _), r in zip(pairs, rows)]
    assert sorted({w[2][0] // 64 for w in want}) == [0, 1, 2, 4, 5, 6]


@pytest.mark.parametrize("ge,go", COST)
@pytest.mark.parametrize("alpha", [4, 20])
def test_tie_across_two_strips(alpha, ge, go):
    rng = np.random.default_rng(1003 + alpha)
    mat = matrix(alpha)
    x = _rand(rng, 130, alpha)
    a = np.concatenate([x, x])
    H = ns.fill(a, x, mat.scores, mat.index, ge, go, 3)[0]
    assert H[130, 130] == H[130, 260] == H[130].max()
    assert ns.end_cell(H, 3)[1:] == (130, 130)
    pairs = [(a, x), (np.concatenate([x, x, x, x]), x)]  # (and across strips 0, 1 and 2)
    hits, _, _, want = align_and_check(pairs, mat, ge, go, 3)
    assert [w[2] for w in want] == [(130, 130), (130, 130)]
    assert [w[1] for w in want] == [(0, 0), (0, 0)]


@pytest.mark.parametrize("ge,go", COST)
@pytest.mark.parametrize("alpha", [4, 20])
def test_tie_down_a_column_and_columns_past_n1(alpha, ge, go):
    """One letter throughout, 5 columns against 100 rows.  With every end free, column 5
    holds 5 s from row 5 on and the earliest row wins; with only s1's end free the score is
    negative, while the three columns past n1 in the lane hold hundreds."""
    mat = matrix(alpha)
    s = int(mat.scores[0, 0])
    pairs = [(np.full(5, 1, np.int8), np.full(100, 1, np.int8))] * 2
    H = ns.fill(*pairs[0], mat.scores, mat.index, ge, go, 15)[0]
    assert (H[5:, 5] == 5 * s).all() and H[100, 5] == 5 * s and H[:5, 5].max() < 5 * s
    assert ns.end_cell(H, 15) == (5 * s, 5, 5)
    hits, _, _, want = align_and_check(pairs, mat, ge, go, 15)
    assert [w[0] for w in want] == [5 * s] * 2 and [w[2] for w in want] == [(5, 5)] * 2
    sc, ei, ej = want_hit(*pairs[0], mat, ge, go, 2)
    assert sc < 0 and (ei, ej) == (100, 5) and 8 * s > 30
    hits, _, _, want = align_and_check(pairs, mat, ge, go, 2)
    assert [w[0] for w in want] == [sc] * 2
    # a column in the middle of a lane as n1, next to a strip seam: 258 columns
    pairs = [(np.full(258, 1, np.int8), np.full(70, 1, np.int8))]
    for ends in (15, 2, 8, 10):
        align_and_check(pairs, mat, ge, go, ends)


@pytest.mark.parametrize("ge,go", COST)
@pytest.mark.parametrize("alpha", [4, 20])
def test_walks_that_reach_a_boundary_that_is_not_free(alpha, ge, go):
    """ends = 2 / 8: the begin cell is (0, 0), so the ops begin with the run of lefts / ups in
    front of the segment, charged go once.  The long side is one letter that the segment
    does not hold, so the 70-long run and the 60 diagonals are the only good path."""
    rng = np.random.default_rng(1005 + alpha)
    mat = matrix(alpha)
    a = np.full(300, alpha, np.int8)
    seg = _rand(rng, 60, alpha - 1)
    a[70:130] = seg
    for ends, pair, op in ((2, (a, seg), 2), (8, (seg, a), 1)):
        hits, ops, _, want = align_and_check([pair, pair], mat, ge, go, ends)
        sc, begin, end, o = want[0]
        assert begin == (0, 0) and end == ((60, 130) if ends == 2 else (130, 60))
        assert o.tolist() == [op] * 70 + [0] * 60
        diag = int(mat.scores[mat.index[seg.view(np.uint8)], mat.index[seg.view(np.uint8)]].sum())
        assert sc == go + 70 * ge + diag
        assert nwhip.ops_score_matrix(*pair, ops[0], mat, ge, go, begin=(0, 0)) == hits["score"][0] == sc


def test_short_pair_after_a_long_one_on_the_same_worker():
    """One worker: 513 x 130 with its end cell in strip 1 (three strips: profile, scratch,
    column bests and the lane's best all used), then 5 x 130, 257 x 1 and 3 x 2."""
    rng = np.random.default_rng(1006)
    mat = matrix(20)
    a = _rand(rng, 513, 20)
    pairs = [(_rand(rng, 257, 20), _rand(rng, 1, 20)), (a, mutate(rng, a[300:430], 20)),
             (_rand(rng, 5, 20), _rand(rng, 130, 20)), (_rand(rng, 3, 20), _rand(rng, 2, 20))]
    for ends in (3, 12, 15, 6):
        hits, ops, st, want = align_and_check(pairs, mat, -1, -11, ends, waves=1)
        assert st.waves == 1
        if ends == 3:
            assert want[1][2] == (130, 430) and want[1][0] > 300 > max(want[2][0], want[3][0], want[0][0])


def test_gap_runs_over_the_seams():
    """300 lefts over the strip seam and 300 ups over the row blocks inside a fit (ends = 3),
    under go = -11: with 100 per match the two halves are worth the gap between them."""
    mat = nwhip.SubMatrix.uniform([1, 2, 3, 4], 100, -100)
    rng = np.random.default_rng(1007)
    P, Q = rng.integers(3, 5, 10).astype(np.int8), rng.integers(3, 5, 10).astype(np.int8)
    a = np.full(400, 1, np.int8)
    a[50:60], a[360:370] = P, Q
    b = np.concatenate([P, Q])
    c = np.full(60, 1, np.int8)
    c[20:40] = b
    d = np.concatenate([P, np.full(300, 2, np.int8), Q])
    pairs = [(a, b), (c, d)]
    hits, ops, _, want = align_and_check(pairs, mat, -1, -11, 3)
    assert hits["score"].tolist() == [2000 - 311, 2000 - 311]
    assert want[0][1] == (0, 50) and want[0][2] == (20, 370)
    assert want[1][1] == (0, 20) and want[1][2] == (320, 40)
    np.testing.assert_array_equal(ops[0], [0] * 10 + [2] * 300 + [0] * 10)
    np.testing.assert_array_equal(ops[1], [0] * 10 + [1] * 300 + [0] * 10)


# ------------------------------------------------------------------ the int8 span
@pytest.mark.parametrize("ends", [3, 15, 6])
@pytest.mark.parametrize("top", [127, 125])
def test_int8_span(top, ends):
    """ge = -1: the table byte is s + 2.  With an entry of 127 it leaves int8 and the kernel
    adds -2 ge per cell (the wide form); with 125 the bytes reach 127 and -126 exactly."""
    rng = np.random.default_rng(1008)
    sc = rng.integers(-9, 8, (8, 8))
    sc[np.arange(8), np.arange(8)] = rng.integers(3, 9, 8)
    sc[0, 0], sc[1, 2], sc[3, 3] = top, -128, top
    mat = nwhip.SubMatrix(list(range(1, 9)), sc)
    assert (sc + 2 > 127).any() == (top == 127)
    pairs = [planted(rng, 300, 130, 8, 100, 100, 10, [("d", 3)], 0.1), planted(rng, 257, 65, 8, 190, 60, 2),
             (_rand(rng, 5, 8), _rand(rng, 63, 8)), (np.full(40, 1, np.int8), np.full(70, 1, np.int8)),
             (_rand(rng, 513, 8), _rand(rng, 64, 8))]
    hits, _, _, want = align_and_check(pairs, mat, -1, -11, ends)
    assert want[3][0] >= 40 * top - 41


# ------------------------------------------------------------------ chunks
def test_chunks_fit_the_budget():
    rng = np.random.default_rng(1009)
    mat = matrix(20)
    pairs = [planted(rng, int(rng.integers(280, 321)), int(rng.integers(150, 200)), 20, 40, 120, 20, [("d", 6)])
             for _ in range(40)]
    h0, ops0, st0 = nwhip.align_batch_semi(pairs, mat, -1, -11, 15)
    assert st0.chunks == 1
    check_alignments(pairs[:6], mat, -1, -11, 15, h0[:6], ops0[:6])
    # 14 pairs' worth of direction bytes for 40 pairs: three chunks at the least, whatever else is held
    mem = 14 * nwhip.batch_affine_dir_bytes(300, 190)
    h, ops, st = nwhip.align_batch_semi(pairs, mat, -1, -11, 15, mem_bytes=mem)
    assert st.chunks >= 3 and st.peak_bytes <= mem and st.dir_bytes == st0.dir_bytes
    assert st.dir_bytes == sum(nwhip.batch_affine_dir_bytes(a.size, b.size) for a, b in pairs)
    np.testing.assert_array_equal(h, h0)
    for x, y in zip(ops, ops0):
        np.testing.assert_array_equal(x, y)
    # below one pair's direction bytes: NW_ERR_OOM
    with pytest.raises(nwhip.NwError) as e:
        nwhip.align_batch_semi(pairs, mat, -1, -11, 15, mem_bytes=nwhip.batch_affine_dir_bytes(300, 190) - 1)
    assert e.value.status == nwhip.NW_ERR_OOM


# ------------------------------------------------------------------ device API
@pytest.mark.parametrize("ends", [3, 15, 0])
def test_context_score_batch_semi_on_a_stream(ends):
    import torch
    alpha, ge, go = 20, -1, -11
    mat = nwhip.SubMatrix(grid_matrix(alpha).letters, grid_matrix(alpha).scores, other=1)
    pairs = list(score_pairs(alpha))
    want = np.array([want_hit(a, b, mat, ge, go, ends) for a, b in pairs], np.int32)
    s1, off1, s2, off2 = nwhip.batch_csr(pairs)
    ctx = nwhip.Context(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = [torch.from_numpy(x).cuda() for x in (s1, off1, s2, off2)]
        got = ctx.score_batch_semi(d[0], d[1], d[2], d[3], 130, mat, ge, go, ends, stream=stream)
        # a second launch on the same context and stream: its workspace is reused
        got2 = ctx.score_batch_semi(d[0], d[1], d[2], d[3], 200, mat, ge, go, ends, stream=stream, waves=2)
        # max_n2 below a pair's rows: that pair is refused, the others computed
        low = ctx.score_batch_semi(d[0], d[1], d[2], d[3], 65, mat, ge, go, ends, stream=stream)
    stream.synchronize()
    assert ctx.status(stream) == nwhip.NW_OK
    for g in (got, got2):
        g = g.cpu().numpy()
        assert g.shape == (len(pairs), 8) and g.dtype == np.int32
        np.testing.assert_array_equal(g[:, :3], want)  # (the empty-side pairs too: by the kernel)
        assert (g[:, 3:5] == -1).all() and (g[:, 5:] == 0).all()
    low = low.cpu().numpy()
    n2 = np.diff(off2)
    assert (n2 > 65).sum() >= 8
    np.testing.assert_array_equal(low[n2 <= 65, :3], want[n2 <= 65])
    assert (low[n2 > 65, 0] == I32_MIN).all() and (low[n2 > 65, 1:5] == -1).all() and (low[:, 5:] == 0).all()
    ctx.close()


def test_empty_sides_by_the_kernel():
    """The async form answers pairs with an empty side on the device: all 16 `ends`."""
    import torch
    mat = nwhip.SubMatrix(matrix(4).letters, matrix(4).scores, other=1)
    rng = np.random.default_rng(1010)
    e = np.zeros(0, np.int8)
    pairs = [(e, _rand(rng, 7, 4)), (_rand(rng, 6, 4), e), (e, e), (_rand(rng, 5, 4), _rand(rng, 3, 4))]
    s1, off1, s2, off2 = nwhip.batch_csr(pairs)
    ctx = nwhip.Context(0)
    d = [torch.from_numpy(x).cuda() for x in (s1, off1, s2, off2)]
    for ends in range(16):
        want = np.array([want_hit(a, b, mat, -2, -3, ends) for a, b in pairs], np.int32)
        got = ctx.score_batch_semi(d[0], d[1], d[2], d[3], 7, mat, -2, -3, ends)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy()[:, :3], want, err_msg=f"ends {ends}")
    ctx.close()


# ------------------------------------------------------------------ CLI
MATRIX_TEXT = """# transitions cost less than transversions; N is the wildcard
   A  C  G  T  *
A  5 -4 -1 -4 -2
C -4  5 -4 -1 -2
G -1 -4  5 -4 -2
T -4 -1 -4  5 -2
* -2 -2 -2 -2 -2
"""
LINE = re.compile(r"Score: (-?\d+)(?: begin \((-?\d+), (-?\d+)\))? end \((-?\d+), (-?\d+)\)$")


@pytest.mark.parametrize("with_matrix", [False, True])
@pytest.mark.parametrize("score_only", [False, True])
def test_cli_batch_ends(tmp_path, with_matrix, score_only):
    rng = np.random.default_rng(1011)
    letters = np.frombuffer(b"ACGTacgtN", np.int8)
    pairs = []
    for k, (n1, n2) in enumerate([(300, 40), (90, 30), (257, 65)]):
        a = letters[rng.integers(0, 9, n1)].copy()
        b = a[25:25 + n2].copy()
        b[7] = ord("N")
        (tmp_path / f"a{k}.bdna").write_bytes(a.tobytes())
        (tmp_path / f"b{k}.bdna").write_bytes(b.tobytes())
        pairs.append((a, b))
    lst = tmp_path / "pairs.txt"
    lst.write_text("".join(f"a{k}.bdna b{k}.bdna\n" for k in range(3)))
    (tmp_path / "m.txt").write_text(MATRIX_TEXT)
    args = ["--batch", str(lst), "--ends", "3", "--scheme", "2,-3,-1", "--gap-open", "-5"]
    if with_matrix:
        args += ["--matrix", str(tmp_path / "m.txt")]
        mat = nwhip.SubMatrix.from_text(MATRIX_TEXT)
    else:
        mat = nwhip.SubMatrix.uniform("ACGT", 2, -3, other="N")
    if score_only:
        args.append("--score-only")
    exe = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    int(lines[0])  # the wall time, ms
    hits, ops, _ = nwhip.align_batch_semi(pairs, mat, -1, -5, 3)
    check_alignments(pairs, mat, -1, -5, 3, hits, ops)
    assert (hits["begin_j"] >= 20).all() and (hits["begin_i"] == 0).all()
    at = 1
    for (a, b), h, o in zip(pairs, hits, ops):
        m = LINE.match(lines[at])
        assert m, lines[at]
        assert int(m[1]) == h["score"] and (int(m[4]), int(m[5])) == (h["end_i"], h["end_j"])
        at += 1
        if score_only:
            assert m[2] is None
            continue
        assert (int(m[2]), int(m[3])) == (h["begin_i"], h["begin_j"])
        row1, row2 = nwhip.ops_expand(a, b, o, begin=(int(h["begin_i"]), int(h["begin_j"])))
        text = [bytes(np.where(r_ == 0, ord("-"), r_).astype(np.uint8)).decode() for r_ in (row1, row2)]
        assert lines[at:at + 2] == ["A: " + text[0], "B: " + text[1]]  # the aligned part alone
        assert len(text[0]) == o.size < a.size
        at += 2
    assert lines[at:] == [""]
