"""GPU: batched local alignment -- Smith-Waterman with affine gaps and a substitution
matrix (nw_score_batch_local, nw_align_batch_local, nw_score_batch_local_async;
csrc/nw_batch_local.hip).

Checker: the plain Python recurrence, best cell and walk of tests/nw_local.py (anchored
to the oracle's Smith-Waterman by tests/test_batch_local_host.py); with gap_open = 0 and a
match / mismatch matrix also nw_sw_align itself.  All comparisons are of integers and
bytes, exact.  The shapes are tests/test_batch.py's -- one lane, a lane boundary, a strip
seam (255 / 256 / 257 columns, three strips at 513), a row-block boundary (63 / 64 / 65
rows, three blocks at 130), empty sides -- plus what only a local alignment can get wrong:
the first row-major maximum among equal ones in one strip, in two strips and in two rows,
a best cell on the last column of a strip, on column n1 and on row n2, columns past n1
that would outscore every real cell, paths that stop on row 0 / column 0, and a best
cell left over from the pair a worker ran before.  Sizes stay within 520 x 200 but for
one ops case of 1500 x 1100 and the run of 300 ups, which needs 360 rows (60 columns).
"""
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import nw_local as nl
import nwhip
from conftest import ROOT
from test_batch import SCORE_N1, SCORE_N2, _rand

pytestmark = pytest.mark.gpu

I32_MIN = np.iinfo(np.int32).min
COST = [(-1, -11), (-3, 0), (-2, -3), (-2, -11)]  # (ge, go)


@functools.lru_cache(maxsize=None)
def matrix(alpha):
    """Seeded and asymmetric over the bytes 1..alpha: 4..11 on the diagonal, -8..-1 off
    it, so that the expected score of two random letters is negative."""
    rng = np.random.default_rng(700 + alpha)
    sc = rng.integers(-8, 0, (alpha, alpha))
    sc[np.arange(alpha), np.arange(alpha)] = rng.integers(4, 12, alpha)
    assert (sc != sc.T).any() and sc.mean() < -1
    return nwhip.SubMatrix(list(range(1, alpha + 1)), sc)


def mutate(rng, seg, alpha, runs=(), subs=0.05):
    """A copy of seg with substitutions and, spread evenly, the indel runs: ('d', L) drops
    L letters of seg (L lefts in the path), ('i', L) inserts L random letters (L ups)."""
    seg = seg.copy()
    hit = rng.random(seg.size) < subs
    seg[hit] = _rand(rng, int(hit.sum()), alpha)
    cuts = np.linspace(0, seg.size, len(runs) + 2).astype(int)[1:-1]
    out, at = [], 0
    for cut, (kind, length) in zip(cuts, runs):
        out.append(seg[at:cut])
        at = cut
        if kind == "d":
            at = min(seg.size, cut + length)
        else:
            out.append(_rand(rng, length, alpha))
    out.append(seg[at:])
    return np.concatenate(out)


def planted(rng, n1, n2, alpha, at1, seg, at2, runs=(), subs=0.05):
    """Random s1 of n1 and s2 of n2 letters; a mutated copy of s1[at1 : at1 + seg] stands in
    s2 from at2 on (cut where s2 ends)."""
    a, b = _rand(rng, n1, alpha), _rand(rng, n2, alpha)
    m = mutate(rng, a[at1:at1 + seg], alpha, runs, subs)[:max(n2 - at2, 0)]
    b[at2:at2 + m.size] = m
    return a, b


@functools.lru_cache(maxsize=None)
def score_pairs(alpha):
    """The cross product of the sizes plus the empty sides, shuffled; where both sides
    have 60 letters, a mutated segment of s1 is planted in s2."""
    rng = np.random.default_rng(800 + alpha)
    pairs = []
    for n1, n2 in itertools.product(SCORE_N1, SCORE_N2):
        if n1 >= 60 and n2 >= 60:
            seg = int(rng.integers(30, min(n1, n2) - 10))
            at1, at2 = int(rng.integers(0, n1 - seg + 1)), int(rng.integers(0, n2 - seg + 1))
            pairs.append(planted(rng, n1, n2, alpha, at1, seg, at2, [("d", 2), ("i", 3)], 0.2))
        else:
            pairs.append((_rand(rng, n1, alpha), _rand(rng, n2, alpha)))
    pairs += [(_rand(rng, 0, alpha), _rand(rng, 7, alpha)), (_rand(rng, 7, alpha), _rand(rng, 0, alpha)),
              (_rand(rng, 0, alpha), _rand(rng, 0, alpha))]
    return tuple(pairs[i] for i in rng.permutation(len(pairs)))


def want_hit(a, b, sc, index, ge, go):
    return nl.best(nl.fill(a, b, sc, index, ge, go)[0])


@functools.lru_cache(maxsize=None)
def score_want(alpha, ge, go, transposed=False):
    m = matrix(alpha)
    sc = m.scores.T if transposed else m.scores
    return np.array([want_hit(a, b, sc, m.index, ge, go) for a, b in score_pairs(alpha)], np.int32)


def hit_rows(hits):
    return np.stack([hits["score"], hits["end_i"], hits["end_j"]], axis=1)


def check_alignments(pairs, mat, ge, go, hits, ops):
    """Hits, begin cells and ops against the checker; returns the checker's (begin, end,
    ops) per pair."""
    out = []
    for (a, b), h, o in zip(pairs, hits, ops):
        tables = nl.fill(a, b, mat.scores, mat.index, ge, go)
        sc, ei, ej = nl.best(tables[0])
        want, begin = nl.walk(a, b, mat.scores, mat.index, ge, go, tables)
        what = f"{a.size} x {b.size} ge {ge} go {go}"
        assert (h["score"], h["end_i"], h["end_j"]) == (sc, ei, ej), what
        assert (h["begin_i"], h["begin_j"]) == begin, what
        assert (h["reserved"] == 0).all()
        np.testing.assert_array_equal(o, want, err_msg=what)
        assert o.size <= a.size + b.size
        assert nwhip.ops_score_matrix(a, b, o, mat, ge, go, begin=begin) == sc
        assert nl.path_score(a, b, o, begin, mat.scores, mat.index, ge, go) == (sc, (ei, ej))
        out.append((begin, (ei, ej), want))
    return out


# ------------------------------------------------------------------ scores and end cells
@pytest.mark.parametrize("ge,go", COST)
@pytest.mark.parametrize("alpha", [4, 20, 32])
def test_hits_at_the_pairs_own_index(alpha, ge, go):
    pairs, mat = score_pairs(alpha), matrix(alpha)
    want = score_want(alpha, ge, go)
    # the asymmetry matters on this batch: a transposed lookup cannot pass
    assert (score_want(alpha, ge, go, True) != want).any()
    assert (want[:, 0] > 40).sum() >= 12 and (want[:, 0] == 0).sum() >= 3
    got, st = nwhip.score_batch_local(pairs, mat, ge, go, return_stats=True)
    np.testing.assert_array_equal(hit_rows(got), want)
    assert (got["begin_i"] == -1).all() and (got["begin_j"] == -1).all() and (got["reserved"] == 0).all()
    assert st.pairs == len(pairs) and st.cells == sum(a.size * b.size for a, b in pairs)
    assert st.chunks == 1 and 1 <= st.waves <= len(pairs) - 3 and st.fill_ms > 0
    # waves = 3: every worker sweeps a dozen pairs one after the other, so a best cell
    # that is not reset per pair fails here
    got, st = nwhip.score_batch_local(pairs, mat, ge, go, waves=3, return_stats=True)
    np.testing.assert_array_equal(hit_rows(got), want)
    assert st.waves == 3


# ------------------------------------------------------------------ ops
@functools.lru_cache(maxsize=None)
def ops_pairs():
    """Over 20 letters.  Three pairs whose path has more than 300 ops, crosses the 256-
    column seam and a 64-row block boundary (150 columns of s1 dropped in runs of up to
    20), the 1500 x 1100 pair, and small shapes with and without a planted segment."""
    rng = np.random.default_rng(900)
    d = [("d", 20), ("d", 17), ("i", 4), ("d", 20), ("d", 19), ("d", 1), ("d", 20), ("d", 18), ("i", 9), ("d", 20),
         ("d", 15)]
    pairs = [planted(rng, 520, 200, 20, 90, 330, 12, d), planted(rng, 500, 190, 20, 130, 330, 3, d),
             planted(rng, 470, 200, 20, 70, 330, 15, d),
             planted(rng, 1500, 1100, 20, 300, 800, 150, [("d", 12), ("i", 20), ("d", 3), ("i", 7), ("d", 20), ("i", 1)])]
    for n1, n2 in [(1, 1), (4, 64), (5, 65), (256, 64), (257, 65), (513, 130), (255, 63), (300, 129)]:
        if n1 >= 200:
            pairs.append(planted(rng, n1, n2, 20, n1 - 150, 50, 5, [("i", 2), ("d", 5)]))
        else:
            pairs.append((_rand(rng, n1, 20), _rand(rng, n2, 20)))
    return tuple(pairs)


@pytest.mark.parametrize("ge,go", [(-1, -11), (-2, -3)])
def test_ops_are_the_walks_from_the_best_cell(ge, go):
    pairs, mat = ops_pairs(), matrix(20)
    hits, ops, st = nwhip.align_batch_local(pairs, mat, ge, go)
    want = check_alignments(pairs, mat, ge, go, hits, ops)
    # locality is exercised -- judged on the checker's results alone
    inner = sum(begin != (0, 0) and end != (b.size, a.size) for (a, b), (begin, end, _) in zip(pairs, want))
    assert 2 * inner >= len(pairs)
    long_ones = sum(o.size >= 300 and begin[1] < 256 < end[1] and begin[0] // 64 != end[0] // 64
                    for begin, end, o in want)
    assert long_ones >= 3
    assert any((o == 1).any() and (o == 2).any() for _, _, o in want)
    assert st.chunks == 1
    assert st.dir_bytes == sum(nwhip.batch_affine_dir_bytes(a.size, b.size) for a, b in pairs)
    assert st.peak_bytes > st.dir_bytes and st.walk_ms > 0
    # the score entry finds the same hits
    np.testing.assert_array_equal(hit_rows(nwhip.score_batch_local(pairs, mat, ge, go)), hit_rows(hits))


# ------------------------------------------------------------------ ties and the place of the best cell
UNI = (5, -4)  # match, mismatch of the hand-made cases


def _bg(n1, n2):
    """s1 all letter 1, s2 all letter 2: nothing matches."""
    return np.full(n1, 1, np.int8), np.full(n2, 2, np.int8)


def _put(seq, at, seg):
    seq[at:at + seg.size] = seg


@functools.lru_cache(maxsize=None)
def placed_pairs():
    """(pairs, the end cells the checker must find, in order).  Segments over the letters
    3 and 4 in backgrounds that match nothing."""
    rng = np.random.default_rng(901)
    P = rng.integers(3, 5, 12).astype(np.int8)
    Q = P[::-1].copy()
    Q[0] = 7 - P[0]  # (not P)
    pairs, ends = [], []

    def add(n1, n2, cols, rows, end):
        a, b = _bg(n1, n2)
        for at, seg in cols:
            _put(a, at, seg)
        for at, seg in rows:
            _put(b, at, seg)
        pairs.append((a, b))
        ends.append(end)

    # two identical segments at different rows and columns: four equal maxima, the first
    # in row-major order is reported
    add(400, 150, [(30, P), (300, P)], [(20, P), (90, P)], (32, 42))
    # equal maxima in strip 0 and strip 1 on one row: strip 0's
    add(500, 100, [(100, P), (400, P)], [(70, P)], (82, 112))
    # the later strip has the smaller row: the later strip's
    add(500, 150, [(100, P), (400, Q)], [(10, Q), (100, P)], (22, 412))
    # the best cell on the last column of a strip
    add(300, 80, [(244, P)], [(30, P)], (42, 256))
    # on column n1 with n1 % 4 != 0 (columns past n1 hold cells, and must not win)
    for n1 in (13, 258, 263):
        add(n1, 90, [(n1 - 12, P)], [(40, P)], (52, n1))
    # on row n2 with n2 % 64 = 63, 0, 1
    for n2 in (63, 64, 65, 127, 128, 129):
        add(70, n2, [(20, P)], [(n2 - 12, P)], (n2, 32))
    # the path begins on column 0 / on row 0: the walk stops on the boundary
    add(70, 90, [(0, P)], [(40, P)], (52, 12))
    add(70, 90, [(30, P)], [(0, P)], (12, 42))
    # columns past n1 would outscore every real cell: all of s1 one letter and s2 the same
    # letter throughout (the pair after it in the batch too, so the row buffer goes on)
    for _ in range(2):
        pairs.append((np.full(5, 1, np.int8), np.full(100, 1, np.int8)))
        ends.append((5, 5))
    pairs.append((np.full(258, 3, np.int8), np.full(70, 3, np.int8)))
    ends.append((70, 70))
    return tuple(pairs), tuple(ends)


@pytest.mark.parametrize("waves", [0, 1])
def test_ties_and_best_cell_placement(waves):
    pairs, ends = placed_pairs()
    mat = nwhip.SubMatrix.uniform([1, 2, 3, 4], *UNI)
    ge, go = -1, -11
    for (a, b), end in zip(pairs[:3], ends[:3]):  # the ties are ties
        H = nl.fill(a, b, mat.scores, mat.index, ge, go)[0]
        top = [tuple(c) for c in np.argwhere(H == H.max())]
        assert len(top) >= 2 and top[0] == end and H.max() == 60
        if end == (22, 412):
            assert top == [(22, 412), (112, 112)]
        if end == (82, 112):
            assert top == [(82, 112), (82, 412)]
    hits, ops, _ = nwhip.align_batch_local(pairs, mat, ge, go, waves=waves)
    want = check_alignments(pairs, mat, ge, go, hits, ops)
    assert tuple(end for _, end, _ in want) == ends
    assert want[-4][0] == (0, 30) and want[-5][0] == (40, 0)  # begin cells on the boundary
    np.testing.assert_array_equal(hit_rows(nwhip.score_batch_local(pairs, mat, ge, go, waves=waves)), hit_rows(hits))


def test_gap_runs_inside_a_local_path():
    """300 lefts over the strip seam and 300 ups over the row blocks, under go = -11: with
    100 per match the two halves are worth the gap between them."""
    mat = nwhip.SubMatrix.uniform([1, 2, 3, 4], 100, -100)
    rng = np.random.default_rng(902)
    P, Q = rng.integers(3, 5, 10).astype(np.int8), rng.integers(3, 5, 10).astype(np.int8)
    a, b = _bg(400, 60)
    _put(a, 50, P)
    _put(a, 360, Q)
    _put(b, 20, np.concatenate([P, Q]))
    c, d = _bg(60, 360)
    _put(c, 20, np.concatenate([P, Q]))
    _put(d, 15, P)
    _put(d, 325, Q)
    pairs = [(a, b), (c, d)]
    hits, ops, _ = nwhip.align_batch_local(pairs, mat, -1, -11)
    want = check_alignments(pairs, mat, -1, -11, hits, ops)
    assert hits["score"].tolist() == [2000 - 311, 2000 - 311]
    assert want[0][0] == (20, 50) and want[0][1] == (40, 370) and (ops[0] == 2).sum() == 300
    assert want[1][0] == (15, 20) and want[1][1] == (335, 40) and (ops[1] == 1).sum() == 300
    np.testing.assert_array_equal(ops[0], [0] * 10 + [2] * 300 + [0] * 10)
    np.testing.assert_array_equal(ops[1], [0] * 10 + [1] * 300 + [0] * 10)


# ------------------------------------------------------------------ independent code
@pytest.mark.parametrize("scheme", [(1, -1, -1), (2, -1, -2)])
def test_linear_uniform_is_nw_sw_align(scheme):
    """gap_open = 0 and a match / mismatch matrix: hit, begin cell and ops of nw_sw_align."""
    rng = np.random.default_rng(903)
    pairs = [planted(rng, 300, 150, 4, 100, 120, 10, [("d", 3), ("i", 2)], 0.1),
             planted(rng, 513, 130, 4, 200, 100, 20, [("i", 5)], 0.1), planted(rng, 257, 65, 4, 190, 60, 2),
             (_rand(rng, 64, 4), _rand(rng, 200, 4)), (_rand(rng, 5, 4), _rand(rng, 63, 4)),
             planted(rng, 400, 200, 4, 0, 150, 50, [("d", 10)], 0.15)]
    mat = nwhip.SubMatrix.uniform([1, 2, 3, 4], scheme[0], scheme[1])
    hits, ops, _ = nwhip.align_batch_local(pairs, mat, scheme[2], 0)
    for (a, b), h, o in zip(pairs, hits, ops):
        al, want = nwhip.sw_align(a, b, scheme)
        assert (h["score"], h["end_i"], h["end_j"]) == (al.score, al.end_i, al.end_j)
        assert (h["begin_i"], h["begin_j"]) == (al.begin_i, al.begin_j)
        np.testing.assert_array_equal(o, want)


# ------------------------------------------------------------------ one worker, pair after pair
def test_short_pair_after_a_long_one_on_the_same_worker():
    """One worker: 513 x 130 with a hit of some hundreds (three strips: profile, scratch and
    best cell all used), then 5 x 130, 257 x 1 and a pair that aligns nothing."""
    rng = np.random.default_rng(904)
    mat = matrix(20)
    pairs = [(_rand(rng, 257, 20), _rand(rng, 1, 20)), planted(rng, 513, 130, 20, 300, 110, 10, [("d", 4)]),
             (_rand(rng, 5, 20), _rand(rng, 130, 20)), (np.full(40, 1, np.int8), np.full(40, 2, np.int8))]
    assert mat.scores[0, 1] < 0
    hits, ops, st = nwhip.align_batch_local(pairs, mat, -1, -11, waves=1)
    assert st.waves == 1
    want = check_alignments(pairs, mat, -1, -11, hits, ops)
    assert hits["score"][1] > 300 and tuple(hits[3])[:5] == (0, 0, 0, 0, 0) and ops[3].size == 0
    assert want[1][1][1] > 256
    got = nwhip.score_batch_local(pairs, mat, -1, -11, waves=1)
    np.testing.assert_array_equal(hit_rows(got), hit_rows(hits))


# ------------------------------------------------------------------ chunks
def test_chunks_fit_the_budget():
    rng = np.random.default_rng(905)
    mat = matrix(20)
    pairs = [planted(rng, int(rng.integers(280, 321)), int(rng.integers(150, 200)), 20, 40, 120, 20, [("d", 6)])
             for _ in range(40)]
    h0, ops0, st0 = nwhip.align_batch_local(pairs, mat, -1, -11)
    assert st0.chunks == 1
    check_alignments(pairs[:6], mat, -1, -11, h0[:6], ops0[:6])
    # 14 pairs' worth of direction bytes for 40 pairs: three chunks at the least, whatever else is held
    mem = 14 * nwhip.batch_affine_dir_bytes(300, 190)
    h, ops, st = nwhip.align_batch_local(pairs, mat, -1, -11, mem_bytes=mem)
    assert st.chunks >= 3 and st.peak_bytes <= mem and st.dir_bytes == st0.dir_bytes
    np.testing.assert_array_equal(h, h0)
    for x, y in zip(ops, ops0):
        np.testing.assert_array_equal(x, y)
    # below one pair's direction bytes: NW_ERR_OOM
    with pytest.raises(nwhip.NwError) as e:
        nwhip.align_batch_local(pairs, mat, -1, -11, mem_bytes=nwhip.batch_affine_dir_bytes(300, 190) - 1)
    assert e.value.status == nwhip.NW_ERR_OOM


# ------------------------------------------------------------------ device API
def test_context_score_batch_local_on_a_stream():
    import torch
    alpha, ge, go = 20, -1, -11
    rng = np.random.default_rng(906)
    mat = nwhip.SubMatrix(matrix(alpha).letters, matrix(alpha).scores, other=1)
    pairs = list(score_pairs(alpha)) + [(np.full(40, 1, np.int8), np.full(40, 2, np.int8)),
                                        planted(rng, 300, 150, alpha, 100, 100, 20)]
    want = np.array([want_hit(a, b, mat.scores, mat.index, ge, go) for a, b in pairs], np.int32)
    assert want[-2].tolist() == [0, 0, 0]
    s1, off1, s2, off2 = nwhip.batch_csr(pairs)
    ctx = nwhip.Context(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = [torch.from_numpy(x).cuda() for x in (s1, off1, s2, off2)]
        got = ctx.score_batch_local(d[0], d[1], d[2], d[3], 150, mat, ge, go, stream=stream)
        # a second launch on the same context and stream: its workspace is reused
        got2 = ctx.score_batch_local(d[0], d[1], d[2], d[3], 200, mat, ge, go, stream=stream, waves=2)
        # max_n2 below a pair's rows: that pair is refused, the others computed
        low = ctx.score_batch_local(d[0], d[1], d[2], d[3], 65, mat, ge, go, stream=stream)
    stream.synchronize()
    assert ctx.status(stream) == nwhip.NW_OK
    for g in (got, got2):
        g = g.cpu().numpy()
        assert g.shape == (len(pairs), 8) and g.dtype == np.int32
        np.testing.assert_array_equal(g[:, :3], want)  # (empty and all-negative pairs: zeros, by the kernel)
        assert (g[:, 3:5] == -1).all() and (g[:, 5:] == 0).all()
    low = low.cpu().numpy()
    n2 = np.diff(off2)
    assert (n2 > 65).sum() >= 9
    np.testing.assert_array_equal(low[n2 <= 65, :3], want[n2 <= 65])
    assert (low[n2 > 65, 0] == I32_MIN).all() and (low[n2 > 65, 1:5] == -1).all() and (low[:, 5:] == 0).all()
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
def test_cli_batch_local(tmp_path, with_matrix, score_only):
    rng = np.random.default_rng(907)
    letters = np.frombuffer(b"ACGTacgtN", np.int8)
    pairs = []
    for k, (n1, n2) in enumerate([(300, 120), (40, 70), (257, 65)]):
        a, b = letters[rng.integers(0, 9, n1)].copy(), letters[rng.integers(0, 9, n2)].copy()
        b[10:40] = a[5:35]
        b[20] = ord("N")
        (tmp_path / f"a{k}.bdna").write_bytes(a.tobytes())
        (tmp_path / f"b{k}.bdna").write_bytes(b.tobytes())
        pairs.append((a, b))
    lst = tmp_path / "pairs.txt"
    lst.write_text("".join(f"a{k}.bdna b{k}.bdna\n" for k in range(3)))
    (tmp_path / "m.txt").write_text(MATRIX_TEXT)
    args = ["--batch", str(lst), "--local", "--scheme", "2,-3,-1", "--gap-open", "-5"]
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
    hits, ops, _ = nwhip.align_batch_local(pairs, mat, -1, -5)
    check_alignments(pairs, mat, -1, -5, hits, ops)
    assert (hits["score"] >= 25).all()
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
        assert lines[at:at + 2] == ["A: " + text[0], "B: " + text[1]]  # the aligned segment alone
        assert len(text[0]) == o.size < a.size
        at += 2
    assert lines[at:] == [""]
