"""GPU: batched global alignment under the two-piece gap cost inside a band (nw_score_batch_dual_
banded, nw_align_batch_dual_banded, nw_score_batch_dual_banded_async; csrc/nw_batch_dual_banded.hip).

Checker: the plain Python recurrence of tests/nw_banded2.py (held to the definition by brute
force, to its own cell fill, to tests/nw_gotoh2.py under a covering band and to tests/nw_banded.py
under equal pieces by tests/test_batch_dual_banded_host.py); for the reductions the parent
entries themselves.  Everything is exact.  The shapes are tests/test_batch.py's grid under bands
from 0 to covering and cost sets with dge = ge2 - ge1 of each sign (the mask must hold piece 2's
drift either way), square pairs of 520 and 700 columns whose later strips enter below iteration
0, the directed pairs of the host file (the 850 x 553 pair at the band that recovers it, runs at
the crossover length, paths the band shuts out) and its coverage list.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import nw_banded2 as b2
import nw_gotoh
import nwhip
from conftest import ROOT
from test_batch import SCORE_N2, _rand, ops_pairs, score_pairs
from test_batch_dual_banded_host import (COSTS, COVERING, DOWN, EQUAL, FLAT, TWO_RUNS_W, UP, cases, directed, grid_pairs,
                                         results)
from test_batch_dual_host import COVER, MM, matrix, planted, two_runs_pair, uniform
from test_batch_paths_host import LETTERS

pytestmark = pytest.mark.gpu

I32_MIN = np.iinfo(np.int32).min
BANDS = [0, 1, 31, 64, 200, COVERING]


def kw(pc, w):
    """The Python entries' keywords of (go1, ge1, go2, ge2) and the band."""
    return dict(gap_open=pc[0], gap=pc[1], gap_open2=pc[2], gap2=pc[3], band=w)


def want_of(pairs, mat, pc, w):
    """[(score, ops)] of the checker; every walk stays in the band (it asserts so)."""
    out = []
    for a, b in pairs:
        tabs = b2.fill(a, b, mat.scores, mat.index, pc, w)
        out.append((int(tabs[0][-1, -1]), b2.walk(a, b, mat.scores, mat.index, pc, w, tables=tabs)))
    return out


def check_alignments(pairs, mat, pc, w, scores, ops, want=None):
    want = want if want is not None else want_of(pairs, mat, pc, w)
    assert scores.tolist() == [s for s, _ in want]
    for (a, b), o, (s, wo) in zip(pairs, ops, want):
        np.testing.assert_array_equal(o, wo, err_msg=f"{a.size} x {b.size} w {w} pieces {pc}")   # (n_ops: the length)
        assert max(a.size, b.size) <= o.size <= a.size + b.size
        k = dict(kw(pc, w))
        k.pop("band")
        assert nwhip.ops_score_dual(a, b, o, mat, **k) == s


# ------------------------------------------------------------------ the grid
@functools.lru_cache(maxsize=None)
def grid_want(alpha, pc, w):
    return want_of(grid_pairs(alpha), matrix(alpha), pc, w)


@pytest.mark.parametrize("w", BANDS)
@pytest.mark.parametrize("pc", COSTS, ids=str)
@pytest.mark.parametrize("alpha", [4, 20, 32])
def test_grid_scores_ops_and_n_ops(alpha, pc, w):
    pairs, mat = grid_pairs(alpha), matrix(alpha)
    want = grid_want(alpha, pc, w)
    scores = np.array([s for s, _ in want], np.int32)
    got, st = nwhip.score_batch_dual_banded(pairs, mat, return_stats=True, **kw(pc, w))
    np.testing.assert_array_equal(got, scores)
    assert st.pairs == len(pairs) and st.cells == sum(a.size * b.size for a, b in pairs)
    assert st.chunks == 1 and 1 <= st.waves <= len(pairs) - 3 and st.fill_ms > 0
    # waves = 3: every worker sweeps a dozen pairs one after the other
    got, st = nwhip.score_batch_dual_banded(pairs, mat, waves=3, return_stats=True, **kw(pc, w))
    np.testing.assert_array_equal(got, scores)
    assert st.waves == 3
    for waves in (0, 3):
        sc, ops, st = nwhip.align_batch_dual_banded(pairs, mat, waves=waves, **kw(pc, w))
        check_alignments(pairs, mat, pc, w, sc, ops, want)
        assert st.dir_bytes == sum(nwhip.batch_dual_banded_dir_bytes(a.size, b.size, w) for a, b in pairs)


# ------------------------------------------------------------------ strips that enter below iteration 0
@pytest.mark.parametrize("pc", COSTS, ids=str)
@pytest.mark.parametrize("w", [0, 64, 192])
def test_square_pairs_whose_strips_start_late(w, pc):
    """520 and 700 columns: strips 1 and 2 have 256p + dlo >= 64 and enter with every value forced;
    677 x 700 and 700 x 650 move the band off the main diagonal."""
    rng = np.random.default_rng(51)
    mat = matrix(20)
    pairs = [(_rand(rng, n1, 20), _rand(rng, n2, 20)) for n1, n2 in [(520, 520), (700, 700), (677, 700), (700, 650)]]
    x = pairs[1][0].copy()   # a near-copy: the path hugs the diagonal, with gaps
    y = np.concatenate([x[:200], x[230:500], _rand(rng, 25, 20), x[500:]])
    pairs.append((x, y))
    # the square pairs' strips 1 and 2 start after iteration 0 at every one of these bands
    assert all(256 * p - w >= 64 for a, _ in pairs[:2] for p in range(1, (a.size + 255) // 256))
    want = want_of(pairs, mat, pc, w)
    for waves in (0, 1):
        sc, ops, st = nwhip.align_batch_dual_banded(pairs, mat, waves=waves, **kw(pc, w))
        check_alignments(pairs, mat, pc, w, sc, ops, want)
        full = sum(nwhip.batch_dual_dir_bytes(a.size, b.size) for a, b in pairs)
        assert st.dir_bytes == sum(nwhip.batch_dual_banded_dir_bytes(a.size, b.size, w) for a, b in pairs) <= full
        assert w > 0 or st.dir_bytes < full   # (w = 0: 8 or 9 slots a strip where the unbanded sweep has 10 to 12)
        np.testing.assert_array_equal(nwhip.score_batch_dual_banded(pairs, mat, waves=waves, **kw(pc, w)), sc)


def test_nothing_leaks_from_the_pair_before():
    """One worker, in this order: 513 x 500 over letters 0..15 (three strips, the later ones
    entering late, all three scratch columns written in band only), 5 x 500 over letters 16..31
    (a stale profile row, or stale scratch read through an unmasked feed, shows here), 257 x 1."""
    rng = np.random.default_rng(43)
    mat = matrix(32)
    lo, hi = (lambda n: _rand(rng, n, 16)), (lambda n: (_rand(rng, n, 16) + 16).astype(np.int8))
    pairs = [(lo(513), lo(500)), (hi(5), hi(500)), (_rand(rng, 257, 32), _rand(rng, 1, 32))]
    for pc in (UP, DOWN):
        for w in (0, 64):
            want = want_of(pairs, mat, pc, w)
            got, st = nwhip.score_batch_dual_banded(pairs, mat, waves=1, return_stats=True, **kw(pc, w))
            assert st.waves == 1 and got.tolist() == [s for s, _ in want]
            sc, ops, st = nwhip.align_batch_dual_banded(pairs, mat, waves=1, **kw(pc, w))
            assert st.waves == 1
            check_alignments(pairs, mat, pc, w, sc, ops, want)


# ------------------------------------------------------------------ reductions on the device
@functools.lru_cache(maxsize=None)
def ops_pairs20():
    rng = np.random.default_rng(78)
    return tuple((_rand(rng, a.size, 20), _rand(rng, b.size, 20)) for a, b in ops_pairs())


@pytest.mark.parametrize("pc", COSTS, ids=str)
def test_a_covering_band_is_align_batch_dual_byte_for_byte(pc):
    pairs, mat = ops_pairs20() + score_pairs(20), matrix(20)
    k = dict(kw(pc, 0))
    k.pop("band")
    sc0, ops0, st0 = nwhip.align_batch_dual(pairs, mat, **k)
    for w in (600, COVERING, 2 ** 40):
        sc, ops, st = nwhip.align_batch_dual_banded(pairs, mat, band=w, **k)
        np.testing.assert_array_equal(sc, sc0)
        for (a, b), x, y in zip(pairs, ops, ops0):
            np.testing.assert_array_equal(x, y, err_msg=f"{a.size} x {b.size}")
        assert st.dir_bytes == st0.dir_bytes
        np.testing.assert_array_equal(nwhip.score_batch_dual_banded(pairs, mat, band=w, **k), sc0)


@pytest.mark.parametrize("pc,single", [(EQUAL, (-2, -3)), ((-2, -1, -4, -2), (-1, -2)), (FLAT, (-2, -1))], ids=str)
@pytest.mark.parametrize("w", [0, 31, 200])
def test_equal_or_dominated_pieces_are_align_batch_banded_byte_for_byte(w, pc, single):
    pairs, mat = ops_pairs20() + score_pairs(20), matrix(20)
    sc0, ops0, st0 = nwhip.align_batch_banded(pairs, mat, single[0], single[1], band=w)
    sc, ops, st = nwhip.align_batch_dual_banded(pairs, mat, **kw(pc, w))
    np.testing.assert_array_equal(sc, sc0)
    for (a, b), x, y in zip(pairs, ops, ops0):
        np.testing.assert_array_equal(x, y, err_msg=f"{a.size} x {b.size}")
    assert st.dir_bytes == 2 * st0.dir_bytes
    np.testing.assert_array_equal(nwhip.score_batch_dual_banded(pairs, mat, **kw(pc, w)), sc0)


# ------------------------------------------------------------------ directed pairs
@pytest.mark.parametrize("tall", [False, True])
def test_the_two_run_pair_at_the_band_that_recovers_it(tall):
    """850 x 553, 300 columns and 3 rows planted: 766 at w = TWO_RUNS_W (the host file finds it),
    less at w = 0; the 300-run is priced by the flat piece inside a single-digit band."""
    mat = uniform()
    a, b = two_runs_pair()
    s1, s2 = (b, a) if tall else (a, b)
    long_op, short_op = (1, 2) if tall else (2, 1)
    for waves in (0, 1):
        sc, ops, st = nwhip.align_batch_dual_banded([(s1, s2)], mat, waves=waves, **kw(MM, TWO_RUNS_W))
        assert sc[0] == 766 == nwhip.score_batch_dual_banded([(s1, s2)], mat, waves=waves, **kw(MM, TWO_RUNS_W))[0]
        check_alignments([(s1, s2)], mat, MM, TWO_RUNS_W, sc, ops)
        (start, length), = nw_gotoh.runs(ops[0], long_op)
        assert length == 300 and 180 <= start <= 200
        (start, length), = nw_gotoh.runs(ops[0], short_op)
        assert length == 3 and start > 600
        assert st.dir_bytes == nwhip.batch_dual_banded_dir_bytes(s1.size, s2.size, TWO_RUNS_W)
        assert st.dir_bytes <= nwhip.batch_dual_dir_bytes(s1.size, s2.size)
    low = nwhip.score_batch_dual_banded([(s1, s2)], mat, **kw(MM, 0))[0]
    assert low < 766 and low == b2.score(s1, s2, mat.scores, mat.index, MM, 0)


@pytest.mark.parametrize("k,want", [(19, 758), (20, 756), (21, 755)])
def test_a_run_at_the_crossover_length_inside_a_band_of_32(k, want):
    mat = uniform()
    a, b = planted(150, k, 250, 31)
    for s1, s2, op in ((a, b, 2), (b, a, 1)):
        sc, ops, _ = nwhip.align_batch_dual_banded([(s1, s2)], mat, **kw(MM, 32))
        assert sc[0] == want == nwhip.score_batch_dual_banded([(s1, s2)], mat, **kw(MM, 32))[0]
        check_alignments([(s1, s2)], mat, MM, 32, sc, ops)
        (start, length), = nw_gotoh.runs(ops[0], op)
        assert length == k and 130 <= start <= 150 and nw_gotoh.runs(ops[0], 3 - op) == []


@pytest.mark.parametrize("pc", COSTS, ids=str)
def test_the_directed_list(pc):
    """The host file's list (it shows that the band and both pieces matter on it), one call per band."""
    mat = uniform()
    for w in sorted({w for _, _, w in directed()}):
        pairs = [(a, b) for a, b, ww in directed() if ww == w]
        sc, ops, _ = nwhip.align_batch_dual_banded(pairs, mat, **kw(pc, w))
        check_alignments(pairs, mat, pc, w, sc, ops)
        np.testing.assert_array_equal(nwhip.score_batch_dual_banded(pairs, mat, **kw(pc, w)), sc)


# ------------------------------------------------------------------ every unrolled cell's byte, every variant
@functools.lru_cache(maxsize=None)
def cover_matrix(variant):
    sc, index, _ = COVER[variant]
    mat = nwhip.SubMatrix(LETTERS, sc)
    assert (mat.index[LETTERS] == index[LETTERS]).all() and (mat.scores == sc).all()
    return mat


@pytest.mark.parametrize("variant", sorted(COVER))
def test_walks_over_every_cell_instance(variant):
    """The host file's list (its paths read all 4 x 64 x 4 x 13 combinations) through the
    directions kernel and the walk -- the default grid, then one worker -- and the score kernel;
    one call per band."""
    pc, mat = COVER[variant][2], cover_matrix(variant)
    for w in sorted({w for _, _, w in cases()}):
        idx = [k for k, (_, _, ww) in enumerate(cases()) if ww == w]
        pairs = [cases()[k][:2] for k in idx]
        want = [results(variant)[k] for k in idx]
        scores = np.array([r.score for r in want], np.int32)
        for waves in (0, 1):
            sc, ops, st = nwhip.align_batch_dual_banded(pairs, mat, waves=waves, **kw(pc, w))
            np.testing.assert_array_equal(sc, scores)
            bad = [(k, a.size, b.size) for k, ((a, b), x, y) in enumerate(zip(pairs, ops, want))
                   if x.size != y.ops.size or (x != y.ops).any()]
            assert not bad, f"w {w}: {len(bad)} of {len(ops)} pairs (index, n1, n2): {bad[:8]}"
            np.testing.assert_array_equal(nwhip.score_batch_dual_banded(pairs, mat, waves=waves, **kw(pc, w)), scores)


# ------------------------------------------------------------------ chunks
def test_three_chunks_against_one():
    rng = np.random.default_rng(23)
    mat = matrix(20)
    pairs = [(_rand(rng, int(rng.integers(280, 321)), 20), _rand(rng, int(rng.integers(280, 320)), 20))
             for _ in range(40)]
    w = 20
    size = lambda a, b: nwhip.batch_dual_banded_dir_bytes(a.size, b.size, w)
    sc0, ops0, st0 = nwhip.align_batch_dual_banded(pairs, mat, **kw(MM, w))
    assert st0.chunks == 1 and st0.dir_bytes == sum(size(a, b) for a, b in pairs)
    want = want_of(pairs, mat, MM, w)
    check_alignments(pairs, mat, MM, w, sc0, ops0, want)
    # 14 pairs' worth of the banded direction bytes for 40 pairs: three chunks at the least
    one = max(size(a, b) for a, b in pairs)
    sc, ops, st = nwhip.align_batch_dual_banded(pairs, mat, mem_bytes=14 * one, **kw(MM, w))
    assert st.chunks >= 3 and st.peak_bytes <= 14 * one and st.dir_bytes == st0.dir_bytes
    check_alignments(pairs, mat, MM, w, sc, ops, want)
    with pytest.raises(nwhip.NwError) as e:   # below one pair's direction bytes: that pair does not fit
        nwhip.align_batch_dual_banded(pairs, mat, mem_bytes=one - 1, **kw(MM, w))
    assert e.value.status == nwhip.NW_ERR_OOM


# ------------------------------------------------------------------ device API
def test_context_score_batch_dual_banded_on_a_stream():
    import torch
    pc, w = (-2, -3, -5, -1), 9
    mat = nwhip.SubMatrix(matrix(20).letters, matrix(20).scores, other=1)
    pairs = sorted(score_pairs(20), key=lambda p: -p[0].size * p[1].size)   # longest first, as the device entry asks
    want = np.array([b2.score(a, b, mat.scores, mat.index, pc, w) for a, b in pairs], np.int32)
    s1, off1, s2, off2 = nwhip.batch_csr(pairs)
    ctx = nwhip.Context(0)
    stream = torch.cuda.Stream()
    k = dict(kw(pc, w))
    k.pop("band")
    with torch.cuda.stream(stream):
        d = [torch.from_numpy(x).cuda() for x in (s1, off1, s2, off2)]
        got = ctx.score_batch_dual_banded(d[0], d[1], d[2], d[3], max(SCORE_N2), mat, stream=stream, **kw(pc, w))
        # the unbanded entry on the scratch the banded launch left, then the banded one again on two workers
        old = ctx.score_batch_dual(d[0], d[1], d[2], d[3], max(SCORE_N2), mat, stream=stream, **k)
        got2 = ctx.score_batch_dual_banded(d[0], d[1], d[2], d[3], 200, mat, stream=stream, waves=2, **kw(pc, w))
        big = ctx.score_batch_dual_banded(d[0], d[1], d[2], d[3], max(SCORE_N2), mat, stream=stream, **kw(pc, 2 ** 40))
        # max_n2 below a pair's rows: that pair is refused (INT32_MIN), the others computed
        low = ctx.score_batch_dual_banded(d[0], d[1], d[2], d[3], 65, mat, stream=stream, **kw(pc, w))
    stream.synchronize()
    assert ctx.status(stream) == nwhip.NW_OK
    for g in (got, got2):
        np.testing.assert_array_equal(g.cpu().numpy(), want)
    np.testing.assert_array_equal(old.cpu().numpy(), nwhip.score_batch_dual(pairs, mat, **k))
    np.testing.assert_array_equal(big.cpu().numpy(), old.cpu().numpy())
    low = low.cpu().numpy()
    n2 = np.diff(off2)
    assert (n2 > 65).any() and (n2 <= 65).any()
    np.testing.assert_array_equal(low[n2 <= 65], want[n2 <= 65])
    assert (low[n2 > 65] == I32_MIN).all()
    with pytest.raises(ValueError):   # a matrix that leaves bytes unlisted
        ctx.score_batch_dual_banded(d[0], d[1], d[2], d[3], 65, matrix(20), stream=stream, **kw(pc, w))
    ctx.close()


# ------------------------------------------------------------------ the whole int8 span
@pytest.mark.parametrize("ge1", [-1, -64, 0, 1])
def test_full_int8_span(ge1):
    """A matrix holding -128 and 127: with ge1 = -1 the table byte s - 2 ge1 leaves int8 upwards,
    with -64 it is far outside, with +1 it leaves it downwards; 0 keeps the bytes as they are.
    Piece 2 crosses piece 1 in every case; dge is -2, -26, -2 and -1 ... of either sign over the set."""
    pc = {-1: (-4, -1, -1, -3), -64: (-300, -64, -3, -90), 0: (-3, 0, 0, -2), 1: (-6, 1, -1, 0)}[ge1]
    rng = np.random.default_rng(41)
    sc = rng.integers(-128, 128, (8, 8))
    sc[0, 1], sc[1, 0], sc[3, 3], sc[5, 2] = -128, 127, 127, -128
    mat = nwhip.SubMatrix(list(range(1, 9)), sc)
    pairs = [(_rand(rng, 257, 8), _rand(rng, 65, 8)), (_rand(rng, 513, 8), _rand(rng, 130, 8)),
             (_rand(rng, 520, 8), _rand(rng, 520, 8))]
    for w in (0, 40):
        want = want_of(pairs, mat, pc, w)
        assert nwhip.score_batch_dual_banded(pairs, mat, **kw(pc, w)).tolist() == [s for s, _ in want]
        s, ops, _ = nwhip.align_batch_dual_banded(pairs, mat, **kw(pc, w))
        check_alignments(pairs, mat, pc, w, s, ops, want)
    # piece 2 alone with the steeper piece 1 (dge = +63): the mask under a large positive drift
    pc = (-3, -64, -300, -1)
    want = want_of(pairs, mat, pc, 3)
    s, ops, _ = nwhip.align_batch_dual_banded(pairs, mat, **kw(pc, 3))
    check_alignments(pairs, mat, pc, 3, s, ops, want)


# ------------------------------------------------------------------ empty sides
def test_empty_sides():
    mat = matrix(4)
    ones, twos = (lambda n: np.full(n, 1, np.int8)), (lambda n: np.full(n, 2, np.int8))
    pairs = [(ones(0), twos(9)), (ones(30), twos(0)), (ones(0), twos(0)), (ones(3), twos(2))]
    for w in (0, 5):
        sc, ops, _ = nwhip.align_batch_dual_banded(pairs, mat, **kw(MM, w))
        assert sc[:3].tolist() == [-4 - 18, -24 - 30, 0]      # g(9) by piece 1, g(30) by piece 2, whatever the band
        assert ops[0].tolist() == [1] * 9 and ops[1].tolist() == [2] * 30 and ops[2].size == 0
        check_alignments(pairs, mat, MM, w, sc, ops)
        assert nwhip.score_batch_dual_banded(pairs, mat, **kw(MM, w)).tolist() == sc.tolist()


# ------------------------------------------------------------------ CLI
@pytest.mark.parametrize("extra", [[], ["--score-only"]])
def test_cli_batch_gap2_band(tmp_path, extra):
    """Three pairs over A, C, G, T, the CLI's alphabet without --matrix: one with 30 columns
    planted (the flat piece, inside any band), one with 5 columns and 5 rows planted apart (the
    band of 2 shuts that path out), one random."""
    rng = np.random.default_rng(61)
    acgt = np.frombuffer(b"ACGT", np.int8)
    seq = lambda n: acgt[rng.integers(0, 4, n)]
    x, y, z, u, v = seq(90), seq(70), seq(40), seq(55), seq(35)
    pairs = [(np.concatenate([x, seq(30), y]), np.concatenate([x, y])),
             (np.concatenate([z, seq(5), u, v]), np.concatenate([z, u, seq(5), v])), (seq(257), seq(65))]
    names = []
    for k, (a, b) in enumerate(pairs):
        names.append((tmp_path / f"a{k}.bdna", tmp_path / f"b{k}.bdna"))
        names[-1][0].write_bytes(a.tobytes())
        names[-1][1].write_bytes(b.tobytes())
    lst = tmp_path / "pairs.txt"
    lst.write_text("".join(f"{a} {b}\n" for a, b in names))
    exe = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")
    mat = nwhip.SubMatrix.uniform([ord(c) for c in "ACGT"], 2, -4)
    outs = {}
    for w in (2, 40):
        r = subprocess.run([exe, "--batch", str(lst), "--gap2", "-24,-1", "--gap2-band", str(w), "--gap-open", "-4",
                            "--scheme", "2,-4,-2"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.split("\n")
        int(lines[0])  # the wall time, ms
        want = [b2.score(a, b, mat.scores, mat.index, MM, w) for a, b in pairs]
        assert nwhip.score_batch_dual_banded(pairs, mat, **kw(MM, w)).tolist() == want
        assert lines[1:4] == [f"Score: {s}" for s in want]
        outs[w] = want
    assert outs[2][0] == outs[40][0] == 320 - 54 and outs[2][1] < outs[40][1]
