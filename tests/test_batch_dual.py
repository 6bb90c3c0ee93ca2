"""GPU: batched global alignment under a two-piece affine gap cost (nw_score_batch_dual,
nw_align_batch_dual, nw_score_batch_dual_async; csrc/nw_batch_dual.hip).

Checker: the plain Python recurrence of tests/nw_gotoh2.py (held to the definition, to its
own cell fill and to tests/nw_gotoh_matrix.py by tests/test_batch_dual_host.py); for the
reductions the matrix entries themselves.  The shapes are tests/test_batch.py's -- one lane,
a lane boundary, a strip seam (255 / 256 / 257 columns, three strips at 513), a row-block
boundary (63 / 64 / 65 rows, three blocks at 130), empty sides -- plus what only two pieces
can get wrong: a run at the crossover length, a long run over a seam or a row block priced
by the flat piece next to a short one priced by the steep piece, a third scratch column or
a profile left over from the pair before, and the coverage list of the host file, whose
paths read every unrolled cell's byte in every way the five-state walk can.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import nw_gotoh
import nw_gotoh2 as g2
import nwhip
from conftest import ROOT
from test_batch import SCORE_N2, _rand, ops_pairs, score_pairs
from test_batch_dual_host import (COVER, CROSSING, DOMINATED, MM, PIECES, REDUCTIONS, RUNS, cases, matrix, piece_mix,
                                  planted, results, score_want, two_runs_pair, uniform)
from test_batch_paths_host import LETTERS

pytestmark = pytest.mark.gpu

I32_MIN = np.iinfo(np.int32).min


def kw(pc):
    """The Python entries' keywords of (go1, ge1, go2, ge2)."""
    return dict(gap_open=pc[0], gap=pc[1], gap_open2=pc[2], gap2=pc[3])


def check_alignments(pairs, mat, pc, scores, ops):
    for (a, b), sc, o in zip(pairs, scores, ops):
        tabs = g2.fill(a, b, mat.scores, mat.index, pc)
        assert sc == tabs[0][-1, -1], (a.size, b.size)
        np.testing.assert_array_equal(o, g2.walk(a, b, mat.scores, mat.index, pc, tabs),
                                      err_msg=f"{a.size} x {b.size} pieces {pc}")
        assert max(a.size, b.size) <= o.size <= a.size + b.size
        assert nwhip.ops_score_dual(a, b, o, mat, **kw(pc)) == sc
        assert g2.path_score(a, b, o, mat.scores, mat.index, pc) == sc


# ------------------------------------------------------------------ scores
@pytest.mark.parametrize("pc", PIECES, ids=str)
@pytest.mark.parametrize("alpha", [4, 20, 32])
def test_scores_at_the_pairs_own_index(alpha, pc):
    pairs, mat = score_pairs(alpha), matrix(alpha)
    want = score_want(alpha, pc)
    if pc in CROSSING:
        # both pieces matter on this batch (the count: tests/test_batch_dual_host.py): the
        # expected scores are neither piece's own on more than a third of the larger pairs
        big, mixed = piece_mix(alpha, pc)
        assert 3 * mixed > big
    got, st = nwhip.score_batch_dual(pairs, mat, return_stats=True, **kw(pc))
    np.testing.assert_array_equal(got, want)
    assert st.pairs == len(pairs) and st.cells == sum(a.size * b.size for a, b in pairs)
    assert st.chunks == 1 and 1 <= st.waves <= len(pairs) - 3 and st.fill_ms > 0
    # waves = 3: every worker sweeps a dozen pairs one after the other
    got, st = nwhip.score_batch_dual(pairs, mat, waves=3, return_stats=True, **kw(pc))
    np.testing.assert_array_equal(got, want)
    assert st.waves == 3
    if alpha == 32:
        assert any((a == 32).any() and (b == 32).any() for a, b in pairs)  # letter 31: the last profile row


# ------------------------------------------------------------------ reductions on the device
@pytest.mark.parametrize("pc,single", REDUCTIONS, ids=str)
def test_reductions_are_the_matrix_entries_bytes(pc, single):
    """Equal pieces, a piece 2 nowhere above piece 1, a piece 1 strictly below piece 2: scores,
    ops and n_ops byte for byte align_batch_matrix's under the piece that counts."""
    ge, go = single
    mat = matrix(20)
    pairs = score_pairs(20)
    np.testing.assert_array_equal(nwhip.score_batch_dual(pairs, mat, **kw(pc)),
                                  nwhip.score_batch_matrix(pairs, mat, ge, go))
    rng = np.random.default_rng(77)
    pairs = tuple((_rand(rng, a.size, 20), _rand(rng, b.size, 20)) for a, b in ops_pairs())
    sc, ops, st = nwhip.align_batch_dual(pairs, mat, **kw(pc))
    sc0, ops0, st0 = nwhip.align_batch_matrix(pairs, mat, ge, go)
    np.testing.assert_array_equal(sc, sc0)
    assert len(ops) == len(ops0) == 24
    for (a, b), x, y in zip(pairs, ops, ops0):
        np.testing.assert_array_equal(x, y, err_msg=f"{a.size} x {b.size}")   # (n_ops: the lengths)
    assert st.dir_bytes == 2 * st0.dir_bytes


# ------------------------------------------------------------------ ops
@functools.lru_cache(maxsize=None)
def ops_pairs20():
    """ops_pairs()' sizes, re-drawn over 20 letters."""
    rng = np.random.default_rng(78)
    return tuple((_rand(rng, a.size, 20), _rand(rng, b.size, 20)) for a, b in ops_pairs())


@pytest.mark.parametrize("pc", CROSSING + DOMINATED[2:], ids=str)
def test_ops_are_the_five_state_walks(pc):
    pairs, mat = ops_pairs20(), matrix(20)
    sc, ops, st = nwhip.align_batch_dual(pairs, mat, **kw(pc))
    check_alignments(pairs, mat, pc, sc, ops)
    assert st.chunks == 1
    assert st.dir_bytes == sum(nwhip.batch_dual_dir_bytes(a.size, b.size) for a, b in pairs)
    assert st.peak_bytes > st.dir_bytes and st.walk_ms > 0
    np.testing.assert_array_equal(nwhip.score_batch_dual(pairs, mat, **kw(pc)), sc)


# ------------------------------------------------------------------ directed piece switching
@pytest.mark.parametrize("k,want,one,two", RUNS)
def test_a_run_at_the_crossover_length(k, want, one, two):
    """400 matches and one left-run of k columns: 800 + g(k); piece 1 alone / piece 2 alone give
    the other two columns (held on the checker by tests/test_batch_dual_host.py)."""
    mat = uniform()
    a, b = planted(150, k, 250, 31)
    for s1, s2, op in ((a, b, 2), (b, a, 1)):
        sc, ops, _ = nwhip.align_batch_dual([(s1, s2)], mat, **kw(MM))
        assert sc[0] == want == nwhip.score_batch_dual([(s1, s2)], mat, **kw(MM))[0]
        check_alignments([(s1, s2)], mat, MM, sc, ops)
        (start, length), = nw_gotoh.runs(ops[0], op)      # exactly the planted run
        assert length == k and 130 <= start <= 150 and nw_gotoh.runs(ops[0], 3 - op) == []


@pytest.mark.parametrize("tall", [False, True])
def test_a_long_and_a_short_run_in_one_pair(tall):
    """550 matches, 300 columns inserted across the strip seam at column 256 (the flat piece:
    -324) and 3 rows inserted further on (the steep piece: -10): 1100 - 334 = 766; piece 1
    alone gives 486, piece 2 alone 749.  Tall: the transposed pair, 300 ups over the row
    blocks and a seam, 3 lefts."""
    mat = uniform()
    a, b = two_runs_pair()
    s1, s2 = (b, a) if tall else (a, b)
    long_op, short_op = (1, 2) if tall else (2, 1)
    for waves in (0, 1):
        sc, ops, _ = nwhip.align_batch_dual([(s1, s2)], mat, waves=waves, **kw(MM))
        assert sc[0] == 766 == nwhip.score_batch_dual([(s1, s2)], mat, waves=waves, **kw(MM))[0]
        check_alignments([(s1, s2)], mat, MM, sc, ops)
        (start, length), = nw_gotoh.runs(ops[0], long_op)
        assert length == 300 and 180 <= start <= 200       # the run crosses column (row) 256
        (start, length), = nw_gotoh.runs(ops[0], short_op)
        assert length == 3 and start > 600
        assert ops[0].size == 550 + 303


# ------------------------------------------------------------------ every unrolled cell's byte
@functools.lru_cache(maxsize=None)
def cover_matrix(variant):
    sc, index, _ = COVER[variant]
    mat = nwhip.SubMatrix(LETTERS, sc)
    assert (mat.index[LETTERS] == index[LETTERS]).all() and (mat.scores == sc).all()
    return mat


@pytest.mark.parametrize("variant", sorted(COVER))
def test_walks_over_every_cell_instance(variant):
    """The host file's list (its paths read all 2 x 64 x 4 x 13 combinations) through the
    directions kernel and the walk -- the default grid, then one worker that sweeps every pair
    after the other -- and through the score kernel."""
    pairs, want, pc, mat = cases(), [r[variant] for r in results()], COVER[variant][2], cover_matrix(variant)
    scores = np.array([r.score for r in want], np.int32)
    for waves in (0, 1):
        sc, ops, st = nwhip.align_batch_dual(pairs, mat, waves=waves, **kw(pc))
        np.testing.assert_array_equal(sc, scores)
        bad = [(k, a.size, b.size) for k, ((a, b), x, y) in enumerate(zip(pairs, ops, want))
               if x.size != y.ops.size or (x != y.ops).any()]
        assert not bad, f"{len(bad)} of {len(ops)} pairs (index, n1, n2): {bad[:8]}"
        assert st.chunks == 1 and (waves == 0 or st.waves == 1)
        if waves == 0:
            assert [nwhip.ops_score_dual(a, b, o, mat, **kw(pc)) for (a, b), o in zip(pairs, ops)] == scores.tolist()
        np.testing.assert_array_equal(nwhip.score_batch_dual(pairs, mat, waves=waves, **kw(pc)), scores)


# ------------------------------------------------------------------ chunks
def test_three_chunks_against_one():
    rng = np.random.default_rng(23)
    mat = matrix(20)
    pairs = [(_rand(rng, int(rng.integers(280, 321)), 20), _rand(rng, int(rng.integers(280, 320)), 20))
             for _ in range(40)]
    sc0, ops0, st0 = nwhip.align_batch_dual(pairs, mat, **kw(MM))
    assert st0.chunks == 1
    assert st0.dir_bytes == sum(nwhip.batch_dual_dir_bytes(a.size, b.size) for a, b in pairs)
    want = [g2.score(a, b, mat.scores, mat.index, MM) for a, b in pairs]
    assert sc0.tolist() == want
    # 14 pairs' worth of direction bytes for 40 pairs: three chunks at the least, whatever else is held
    mem = 14 * nwhip.batch_dual_dir_bytes(300, 300)
    sc, ops, st = nwhip.align_batch_dual(pairs, mat, mem_bytes=mem, **kw(MM))
    assert st.chunks >= 3 and st.peak_bytes <= mem and st.dir_bytes == st0.dir_bytes
    assert sc.tolist() == want
    for x, y in zip(ops, ops0):
        np.testing.assert_array_equal(x, y)
    for k in (0, 17, 39):
        np.testing.assert_array_equal(ops[k], g2.walk(pairs[k][0], pairs[k][1], mat.scores, mat.index, MM))
    # below one pair's direction bytes: that pair does not fit
    with pytest.raises(nwhip.NwError) as e:
        nwhip.align_batch_dual(pairs, mat, mem_bytes=nwhip.batch_dual_dir_bytes(300, 300) - 1, **kw(MM))
    assert e.value.status == nwhip.NW_ERR_OOM


# ------------------------------------------------------------------ device API
def test_context_score_batch_dual_on_a_stream():
    import torch
    pc = (-2, -3, -5, -1)
    mat = nwhip.SubMatrix(matrix(20).letters, matrix(20).scores, other=1)
    pairs = sorted(score_pairs(20), key=lambda p: -p[0].size * p[1].size)   # longest first, as the device entry asks
    want = np.array([g2.score(a, b, mat.scores, mat.index, pc) for a, b in pairs], np.int32)
    np.testing.assert_array_equal(nwhip.score_batch_dual(pairs, mat, **kw(pc)), want)
    s1, off1, s2, off2 = nwhip.batch_csr(pairs)
    ctx = nwhip.Context(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = [torch.from_numpy(x).cuda() for x in (s1, off1, s2, off2)]
        got = ctx.score_batch_dual(d[0], d[1], d[2], d[3], max(SCORE_N2), mat, stream=stream, **kw(pc))
        # a second launch on the same context and stream, then a matrix one on the three-column
        # scratch the two-piece launches left, then the two-piece one again
        got2 = ctx.score_batch_dual(d[0], d[1], d[2], d[3], 200, mat, stream=stream, waves=2, **kw(pc))
        old = ctx.score_batch_matrix(d[0], d[1], d[2], d[3], max(SCORE_N2), mat, -3, -2, stream=stream)
        got3 = ctx.score_batch_dual(d[0], d[1], d[2], d[3], max(SCORE_N2), mat, stream=stream, **kw(pc))
        # max_n2 below a pair's rows: that pair is refused (INT32_MIN), the others computed
        low = ctx.score_batch_dual(d[0], d[1], d[2], d[3], 65, mat, stream=stream, **kw(pc))
    stream.synchronize()
    assert ctx.status(stream) == nwhip.NW_OK
    for g in (got, got2, got3):
        np.testing.assert_array_equal(g.cpu().numpy(), want)
    np.testing.assert_array_equal(old.cpu().numpy(), nwhip.score_batch_matrix(pairs, mat, -3, -2))
    low = low.cpu().numpy()
    n2 = np.diff(off2)
    assert (n2 > 65).any() and (n2 <= 65).any()
    np.testing.assert_array_equal(low[n2 <= 65], want[n2 <= 65])
    assert (low[n2 > 65] == I32_MIN).all()
    with pytest.raises(ValueError):   # a matrix that leaves bytes unlisted
        ctx.score_batch_dual(d[0], d[1], d[2], d[3], 65, matrix(20), stream=stream, **kw(pc))
    ctx.close()


def test_nothing_leaks_from_the_pair_before():
    """One worker, in this order: 513 x 130 over letters 0..15 (three strips, each with its own
    profile, and all three scratch columns), 5 x 130 over letters 16..31 (a stale profile row or
    a stale scratch column -- the third one too -- shows here), 257 x 1."""
    rng = np.random.default_rng(43)
    mat = matrix(32)
    lo, hi = (lambda n: _rand(rng, n, 16)), (lambda n: (_rand(rng, n, 16) + 16).astype(np.int8))
    pairs = [(lo(513), lo(130)), (hi(5), hi(130)), (_rand(rng, 257, 32), _rand(rng, 1, 32))]
    for pc in [MM, (-2, -3, -5, -1)]:
        want = [g2.score(a, b, mat.scores, mat.index, pc) for a, b in pairs]
        got, st = nwhip.score_batch_dual(pairs, mat, waves=1, return_stats=True, **kw(pc))
        assert st.waves == 1 and got.tolist() == want
        sc, ops, st = nwhip.align_batch_dual(pairs, mat, waves=1, **kw(pc))
        assert st.waves == 1
        check_alignments(pairs, mat, pc, sc, ops)
    # the device entry claims pairs in index order: the same three, one worker
    import torch
    full = nwhip.SubMatrix(mat.letters, mat.scores, other=1)
    ctx = nwhip.Context(0)
    d = [torch.from_numpy(x).cuda() for x in nwhip.batch_csr(pairs)]
    got = ctx.score_batch_dual(d[0], d[1], d[2], d[3], 130, full, waves=1, **kw(MM))
    torch.cuda.synchronize()
    assert got.cpu().numpy().tolist() == [g2.score(a, b, mat.scores, mat.index, MM) for a, b in pairs]
    ctx.close()


# ------------------------------------------------------------------ the whole int8 span
@pytest.mark.parametrize("ge1", [-1, -64, 0, 1])
def test_full_int8_span(ge1):
    """A matrix holding -128 and 127: with ge1 = -1 the table byte s - 2 ge1 leaves int8 upwards,
    with -64 it is far outside, with +1 it leaves it downwards; 0 keeps the bytes as they are.
    Piece 2 crosses piece 1 in every case."""
    pc = {-1: (-4, -1, -1, -3), -64: (-300, -64, -3, -90), 0: (-3, 0, 0, -2), 1: (-6, 1, -1, 0)}[ge1]
    k = np.arange(1, 200)
    one = pc[0] + k * pc[1] >= pc[2] + k * pc[3]
    assert one.any() and (~one).any()
    rng = np.random.default_rng(41)
    sc = rng.integers(-128, 128, (8, 8))
    sc[0, 1], sc[1, 0], sc[3, 3], sc[5, 2] = -128, 127, 127, -128
    mat = nwhip.SubMatrix(list(range(1, 9)), sc)
    pairs = [(_rand(rng, 257, 8), _rand(rng, 65, 8)), (_rand(rng, 513, 8), _rand(rng, 130, 8))]
    want = [g2.score(a, b, mat.scores, mat.index, pc) for a, b in pairs]
    assert nwhip.score_batch_dual(pairs, mat, **kw(pc)).tolist() == want
    s, ops, _ = nwhip.align_batch_dual(pairs, mat, **kw(pc))
    check_alignments(pairs, mat, pc, s, ops)


# ------------------------------------------------------------------ empty sides
def test_empty_sides():
    mat = matrix(4)
    ones, twos = (lambda n: np.full(n, 1, np.int8)), (lambda n: np.full(n, 2, np.int8))
    pairs = [(ones(0), twos(9)), (ones(30), twos(0)), (ones(0), twos(0)), (ones(3), twos(2))]
    sc, ops, _ = nwhip.align_batch_dual(pairs, mat, **kw(MM))
    assert sc[:3].tolist() == [-4 - 18, -24 - 30, 0]      # g(9) by piece 1, g(30) by piece 2
    assert ops[0].tolist() == [1] * 9 and ops[1].tolist() == [2] * 30 and ops[2].size == 0
    check_alignments(pairs, mat, MM, sc, ops)
    assert nwhip.score_batch_dual(pairs, mat, **kw(MM)).tolist() == sc.tolist()


# ------------------------------------------------------------------ CLI
@pytest.mark.parametrize("extra", [[], ["--score-only"]])
def test_cli_batch_gap2(tmp_path, extra):
    """Three pairs over A, C, G, T, the CLI's alphabet without --matrix: one with 30 columns
    planted (the flat piece), one with 3 (the steep piece), one random."""
    rng = np.random.default_rng(61)
    acgt = np.frombuffer(b"ACGT", np.int8)
    seq = lambda n: acgt[rng.integers(0, 4, n)]
    x, y, z, w = seq(90), seq(70), seq(40), seq(55)
    pairs = [(np.concatenate([x, seq(30), y]), np.concatenate([x, y])),
             (np.concatenate([z, w]), np.concatenate([z, seq(3), w])), (seq(257), seq(65))]
    names = []
    for k, (a, b) in enumerate(pairs):
        names.append((tmp_path / f"a{k}.bdna", tmp_path / f"b{k}.bdna"))
        names[-1][0].write_bytes(a.tobytes())
        names[-1][1].write_bytes(b.tobytes())
    lst = tmp_path / "pairs.txt"
    lst.write_text("".join(f"{a} {b}\n" for a, b in names))
    exe = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")
    r = subprocess.run([exe, "--batch", str(lst), "--gap2", "-24,-1", "--gap-open", "-4", "--scheme", "2,-4,-2"] + extra,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    int(lines[0])  # the wall time, ms
    mat = nwhip.SubMatrix.uniform([ord(c) for c in "ACGT"], 2, -4)
    want = nwhip.score_batch_dual(pairs, mat, **kw(MM))
    assert want.tolist() == [g2.score(a, b, mat.scores, mat.index, MM) for a, b in pairs]
    assert want[0] == 320 - 54 and want[1] == 190 - 10
    assert lines[1:4] == [f"Score: {w}" for w in want]
