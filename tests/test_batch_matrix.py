"""GPU: batched pairwise alignment with a substitution matrix (nw_score_batch_matrix,
nw_align_batch_matrix, nw_score_batch_matrix_async; csrc/nw_batch_matrix.hip).

Checker: the plain Python Gotoh with a matrix of tests/nw_gotoh_matrix.py (anchored to
tests/nw_gotoh.py by tests/test_batch_matrix_host.py); for identity-type matrices also the
affine and the linear entries themselves.  The shapes are tests/test_batch.py's -- one
lane, a lane boundary, a strip seam (255 / 256 / 257 columns, three strips at 513), a
row-block boundary (63 / 64 / 65 rows, three blocks at 130), empty sides -- plus what only
a matrix can get wrong: the last profile row (letter 31), a transposed lookup, table
bytes that leave int8 in either direction, a profile left over from the strip or the pair
before, one letter, a wildcard.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import nw_gotoh
import nw_gotoh_matrix as gm
import nwhip
from conftest import ROOT, bdna_path, read_bdna
from test_batch import SCHEMES, SCORE_N2, _rand, ops_pairs, score_pairs
from test_batch_matrix_host import identity_matrix, random_matrix

pytestmark = pytest.mark.gpu

I32_MIN = np.iinfo(np.int32).min


@functools.lru_cache(maxsize=None)
def matrix(alpha):
    """Seeded, asymmetric, entries in -8..12, over the bytes 1..alpha (letter k = byte k + 1)."""
    m = random_matrix(np.random.default_rng(500 + alpha), alpha)
    assert (m.scores != m.scores.T).any()
    return m


@functools.lru_cache(maxsize=None)
def score_want(alpha, ge, go, transposed=False):
    m = matrix(alpha)
    sc = m.scores.T if transposed else m.scores
    return np.array([gm.score(a, b, sc, m.index, ge, go) for a, b in score_pairs(alpha)], np.int32)


def check_alignments(pairs, mat, ge, go, scores, ops):
    for (a, b), sc, o in zip(pairs, scores, ops):
        tables = gm.fill(a, b, mat.scores, mat.index, ge, go)
        assert sc == tables[0][-1, -1], (a.size, b.size)
        np.testing.assert_array_equal(o, gm.walk(a, b, mat.scores, mat.index, ge, go, tables),
                                      err_msg=f"{a.size} x {b.size} ge {ge} go {go}")
        assert max(a.size, b.size) <= o.size <= a.size + b.size
        assert nwhip.ops_score_matrix(a, b, o, mat, ge, go) == sc
        assert gm.path_score(a, b, o, mat.scores, mat.index, ge, go) == sc


# ------------------------------------------------------------------ scores
@pytest.mark.parametrize("ge,go", [(-1, -1), (-1, -11), (-2, -1), (-2, -11)])
@pytest.mark.parametrize("alpha", [4, 20, 32])
def test_scores_at_the_pairs_own_index(alpha, ge, go):
    pairs, mat = score_pairs(alpha), matrix(alpha)
    want = score_want(alpha, ge, go)
    # the asymmetry matters on this batch: a transposed lookup cannot pass
    assert (score_want(alpha, ge, go, True) != want).any()
    got, st = nwhip.score_batch_matrix(pairs, mat, ge, go, return_stats=True)
    np.testing.assert_array_equal(got, want)
    assert st.pairs == len(pairs) and st.cells == sum(a.size * b.size for a, b in pairs)
    assert st.chunks == 1 and 1 <= st.waves <= len(pairs) - 3 and st.fill_ms > 0
    # waves = 3: every worker sweeps a dozen pairs one after the other
    got, st = nwhip.score_batch_matrix(pairs, mat, ge, go, waves=3, return_stats=True)
    np.testing.assert_array_equal(got, want)
    assert st.waves == 3
    if alpha == 32:
        assert any((a == 32).any() and (b == 32).any() for a, b in pairs)  # letter 31: the last profile row


# ------------------------------------------------------------------ identity matrices
@pytest.mark.parametrize("go", [-3, -11, 0])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_identity_matrix_is_the_affine_batch(scheme, go):
    """match / mismatch over the letters 1..9 as a matrix: scores and ops byte-equal to the
    affine entries', and with gap_open = 0 to the linear ones'."""
    mat = identity_matrix(list(range(1, 10)), scheme[0], scheme[1])
    pairs = score_pairs(9)
    got = nwhip.score_batch_matrix(pairs, mat, scheme[2], go)
    np.testing.assert_array_equal(got, nwhip.score_batch_affine(pairs, scheme, go))
    pairs = ops_pairs()
    sc, ops, st = nwhip.align_batch_matrix(pairs, mat, scheme[2], go)
    sc0, ops0, st0 = nwhip.align_batch_affine(pairs, scheme, go)
    np.testing.assert_array_equal(sc, sc0)
    assert len(ops) == len(ops0) == 24
    for (a, b), x, y in zip(pairs, ops, ops0):
        np.testing.assert_array_equal(x, y, err_msg=f"{a.size} x {b.size}")
    assert st.dir_bytes == st0.dir_bytes
    if go == 0:
        np.testing.assert_array_equal(got, nwhip.score_batch(score_pairs(9), scheme))
        sc1, ops1, _ = nwhip.align_batch(pairs, scheme)
        np.testing.assert_array_equal(sc, sc1)
        for x, y in zip(ops, ops1):
            np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------ ops
@functools.lru_cache(maxsize=None)
def ops_pairs20():
    """ops_pairs()' sizes, re-drawn over 20 letters."""
    rng = np.random.default_rng(77)
    return tuple((_rand(rng, a.size, 20), _rand(rng, b.size, 20)) for a, b in ops_pairs())


@pytest.mark.parametrize("ge,go", [(-1, -11), (-2, -3)])
def test_ops_are_the_three_state_walks(ge, go):
    pairs, mat = ops_pairs20(), matrix(20)
    sc, ops, st = nwhip.align_batch_matrix(pairs, mat, ge, go)
    check_alignments(pairs, mat, ge, go, sc, ops)
    assert st.chunks == 1
    assert st.dir_bytes == sum(nwhip.batch_affine_dir_bytes(a.size, b.size) for a, b in pairs)
    assert st.peak_bytes > st.dir_bytes and st.walk_ms > 0
    np.testing.assert_array_equal(nwhip.score_batch_matrix(pairs, mat, ge, go), sc)


# ------------------------------------------------------------------ the whole int8 span
@pytest.mark.parametrize("ge,go", [(-1, -11), (-64, -11), (0, -3), (1, -1)])
def test_full_int8_span(ge, go):
    """A matrix holding -128 and 127: with gap -1 the table byte s - 2 ge leaves int8 upwards,
    with gap -64 it is far outside, with gap +1 it leaves it downwards; gap 0 keeps the
    bytes as they are."""
    rng = np.random.default_rng(41)
    sc = rng.integers(-128, 128, (8, 8))
    sc[0, 1], sc[1, 0], sc[3, 3], sc[5, 2] = -128, 127, 127, -128
    mat = nwhip.SubMatrix(list(range(1, 9)), sc)
    pairs = [(_rand(rng, 257, 8), _rand(rng, 65, 8)), (_rand(rng, 513, 8), _rand(rng, 130, 8))]
    want = [gm.score(a, b, mat.scores, mat.index, ge, go) for a, b in pairs]
    assert nwhip.score_batch_matrix(pairs, mat, ge, go).tolist() == want
    s, ops, _ = nwhip.align_batch_matrix(pairs, mat, ge, go)
    check_alignments(pairs, mat, ge, go, s, ops)


# ------------------------------------------------------------------ profile per strip and per pair
def test_profile_is_per_strip_and_per_pair():
    """One worker, in this order: 513 x 130 over letters 0..15 (three strips, each with its own
    profile, and the scratch columns), 5 x 130 over letters 16..31 (a stale profile row or a
    stale scratch column shows here), 257 x 1."""
    rng = np.random.default_rng(43)
    mat = matrix(32)
    lo, hi = (lambda n: _rand(rng, n, 16)), (lambda n: (_rand(rng, n, 16) + 16).astype(np.int8))
    pairs = [(lo(513), lo(130)), (hi(5), hi(130)), (_rand(rng, 257, 32), _rand(rng, 1, 32))]
    for ge, go in [(-1, -11), (-2, -1)]:
        want = [gm.score(a, b, mat.scores, mat.index, ge, go) for a, b in pairs]
        got, st = nwhip.score_batch_matrix(pairs, mat, ge, go, waves=1, return_stats=True)
        assert st.waves == 1 and got.tolist() == want
        sc, ops, st = nwhip.align_batch_matrix(pairs, mat, ge, go, waves=1)
        assert st.waves == 1
        check_alignments(pairs, mat, ge, go, sc, ops)


# ------------------------------------------------------------------ one long run
@functools.lru_cache(maxsize=None)
def seam_pair():
    rng = np.random.default_rng(29)
    x, ins, y = _rand(rng, 200, 4), _rand(rng, 300, 4), _rand(rng, 100, 4)
    return np.concatenate([x, ins, y]), np.concatenate([x, y])


@pytest.mark.parametrize("tall", [False, True])
def test_one_long_run_across_the_seams(tall):
    """a = x + ins + y against b = x + y under a matrix with 5 on the diagonal and an asymmetric
    -4..-2 off it: 300 matches and ONE run of 300 gap ops is the optimum (b has 300 characters,
    and a second run costs another gap_open).  Wide: 300 lefts over the strip seam at column
    256 / 257.  Tall: 300 ups over the row blocks."""
    sc = np.random.default_rng(47).integers(-4, -1, (4, 4))
    sc[np.arange(4), np.arange(4)] = 5
    mat = nwhip.SubMatrix([1, 2, 3, 4], sc)
    ge, go = -1, -10
    a, b = seam_pair()
    s1, s2 = (b, a) if tall else (a, b)
    op = 1 if tall else 2
    want = gm.walk(s1, s2, mat.scores, mat.index, ge, go)
    (start, length), = nw_gotoh.runs(want, op)
    assert length == 300 and 190 <= start <= 200
    assert nw_gotoh.runs(want, 3 - op) == [] and want.size == 600
    for waves in (0, 1):
        s, ops, _ = nwhip.align_batch_matrix([(s1, s2)], mat, ge, go, waves=waves)
        np.testing.assert_array_equal(ops[0], want)
        assert s[0] == gm.score(s1, s2, mat.scores, mat.index, ge, go) == 300 * 5 - 10 - 300
        assert nwhip.score_batch_matrix([(s1, s2)], mat, ge, go, waves=waves)[0] == s[0]


# ------------------------------------------------------------------ alphabets at the edges
def test_one_letter():
    """n = 1: every byte maps to the one letter."""
    rng = np.random.default_rng(53)
    mat = nwhip.SubMatrix([7], [[3]], other=7)
    pairs = [(rng.integers(-128, 128, n1).astype(np.int8), rng.integers(-128, 128, n2).astype(np.int8))
             for n1, n2 in [(1, 1), (5, 64), (257, 65), (40, 0)]]
    sc, ops, _ = nwhip.align_batch_matrix(pairs, mat, -1, -4)
    check_alignments(pairs, mat, -1, -4, sc, ops)
    assert sc.tolist() == [3, 3 * 5 - 4 - 59, 3 * 65 - 4 - 192, -4 - 40]
    assert nwhip.score_batch_matrix(pairs, mat, -1, -4).tolist() == sc.tolist()


def test_wildcard():
    """A wildcard letter scoring +1 against everything; unlisted bytes (also negative ones) map to it."""
    rng = np.random.default_rng(59)
    sc = np.full((5, 5), -3, np.int64)
    sc[np.arange(4), np.arange(4)] = 4
    sc[4, :] = sc[:, 4] = 1
    mat = nwhip.SubMatrix([1, 2, 3, 4, ord("X")], sc, other="X")
    odd = np.array([0, 9, ord("X"), -5, -128, 127], np.int8)

    def seq(n):
        s = _rand(rng, n, 4)
        mask = rng.random(n) < 0.2
        s[mask] = rng.choice(odd, int(mask.sum()))
        return s
    pairs = [(seq(n1), seq(n2)) for n1, n2 in [(5, 3), (255, 64), (300, 130)]]
    sc_, ops, _ = nwhip.align_batch_matrix(pairs, mat, -1, -5)
    check_alignments(pairs, mat, -1, -5, sc_, ops)
    assert nwhip.score_batch_matrix(pairs, mat, -1, -5).tolist() == sc_.tolist()
    # all wildcards against anything: +1 per column
    assert nwhip.score_batch_matrix([(np.full(70, 9, np.int8), _rand(rng, 70, 4))], mat, -1, -5)[0] == 70


def test_empty_sides():
    mat = matrix(4)
    ones, twos = (lambda n: np.full(n, 1, np.int8)), (lambda n: np.full(n, 2, np.int8))
    pairs = [(ones(0), twos(9)), (ones(9), twos(0)), (ones(0), twos(0)), (ones(3), twos(2))]
    sc, ops, _ = nwhip.align_batch_matrix(pairs, mat, -2, -5)
    assert sc[:3].tolist() == [-5 - 18, -5 - 18, 0]
    assert ops[0].tolist() == [1] * 9 and ops[1].tolist() == [2] * 9 and ops[2].size == 0
    check_alignments(pairs, mat, -2, -5, sc, ops)
    assert nwhip.score_batch_matrix(pairs, mat, -2, -5).tolist() == sc.tolist()


# ------------------------------------------------------------------ chunks
def test_three_chunks_against_one():
    rng = np.random.default_rng(23)
    mat = matrix(20)
    pairs = [(_rand(rng, int(rng.integers(280, 321)), 20), _rand(rng, int(rng.integers(280, 320)), 20))
             for _ in range(40)]
    ge, go = -1, -11
    sc0, ops0, st0 = nwhip.align_batch_matrix(pairs, mat, ge, go)
    assert st0.chunks == 1
    assert st0.dir_bytes == sum(nwhip.batch_affine_dir_bytes(a.size, b.size) for a, b in pairs)
    want = [gm.score(a, b, mat.scores, mat.index, ge, go) for a, b in pairs]
    assert sc0.tolist() == want
    # 14 pairs' worth of direction bytes for 40 pairs: three chunks at the least, whatever else is held
    mem = 14 * nwhip.batch_affine_dir_bytes(300, 300)
    sc, ops, st = nwhip.align_batch_matrix(pairs, mat, ge, go, mem_bytes=mem)
    assert st.chunks >= 3 and st.peak_bytes <= mem and st.dir_bytes == st0.dir_bytes
    assert sc.tolist() == want
    for x, y in zip(ops, ops0):
        np.testing.assert_array_equal(x, y)
    for k in (0, 17, 39):
        np.testing.assert_array_equal(ops[k], gm.walk(pairs[k][0], pairs[k][1], mat.scores, mat.index, ge, go))
    # below one pair's direction bytes: that pair does not fit
    with pytest.raises(nwhip.NwError) as e:
        nwhip.align_batch_matrix(pairs, mat, ge, go, mem_bytes=nwhip.batch_affine_dir_bytes(300, 300) - 1)
    assert e.value.status == nwhip.NW_ERR_OOM


# ------------------------------------------------------------------ device API
def test_context_score_batch_matrix_on_a_stream():
    import torch
    ge, go = -2, -3
    mat = nwhip.SubMatrix(matrix(20).letters, matrix(20).scores, other=1)
    # longest first, as the device entry asks
    pairs = sorted(score_pairs(20), key=lambda p: -p[0].size * p[1].size)
    want = np.array([gm.score(a, b, mat.scores, mat.index, ge, go) for a, b in pairs], np.int32)
    s1, off1, s2, off2 = nwhip.batch_csr(pairs)
    ctx = nwhip.Context(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = [torch.from_numpy(x).cuda() for x in (s1, off1, s2, off2)]
        got = ctx.score_batch_matrix(d[0], d[1], d[2], d[3], max(SCORE_N2), mat, ge, go, stream=stream)
        # a second launch on the same context and stream: its workspace is reused
        got2 = ctx.score_batch_matrix(d[0], d[1], d[2], d[3], 200, mat, ge, go, stream=stream, waves=2)
        # an affine and a linear one after it, on the rows and the scratch the matrix launches left
        aff = ctx.score_batch_affine(d[0], d[1], d[2], d[3], max(SCORE_N2), (2, -1, -2), go, stream=stream)
        lin = ctx.score_batch(d[0], d[1], d[2], d[3], max(SCORE_N2), (2, -1, -2), stream=stream)
        got3 = ctx.score_batch_matrix(d[0], d[1], d[2], d[3], max(SCORE_N2), mat, ge, go, stream=stream)
    stream.synchronize()
    assert ctx.status(stream) == nwhip.NW_OK
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(got2.cpu().numpy(), want)
    np.testing.assert_array_equal(got3.cpu().numpy(), want)
    np.testing.assert_array_equal(aff.cpu().numpy(), nwhip.score_batch_affine(pairs, (2, -1, -2), go))
    np.testing.assert_array_equal(lin.cpu().numpy(), nwhip.score_batch(pairs, (2, -1, -2)))
    # max_n2 below a pair's rows: that pair is refused (INT32_MIN), the others computed
    with torch.cuda.stream(stream):
        low = ctx.score_batch_matrix(d[0], d[1], d[2], d[3], 65, mat, ge, go, stream=stream)
    stream.synchronize()
    low = low.cpu().numpy()
    n2 = np.diff(off2)
    np.testing.assert_array_equal(low[n2 <= 65], want[n2 <= 65])
    assert (low[n2 > 65] == I32_MIN).all()
    # a matrix that leaves bytes unlisted cannot be used where the sequences are not looked at
    with pytest.raises(ValueError):
        ctx.score_batch_matrix(d[0], d[1], d[2], d[3], 65, matrix(20), ge, go, stream=stream)
    ctx.close()


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
def test_cli_batch_matrix(tmp_path, golden, extra):
    """One text file, read by the C++ parser and by SubMatrix.from_text."""
    names = ["small", "debug", "t"]
    files = [(golden["pairs"][n]["argv1"], golden["pairs"][n]["argv2"]) for n in names]
    lst = tmp_path / "pairs.txt"
    lst.write_text("".join(f"{bdna_path(a)} {bdna_path(b)}\n" for a, b in files))
    mfile = tmp_path / "matrix.txt"
    mfile.write_text(MATRIX_TEXT)
    exe = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")
    r = subprocess.run([exe, "--batch", str(lst), "--scheme", "1,-1,-2", "--matrix", str(mfile), "--gap-open", "-11"]
                       + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    int(lines[0])  # the wall time, ms
    mat = nwhip.SubMatrix.from_text(str(mfile))
    assert mat.scores[1, 0] == -2 and mat.scores[0, 1] == -4 and mat.other == ord("*")
    pairs = [(read_bdna(a), read_bdna(b)) for a, b in files]
    want = nwhip.score_batch_matrix(pairs, mat, -2, -11)
    assert want.tolist() == [gm.score(a, b, mat.scores, mat.index, -2, -11) for a, b in pairs]
    assert lines[1:4] == [f"Score: {w}" for w in want]


def test_cli_matrix_needs_batch(tmp_path):
    """No device work: --matrix without --batch, a file that is no matrix, and a sequence byte
    the matrix does not list are refused with a message."""
    exe = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")
    a, b = bdna_path("small1.bdna"), bdna_path("small2.bdna")
    mfile = tmp_path / "matrix.txt"
    mfile.write_text(MATRIX_TEXT)
    r = subprocess.run([exe, a, b, "--matrix", str(mfile)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--matrix needs --batch" in r.stdout
    lst = tmp_path / "pairs.txt"
    lst.write_text(f"{a} {b}\n")
    bad = tmp_path / "bad.txt"
    bad.write_text("0x01 0x02\n0x01 1 300\n0x02 1 1\n")
    r = subprocess.run([exe, "--batch", str(lst), "--matrix", str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--matrix" in r.stdout and "-128..127" in r.stdout
    strict = tmp_path / "strict.txt"
    strict.write_text("0x01 0x02\n0x01 1 0\n0x02 0 1\n")  # the files hold 3 and 4 too
    r = subprocess.run([exe, "--batch", str(lst), "--matrix", str(strict)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "not a letter of the matrix" in r.stdout
