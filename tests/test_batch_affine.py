"""GPU: batched pairwise alignment under affine gap cost (nw_score_batch_affine,
nw_align_batch_affine, nw_score_batch_affine_async; csrc/nw_batch_affine.hip).

Checkers: the plain Python Gotoh of tests/nw_gotoh.py (fill and three-state walk) and,
for gap_open = 0, the linear entries nw_score_batch / nw_align_batch.  The shapes are
tests/test_batch.py's -- one lane, a lane boundary, a strip boundary (255 / 256 / 257
columns, three strips at 513), a row-block boundary (63 / 64 / 65 rows, three blocks at
130), empty sides -- plus pairs whose one long gap crosses the strip seam (E carried
over the two-column scratch in the "extended" state) or the row blocks (F likewise), a
worker that takes a short pair after a long one, both substitution forms, chunks.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import nw_gotoh
import nwhip
from conftest import ROOT, bdna_path, read_bdna
from test_batch import SCHEMES, SCORE_N2, _rand, ops_pairs, score_pairs

pytestmark = pytest.mark.gpu

OPENS = [-1, -3, -11]


@functools.lru_cache(maxsize=None)
def score_want(alpha, scheme, go):
    return np.array([nw_gotoh.score(a, b, scheme, go) for a, b in score_pairs(alpha)], np.int32)


def check_alignments(pairs, scheme, go, scores, ops):
    for (a, b), sc, o in zip(pairs, scores, ops):
        tables = nw_gotoh.fill(a, b, scheme, go)
        assert sc == tables[0][-1, -1], (a.size, b.size)
        np.testing.assert_array_equal(o, nw_gotoh.walk(a, b, scheme, go, tables),
                                      err_msg=f"{a.size} x {b.size} {scheme} {go}")
        assert max(a.size, b.size) <= o.size <= a.size + b.size
        assert nwhip.ops_score_affine(a, b, o, scheme, go) == sc
        assert nw_gotoh.path_score_affine(a, b, o, scheme, go) == sc


# ------------------------------------------------------------------ scores
@pytest.mark.parametrize("go", OPENS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_scores_at_the_pairs_own_index(scheme, go):
    pairs = score_pairs()
    want = score_want(4, scheme, go)
    got, st = nwhip.score_batch_affine(pairs, scheme, go, return_stats=True)
    np.testing.assert_array_equal(got, want)
    assert st.pairs == len(pairs) and st.cells == sum(a.size * b.size for a, b in pairs)
    assert st.chunks == 1 and 1 <= st.waves <= len(pairs) - 3 and st.fill_ms > 0
    # waves = 3: every worker sweeps a dozen pairs one after the other
    got, st = nwhip.score_batch_affine(pairs, scheme, go, waves=3, return_stats=True)
    np.testing.assert_array_equal(got, want)
    assert st.waves == 3


# ------------------------------------------------------------------ gap_open = 0
@pytest.mark.parametrize("scheme", SCHEMES)
def test_gap_open_0_is_the_linear_batch(scheme):
    pairs = score_pairs()
    np.testing.assert_array_equal(nwhip.score_batch_affine(pairs, scheme, 0), nwhip.score_batch(pairs, scheme))
    pairs = ops_pairs()
    sc, ops, st = nwhip.align_batch_affine(pairs, scheme, 0)
    sc0, ops0, st0 = nwhip.align_batch(pairs, scheme)
    np.testing.assert_array_equal(sc, sc0)
    assert len(ops) == len(ops0) == 24
    for (a, b), x, y in zip(pairs, ops, ops0):
        np.testing.assert_array_equal(x, y, err_msg=f"{a.size} x {b.size}")
    assert st.dir_bytes == 2 * st0.dir_bytes


# ------------------------------------------------------------------ ops
@pytest.mark.parametrize("go", [-3, -11])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_ops_are_the_three_state_walks(scheme, go):
    pairs = ops_pairs()
    sc, ops, st = nwhip.align_batch_affine(pairs, scheme, go)
    check_alignments(pairs, scheme, go, sc, ops)
    assert st.chunks == 1
    assert st.dir_bytes == sum(nwhip.batch_affine_dir_bytes(a.size, b.size) for a, b in pairs)
    assert st.peak_bytes > st.dir_bytes and st.walk_ms > 0
    np.testing.assert_array_equal(nwhip.score_batch_affine(pairs, scheme, go), sc)


@functools.lru_cache(maxsize=None)
def seam_pair():
    rng = np.random.default_rng(29)
    x, ins, y = _rand(rng, 200, 4), _rand(rng, 300, 4), _rand(rng, 100, 4)
    return np.concatenate([x, ins, y]), np.concatenate([x, y])


@pytest.mark.parametrize("scheme,go", [((1, -1, -1), -10), ((2, -1, -2), -5), ((1, 0, -1), -4)])
@pytest.mark.parametrize("tall", [False, True])
def test_one_long_run_across_the_seams(scheme, go, tall):
    """a = x + ins + y against b = x + y: the path is 200 diags, ONE run of 300 gap ops, 100
    diags.  Wide (a on top): 300 lefts from column 500 down to 201, E "extended" over the
    strip seam at column 256 / 257.  Tall (a down the side): 300 ups over the row blocks at
    256 and 320, F likewise."""
    a, b = seam_pair()
    s1, s2 = (b, a) if tall else (a, b)
    op = 1 if tall else 2
    want = nw_gotoh.walk(s1, s2, scheme, go)
    (start, length), = nw_gotoh.runs(want, op)
    assert length == 300 and 190 <= start <= 200  # (the run may slide left over letters ins shares with x)
    assert nw_gotoh.runs(want, 3 - op) == [] and want.size == 600
    for waves in (0, 1):
        sc, ops, _ = nwhip.align_batch_affine([(s1, s2)], scheme, go, waves=waves)
        np.testing.assert_array_equal(ops[0], want)
        assert sc[0] == nw_gotoh.score(s1, s2, scheme, go) == nw_gotoh.path_score_affine(s1, s2, want, scheme, go)
        assert nwhip.score_batch_affine([(s1, s2)], scheme, go, waves=waves)[0] == sc[0]


@pytest.mark.parametrize("go", [-3, -11])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_short_pair_after_a_long_one_on_the_same_worker(scheme, go):
    """One worker: 513 x 130 (three strips: the scratch holds its H and E columns), then 5 x
    130 and 257 x 1, whose first strips must take the boundary and not the scratch."""
    rng = np.random.default_rng(11)
    pairs = [(_rand(rng, 257, 4), _rand(rng, 1, 4)), (_rand(rng, 513, 4), _rand(rng, 130, 4)),
             (_rand(rng, 5, 4), _rand(rng, 130, 4))]
    want = [nw_gotoh.score(a, b, scheme, go) for a, b in pairs]
    assert nwhip.score_batch_affine(pairs, scheme, go, waves=1).tolist() == want
    sc, ops, st = nwhip.align_batch_affine(pairs, scheme, go, waves=1)
    assert st.waves == 1
    check_alignments(pairs, scheme, go, sc, ops)


# ------------------------------------------------------------------ alphabet
@pytest.mark.parametrize("scheme,go", [((1, 0, -1), -3), ((2, -1, -2), -11)])
def test_alphabets(scheme, go):
    # 9 letters: more than the v_perm tables cover, byte compares
    np.testing.assert_array_equal(nwhip.score_batch_affine(score_pairs(9), scheme, go), score_want(9, scheme, go))
    # 4 letters with the tables switched off
    got = nwhip.score_batch_affine(score_pairs(), scheme, go, flags=nwhip.FLAG_NO_PROFILE)
    np.testing.assert_array_equal(got, score_want(4, scheme, go))
    # a 3-letter s1 next to a 9-letter s1: the batch-wide decision falls to compares
    rng = np.random.default_rng(13)
    pairs = [(_rand(rng, 300, 3), _rand(rng, 200, 9)), (_rand(rng, 270, 9), _rand(rng, 131, 3)),
             (_rand(rng, 40, 3), _rand(rng, 70, 3))]
    assert len(set(np.concatenate([p[0] for p in pairs]).tolist())) == 9
    sc, ops, _ = nwhip.align_batch_affine(pairs, scheme, go)
    check_alignments(pairs, scheme, go, sc, ops)
    assert nwhip.score_batch_affine(pairs, scheme, go).tolist() == sc.tolist()
    sc2, ops2, _ = nwhip.align_batch_affine(pairs, scheme, go, flags=nwhip.FLAG_NO_PROFILE)
    check_alignments(pairs, scheme, go, sc2, ops2)


def test_empty_sides():
    ones, twos = (lambda n: np.full(n, 1, np.int8)), (lambda n: np.full(n, 2, np.int8))
    pairs = [(ones(0), twos(9)), (ones(9), twos(0)), (ones(0), twos(0)), (ones(3), twos(2))]
    scheme, go = (2, -1, -2), -5
    sc, ops, _ = nwhip.align_batch_affine(pairs, scheme, go)
    assert sc[:3].tolist() == [-5 - 18, -5 - 18, 0]
    assert ops[0].tolist() == [1] * 9 and ops[1].tolist() == [2] * 9 and ops[2].size == 0
    check_alignments(pairs, scheme, go, sc, ops)
    assert nwhip.score_batch_affine(pairs, scheme, go).tolist() == sc.tolist()


# ------------------------------------------------------------------ chunks
def test_chunks_fit_the_budget():
    rng = np.random.default_rng(23)
    pairs = [(_rand(rng, int(rng.integers(280, 321)), 4), _rand(rng, int(rng.integers(280, 320)), 4))
             for _ in range(40)]
    scheme, go = (1, -1, -1), -3
    sc0, ops0, st0 = nwhip.align_batch_affine(pairs, scheme, go)
    assert st0.chunks == 1
    assert st0.dir_bytes == sum(nwhip.batch_affine_dir_bytes(a.size, b.size) for a, b in pairs)
    want = [nw_gotoh.score(a, b, scheme, go) for a, b in pairs]
    assert sc0.tolist() == want
    # 14 pairs' worth of direction bytes for 40 pairs: three chunks at the least, whatever else is held
    mem = 14 * nwhip.batch_affine_dir_bytes(300, 300)
    sc, ops, st = nwhip.align_batch_affine(pairs, scheme, go, mem_bytes=mem)
    assert st.chunks >= 3 and st.peak_bytes <= mem and st.dir_bytes == st0.dir_bytes
    assert sc.tolist() == want
    for x, y in zip(ops, ops0):
        np.testing.assert_array_equal(x, y)
    for k in (0, 17, 39):
        np.testing.assert_array_equal(ops[k], nw_gotoh.walk(pairs[k][0], pairs[k][1], scheme, go))
    # below one pair's direction bytes: that pair does not fit
    with pytest.raises(nwhip.NwError) as e:
        nwhip.align_batch_affine(pairs, scheme, go, mem_bytes=nwhip.batch_affine_dir_bytes(300, 300) - 1)
    assert e.value.status == nwhip.NW_ERR_OOM


# ------------------------------------------------------------------ device API
def test_context_score_batch_affine_on_a_stream():
    import torch
    scheme, go = (2, -1, -2), -3
    # longest first, as the device entry asks
    pairs = sorted(score_pairs(), key=lambda p: -p[0].size * p[1].size)
    want = np.array([nw_gotoh.score(a, b, scheme, go) for a, b in pairs], np.int32)
    s1, off1, s2, off2 = nwhip.batch_csr(pairs)
    ctx = nwhip.Context(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = [torch.from_numpy(x).cuda() for x in (s1, off1, s2, off2)]
        got = ctx.score_batch_affine(d[0], d[1], d[2], d[3], max(SCORE_N2), scheme, go, stream=stream)
        # a second launch on the same context and stream: its workspace is reused
        got2 = ctx.score_batch_affine(d[0], d[1], d[2], d[3], 200, scheme, go, stream=stream, waves=2)
        # and a linear one after it, on the scratch the affine launches left
        lin = ctx.score_batch(d[0], d[1], d[2], d[3], max(SCORE_N2), scheme, stream=stream)
    stream.synchronize()
    assert ctx.status(stream) == nwhip.NW_OK
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(got2.cpu().numpy(), want)
    np.testing.assert_array_equal(lin.cpu().numpy(), nwhip.score_batch(pairs, scheme))
    # max_n2 below a pair's rows: that pair is refused (INT32_MIN), the others computed
    with torch.cuda.stream(stream):
        low = ctx.score_batch_affine(d[0], d[1], d[2], d[3], 65, scheme, go, stream=stream)
    stream.synchronize()
    low = low.cpu().numpy()
    n2 = np.diff(off2)
    np.testing.assert_array_equal(low[n2 <= 65], want[n2 <= 65])
    assert (low[n2 > 65] == np.iinfo(np.int32).min).all()
    ctx.close()


# ------------------------------------------------------------------ CLI
@pytest.mark.parametrize("extra", [[], ["--score-only"]])
def test_cli_batch_gap_open(tmp_path, golden, extra):
    names = ["small", "debug", "t"]
    files = [(golden["pairs"][n]["argv1"], golden["pairs"][n]["argv2"]) for n in names]
    lst = tmp_path / "pairs.txt"
    lst.write_text("".join(f"{bdna_path(a)} {bdna_path(b)}\n" for a, b in files))
    exe = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")
    r = subprocess.run([exe, "--batch", str(lst), "--scheme", "1,-1,-1", "--gap-open", "-5"] + extra,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    int(lines[0])  # the wall time, ms
    want = [nw_gotoh.score(read_bdna(a), read_bdna(b), (1, -1, -1), -5) for a, b in files]
    assert lines[1:4] == [f"Score: {w}" for w in want]


def test_cli_gap_open_needs_batch():
    """No device work: --gap-open without --batch, and a positive one, are refused with a message."""
    exe = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")
    a, b = bdna_path("small1.bdna"), bdna_path("small2.bdna")
    r = subprocess.run([exe, a, b, "--gap-open", "-5"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--gap-open needs --batch" in r.stdout
    r = subprocess.run([exe, "--batch", "x", "--gap-open", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--gap-open expects" in r.stdout
