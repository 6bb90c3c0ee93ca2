"""GPU: batched pairwise alignment (nw_score_batch, nw_align_batch, nw_score_batch_async;
csrc/nw_batch.hip).

Checkers: oracle.score / oracle.fill (the serial fill restated in C) and the plain
Python walk of tests/nw_walk.py.  The shapes are the smallest at which each mechanism
can go wrong: one lane, a lane boundary (4 / 5 columns), a strip boundary (255 / 256 /
257 columns, three strips at 513), a row-block boundary (63 / 64 / 65 rows, three
blocks at 130), empty sides, a worker that takes a short pair after a long one (the
column scratch still holds the long pair's column), both substitution forms, chunks.
"""
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import nwhip
import oracle
from conftest import ROOT, bdna_path
from nw_walk import walk

pytestmark = pytest.mark.gpu

SCHEMES = [(1, 0, -1), (1, -1, -1), (2, -1, -2), (2, -1, 0)]
SCORE_N1 = [1, 3, 4, 5, 255, 256, 257, 513]
SCORE_N2 = [1, 63, 64, 65, 130]
OPS_N1 = [1, 4, 5, 256, 257, 600]
OPS_N2 = [1, 64, 65, 200]


def _rand(rng, n, alpha):
    return rng.integers(1, alpha + 1, n).astype(np.int8)


@functools.lru_cache(maxsize=None)
def score_pairs(alpha=4):
    """The score batch: the cross product of the sizes plus the empty sides, shuffled."""
    rng = np.random.default_rng(100 + alpha)
    sizes = list(itertools.product(SCORE_N1, SCORE_N2)) + [(0, 7), (7, 0), (0, 0)]
    pairs = [(_rand(rng, n1, alpha), _rand(rng, n2, alpha)) for n1, n2 in sizes]
    return tuple(pairs[i] for i in rng.permutation(len(pairs)))


@functools.lru_cache(maxsize=None)
def score_want(alpha, scheme):
    return np.array([oracle.score(a, b, scheme) for a, b in score_pairs(alpha)], np.int32)


@functools.lru_cache(maxsize=None)
def ops_pairs():
    rng = np.random.default_rng(7)
    return tuple((_rand(rng, n1, 4), _rand(rng, n2, 4)) for n1, n2 in itertools.product(OPS_N1, OPS_N2))


def check_alignments(pairs, scheme, scores, ops):
    for (a, b), sc, o in zip(pairs, scores, ops):
        t = oracle.fill(a, b, scheme)
        assert sc == t[-1, -1], (a.size, b.size)
        np.testing.assert_array_equal(o, walk(a, b, t, scheme), err_msg=f"{a.size} x {b.size} {scheme}")
        assert max(a.size, b.size) <= o.size <= a.size + b.size
        assert nwhip.ops_score(a, b, o, scheme) == sc


# ------------------------------------------------------------------ scores
@pytest.mark.parametrize("scheme", SCHEMES)
def test_scores_at_the_pairs_own_index(scheme):
    pairs = score_pairs()
    got, st = nwhip.score_batch(pairs, scheme, return_stats=True)
    np.testing.assert_array_equal(got, score_want(4, scheme))
    assert st.pairs == len(pairs) and st.cells == sum(a.size * b.size for a, b in pairs)
    assert st.chunks == 1 and 1 <= st.waves <= len(pairs) - 3 and st.fill_ms > 0


@pytest.mark.parametrize("scheme", SCHEMES)
def test_three_workers_take_the_whole_batch(scheme):
    """waves = 3: every worker sweeps a dozen pairs one after the other."""
    got, st = nwhip.score_batch(score_pairs(), scheme, waves=3, return_stats=True)
    np.testing.assert_array_equal(got, score_want(4, scheme))
    assert st.waves == 3


@pytest.mark.parametrize("scheme", SCHEMES)
def test_short_pair_after_a_long_one_on_the_same_worker(scheme):
    """One worker: 513 x 130 (three strips: the scratch holds its columns), then 5 x 130
    and 257 x 1, whose first strips must take the boundary and not the scratch."""
    rng = np.random.default_rng(11)
    pairs = [(_rand(rng, 257, 4), _rand(rng, 1, 4)), (_rand(rng, 513, 4), _rand(rng, 130, 4)),
             (_rand(rng, 5, 4), _rand(rng, 130, 4))]
    want = [oracle.score(a, b, scheme) for a, b in pairs]
    assert nwhip.score_batch(pairs, scheme, waves=1).tolist() == want
    sc, ops, st = nwhip.align_batch(pairs, scheme, waves=1)
    assert st.waves == 1
    check_alignments(pairs, scheme, sc, ops)


# ------------------------------------------------------------------ alphabet
@pytest.mark.parametrize("scheme", [(1, 0, -1), (2, -1, -2)])
def test_alphabets(scheme):
    # 9 letters: more than the v_perm tables cover, byte compares
    np.testing.assert_array_equal(nwhip.score_batch(score_pairs(9), scheme), score_want(9, scheme))
    # 4 letters with the tables switched off
    got = nwhip.score_batch(score_pairs(), scheme, flags=nwhip.FLAG_NO_PROFILE)
    np.testing.assert_array_equal(got, score_want(4, scheme))
    # a 3-letter s1 next to a 9-letter s1: the batch-wide decision falls to compares
    rng = np.random.default_rng(13)
    pairs = [(_rand(rng, 300, 3), _rand(rng, 200, 9)), (_rand(rng, 270, 9), _rand(rng, 131, 3)),
             (_rand(rng, 40, 3), _rand(rng, 70, 3))]
    assert len(set(np.concatenate([p[0] for p in pairs]).tolist())) == 9
    sc, ops, _ = nwhip.align_batch(pairs, scheme)
    check_alignments(pairs, scheme, sc, ops)
    assert nwhip.score_batch(pairs, scheme).tolist() == sc.tolist()


# ------------------------------------------------------------------ ops
@pytest.mark.parametrize("scheme", SCHEMES)
def test_ops_are_the_walks(scheme):
    pairs = ops_pairs()
    sc, ops, st = nwhip.align_batch(pairs, scheme)
    check_alignments(pairs, scheme, sc, ops)
    assert st.chunks == 1 and st.dir_bytes == sum(nwhip.batch_dir_bytes(a.size, b.size) for a, b in pairs)
    assert st.peak_bytes > st.dir_bytes and st.walk_ms > 0


def test_ops_equal_nw_align():
    rng = np.random.default_rng(17)
    a, b = _rand(rng, 1500, 4), _rand(rng, 1100, 4)
    al, want, _ = nwhip.align(a, b, (1, 0, -1))
    sc, ops, _ = nwhip.align_batch([(a, b)], (1, 0, -1))
    assert sc[0] == al.score == oracle.score(a, b, (1, 0, -1))
    np.testing.assert_array_equal(ops[0], want)


@pytest.mark.parametrize("scheme", [(2, -1, 0), (1, 0, -1)])
def test_boundary_runs(scheme):
    """Paths that reach row 0 or column 0 early, and very flat / very tall pairs; empty
    sides are all ups / all lefts."""
    rng = np.random.default_rng(19)
    ones, twos = (lambda n: np.full(n, 1, np.int8)), (lambda n: np.full(n, 2, np.int8))
    pairs = [(ones(300), twos(70)), (ones(70), twos(300)), (ones(5), twos(5)), (_rand(rng, 600, 4), _rand(rng, 3, 4)),
             (_rand(rng, 3, 4), _rand(rng, 600, 4)), (ones(0), twos(9)), (ones(9), twos(0)), (ones(0), twos(0))]
    sc, ops, _ = nwhip.align_batch(pairs, scheme)
    check_alignments(pairs[:5], scheme, sc[:5], ops[:5])
    g = scheme[2]
    assert sc[5:].tolist() == [9 * g, 9 * g, 0]
    assert ops[5].tolist() == [1] * 9 and ops[6].tolist() == [2] * 9 and ops[7].size == 0


# ------------------------------------------------------------------ chunks
def test_chunks_fit_the_budget():
    rng = np.random.default_rng(23)
    pairs = [(_rand(rng, int(rng.integers(280, 321)), 4), _rand(rng, int(rng.integers(280, 320)), 4))
             for _ in range(40)]
    scheme = (1, -1, -1)
    sc0, ops0, st0 = nwhip.align_batch(pairs, scheme)
    assert st0.chunks == 1
    want = [oracle.score(a, b, scheme) for a, b in pairs]
    assert sc0.tolist() == want
    # 14 pairs' worth of direction bytes for 40 pairs: three chunks at the least, whatever else is held
    mem = 14 * nwhip.batch_dir_bytes(300, 300)
    sc, ops, st = nwhip.align_batch(pairs, scheme, mem_bytes=mem)
    assert st.chunks >= 3 and st.peak_bytes <= mem and st.dir_bytes == st0.dir_bytes
    assert sc.tolist() == want
    for x, y in zip(ops, ops0):
        np.testing.assert_array_equal(x, y)
    for k in (0, 17, 39):
        np.testing.assert_array_equal(ops[k], walk(pairs[k][0], pairs[k][1], None, scheme))
    # below one pair's direction bytes: that pair is nw_align_ckpt's
    with pytest.raises(nwhip.NwError) as e:
        nwhip.align_batch(pairs, scheme, mem_bytes=nwhip.batch_dir_bytes(300, 300) - 1)
    assert e.value.status == nwhip.NW_ERR_OOM


# ------------------------------------------------------------------ device API
def test_context_score_batch_on_a_stream():
    import torch
    pairs = score_pairs()
    scheme = (2, -1, -2)
    s1, off1, s2, off2 = nwhip.batch_csr(pairs)
    ctx = nwhip.Context(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d = [torch.from_numpy(x).cuda() for x in (s1, off1, s2, off2)]
        got = ctx.score_batch(d[0], d[1], d[2], d[3], max(SCORE_N2), scheme, stream=stream)
        # a second launch on the same context and stream: its workspace is reused
        got2 = ctx.score_batch(d[0], d[1], d[2], d[3], 200, scheme, stream=stream, waves=2)
    stream.synchronize()
    assert ctx.status(stream) == nwhip.NW_OK
    np.testing.assert_array_equal(got.cpu().numpy(), score_want(4, scheme))
    np.testing.assert_array_equal(got2.cpu().numpy(), score_want(4, scheme))
    np.testing.assert_array_equal(nwhip.score_batch(pairs, scheme), score_want(4, scheme))
    # max_n2 below a pair's rows: that pair is refused (INT32_MIN), the others computed
    with torch.cuda.stream(stream):
        low = ctx.score_batch(d[0], d[1], d[2], d[3], 65, scheme, stream=stream)
    stream.synchronize()
    low = low.cpu().numpy()
    n2 = np.diff(off2)
    np.testing.assert_array_equal(low[n2 <= 65], score_want(4, scheme)[n2 <= 65])
    assert (low[n2 > 65] == np.iinfo(np.int32).min).all()
    ctx.close()


# ------------------------------------------------------------------ CLI
@pytest.mark.parametrize("extra,key", [([], "shipped"), (["--scheme", "1,-1,-1"], "mm1"),
                                       (["--score-only"], "shipped")])
def test_cli_batch(tmp_path, golden, extra, key):
    names = ["small", "debug", "t"]
    lst = tmp_path / "pairs.txt"
    lst.write_text("".join(f"{bdna_path(golden['pairs'][n]['argv1'])} {bdna_path(golden['pairs'][n]['argv2'])}\n"
                           for n in names))
    exe = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")
    r = subprocess.run([exe, "--batch", str(lst)] + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    int(lines[0])  # the wall time, ms
    assert lines[1:4] == [f"Score: {golden['pairs'][n]['scores'][key]}" for n in names]
