"""GPU: the batch walks over every unrolled cell's direction bits (nw_align_batch,
nw_align_batch_affine, nw_align_batch_matrix, nw_align_batch_local and the four score
entries; csrc/nw_batch.hip, nw_batch_affine.hip, nw_batch_matrix.hip, nw_batch_local.hip,
nw_batch_dev.h).

The pairs are the lists of tests/test_batch_paths_host.py, which proves from the checkers
alone that their paths read all 2 x 64 x 4 cell instances of a sweep's iteration in every
way a walk can read one (tests/nw_dirmap.py), in the EDGE and the plain variant, and the
local list also every instance as the walk's stop cell and as the hit's end cell.  Here the
device runs them: one test is one kernel variant and loops over its list in single batch
calls.  Every comparison is exact: ops byte for byte the checker's walk, scores and hits,
n_ops, and the library's own ops_score of the device ops.
"""
import functools

import numpy as np
import pytest

import nwhip
from test_batch_paths_host import LETTERS, MAT_INT8, MAT_LOCAL, MAT_WIDE, OPEN, SCHEME, cases, results, wide_form

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def submatrix(which):
    sc, index = {"int8": MAT_INT8, "wide": MAT_WIDE, "local": MAT_LOCAL}[which][:2]
    mat = nwhip.SubMatrix(LETTERS, sc)
    assert (mat.index[LETTERS] == index[LETTERS]).all() and (mat.scores == sc).all()
    return mat


def same_ops(name, got, want):
    assert len(got) == len(want)
    bad = [(k, a.size, b.size) for k, ((a, b), x, y) in enumerate(zip(cases(name), got, want))
           if x.size != y.ops.size or (x != y.ops).any()]
    assert not bad, f"{len(bad)} of {len(got)} pairs (index, n1, n2): {bad[:8]}"


def check_global(name, variant, align, score, ops_score):
    """The list through the directions kernel and its walk (the default grid, then one
    worker that sweeps every pair after the other with the scratch -- and the LDS profile --
    reused) and through the score kernel, a separate DIRS = false instantiation."""
    pairs, want = cases(name), results(name, variant)
    scores = np.array([r[0].score for r in want], np.int32)
    for waves in (0, 1):
        sc, ops, st = align(pairs, waves=waves)
        np.testing.assert_array_equal(sc, scores)
        same_ops(name, ops, [r[0] for r in want])       # (n_ops: the lengths)
        assert st.chunks == 1 and (waves == 0 or st.waves == 1)
        if waves == 0:
            assert [ops_score(a, b, o) for (a, b), o in zip(pairs, ops)] == scores.tolist()
        np.testing.assert_array_equal(score(pairs, waves=waves), scores)


# ------------------------------------------------------------------ linear
@pytest.mark.parametrize("flags", [0, nwhip.FLAG_NO_PROFILE], ids=["SUB_PERM", "SUB_GEN"])
def test_linear_walks(flags):
    """flags = 0 takes SUB_PERM on this list (test_the_lists_shapes: 5 distinct bytes in s1, table
    bytes in int8), NW_FLAG_NO_PROFILE the compares."""
    check_global("linear", "linear",
                 lambda p, waves: nwhip.align_batch(p, SCHEME, waves=waves, flags=flags),
                 lambda p, waves: nwhip.score_batch(p, SCHEME, waves=waves, flags=flags),
                 lambda a, b, o: nwhip.ops_score(a, b, o, SCHEME))


# ------------------------------------------------------------------ affine
@pytest.mark.parametrize("flags", [0, nwhip.FLAG_NO_PROFILE], ids=["SUB_PERM", "SUB_GEN"])
def test_affine_walks(flags):
    check_global("affine", "affine",
                 lambda p, waves: nwhip.align_batch_affine(p, SCHEME, OPEN, waves=waves, flags=flags),
                 lambda p, waves: nwhip.score_batch_affine(p, SCHEME, OPEN, waves=waves, flags=flags),
                 lambda a, b, o: nwhip.ops_score_affine(a, b, o, SCHEME, OPEN))


# ------------------------------------------------------------------ matrix
@pytest.mark.parametrize("variant", ["int8", "wide"])
def test_matrix_walks(variant):
    sc, _, ge, go = MAT_INT8 if variant == "int8" else MAT_WIDE
    assert wide_form(sc, ge) == (variant == "wide")
    mat = submatrix(variant)
    check_global("matrix", variant,
                 lambda p, waves: nwhip.align_batch_matrix(p, mat, ge, go, waves=waves),
                 lambda p, waves: nwhip.score_batch_matrix(p, mat, ge, go, waves=waves),
                 lambda a, b, o: nwhip.ops_score_matrix(a, b, o, mat, ge, go))


# ------------------------------------------------------------------ local
def hit_rows(hits, begin=True):
    cols = ["score", "end_i", "end_j"] + (["begin_i", "begin_j"] if begin else [])
    return np.stack([hits[c] for c in cols], axis=1)


@functools.lru_cache(maxsize=None)
def local_want():
    return np.array([(r[0].score,) + tuple(r[0].end) + tuple(r[0].begin) for r in results("local", "local")], np.int32)


@pytest.mark.parametrize("waves", [0, 1])
def test_local_walks(waves):
    pairs, want = cases("local"), results("local", "local")
    mat, (_, _, ge, go) = submatrix("local"), MAT_LOCAL
    hits, ops, st = nwhip.align_batch_local(pairs, mat, ge, go, waves=waves)
    np.testing.assert_array_equal(hit_rows(hits), local_want())
    same_ops("local", ops, [r[0] for r in want])
    assert (hits["reserved"] == 0).all() and st.chunks == 1 and (waves == 0 or st.waves == 1)
    if waves == 0:
        got = [nwhip.ops_score_matrix(a, b, o, mat, ge, go, begin=tuple(r[0].begin))
               for (a, b), o, r in zip(pairs, ops, want)]
        assert got == local_want()[:, 0].tolist()
    # the score kernel: the same end cells from its own `step` constants
    got = nwhip.score_batch_local(pairs, mat, ge, go, waves=waves)
    np.testing.assert_array_equal(hit_rows(got, begin=False), local_want()[:, :3])


def test_local_walks_in_chunks():
    pairs = cases("local")
    mat, (_, _, ge, go) = submatrix("local"), MAT_LOCAL
    h0, ops0, st0 = nwhip.align_batch_local(pairs, mat, ge, go)
    assert st0.chunks == 1
    # a third of the direction bytes: three chunks at the least, whatever else is held
    h, ops, st = nwhip.align_batch_local(pairs, mat, ge, go, mem_bytes=st0.dir_bytes // 3)
    assert st.chunks >= 3 and st.dir_bytes == st0.dir_bytes
    np.testing.assert_array_equal(h, h0)
    assert all(x.size == y.size and (x == y).all() for x, y in zip(ops, ops0))
    np.testing.assert_array_equal(hit_rows(h), local_want())
