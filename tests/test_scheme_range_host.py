"""CPU: the scheme list and the range edges of tests/test_scheme_range.py, and the
checkers on them, so that a failure on the device points at a kernel.

WIDE_SCHEMES leaves the box every other batch, affine, checkpoint and traceback test
draws from (|v| <= 2, negative gap, match > mismatch): the int8 edge of the v_perm table
bytes match - 2 gap and mismatch - 2 gap on both sides, positive and zero gap, match <=
mismatch, the largest values nw_params takes.

The range edges.  The bounds are restated here in Python (lin_sum, aff_sum) and never
taken from the library:
    linear   (M + |gap|) * (n1 + n2 + 2) < 2^28             M = max |match|, |mismatch|, |gap|
    affine   3 |go| + (M + |gap|) * (n1 + n2 + 2) < 2^28
    matrix   the affine one, M = max(largest |entry|, |gap|)
nw_params also takes only |match|, |mismatch|, |gap| < 2^12, and checks that first.  For
a pair of 513 x 130 the linear bound would bind at m = (2^28 - 1) // 645 // 2 = 208089,
fifty times beyond that limit; no pair below 32768 characters reaches it.  So the accepted
edge of a SCHEME is (4095, -4095, -4095) whatever the pair (test_scheme_edge_is_the_
parameter_limit pins that, and that the m of the range formula is refused), and a range
bound is met at its edge only through gap_open, which has no limit of its own: the edge
cases put gap_open there, next to -1 and next to 4095.
"""
import numpy as np
import pytest

import nw_gotoh
import nw_gotoh_matrix as gm
import nwhip
import oracle
from nw_walk import path_score, walk
from test_batch_host import VALID
from test_batch_matrix_host import identity_matrix, random_matrix

# (scheme, why it is here)
WIDE = [
    ((125, -1, -1), "msp = 127: tables, top byte"),
    ((126, -1, -1), "msp = 128: compares, one past"),
    ((1, -130, -1), "mmp = -128: tables, bottom byte"),
    ((1, -131, -1), "mmp = -129: compares"),
    ((2, -3, 1), "positive gap"),
    ((7, -5, 3), "positive gap"),
    ((1, 1, -1), "match = mismatch"),
    ((-5, -200, 3), "match < 0, positive gap, compares"),
    ((5, 0, 0), "gap 0"),
    ((4095, -4095, -4095), "large values"),
    # Under a positive gap with match <= 2 gap, and under (-5, -200, 3), the all-gaps path wins
    # every cell: w is 0 throughout and only the tie order is tested.  (7, -5, 3) is the one
    # entry above with a positive gap and a table worth the name; two more of that kind:
    ((9, -4, 2), "positive gap, match > 2 gap: diagonals and gaps both win cells"),
    ((-1, -3, -2), "match < 0 under a negative gap: diagonals still win cells"),
]
WIDE_SCHEMES = [s for s, _ in WIDE]

LIMIT = 2 ** 28
CAP = 4095  # nw_params: |match|, |mismatch|, |gap| < 2^12
BIG, MID = (513, 130), (257, 65)  # three strips and three row blocks; two and two
TINY = [(1, 1), (1, 3), (3, 1), (4, 4), (5, 5), (4, 5)]
CAP_SCHEME = (CAP, -CAP, -CAP)


def table_form(scheme):
    """Both table bytes fit int8: the kernels may take the v_perm tables."""
    m, mm, g = scheme
    return -128 <= m - 2 * g <= 127 and -128 <= mm - 2 * g <= 127


def lin_sum(scheme, n1, n2):
    m = max(abs(v) for v in scheme)
    return (m + abs(scheme[2])) * (n1 + n2 + 2)


def aff_sum(scheme, go, n1, n2, mat_abs=None):
    """mat_abs: the matrix form, the largest |entry| in the place of match / mismatch."""
    m = max(abs(v) for v in scheme) if mat_abs is None else max(mat_abs, abs(scheme[2]))
    return 3 * abs(go) + (m + abs(scheme[2])) * (n1 + n2 + 2)


def go_edge(scheme, n1, n2, mat_abs=None):
    """The most negative gap_open the affine (or matrix) bound takes for an n1 x n2 pair."""
    go = -((LIMIT - 1 - aff_sum(scheme, 0, n1, n2, mat_abs)) // 3)
    assert aff_sum(scheme, go, n1, n2, mat_abs) < LIMIT <= aff_sum(scheme, go - 1, n1, n2, mat_abs)
    return go


def edge_matrix():
    """tests/test_batch_matrix.py matrix(20): entries -8..12."""
    m = random_matrix(np.random.default_rng(520), 20)
    assert int(np.abs(m.scores).max()) == 12
    return m


# The affine and matrix edge cases: (name, scheme or gap_extend, gap_open, largest pair)
AFFINE_EDGES = {
    "go_at_the_edge": ((1, -1, -1), go_edge((1, -1, -1), *BIG), BIG),
    "go_at_the_edge_tiny": ((1, -1, -1), go_edge((1, -1, -1), 5, 5), (5, 5)),
    "go_at_the_edge_seam": ((1, -1, -1), go_edge((1, -1, -1), 600, 300), (600, 300)),
    "scheme_at_its_limit": (CAP_SCHEME, go_edge(CAP_SCHEME, *BIG), BIG),
}
MATRIX_EDGES = {
    "ge_at_its_limit": (-CAP, go_edge((0, 0, -CAP), *BIG, mat_abs=12), BIG),
    "go_at_the_edge": (-1, go_edge((0, 0, -1), *BIG, mat_abs=12), BIG),
}


def rand_pair(seed, n1, n2, alpha=4):
    rng = np.random.default_rng(seed)
    return rng.integers(1, alpha + 1, n1).astype(np.int8), rng.integers(1, alpha + 1, n2).astype(np.int8)


def status_of(f, *a, **kw):
    try:
        f(*a, **kw)
    except nwhip.NwError as e:
        return e.status
    return nwhip.NW_OK


# ------------------------------------------------------------------ the list itself
def test_the_list_sits_where_it_says():
    b = {s: (s[0] - 2 * s[2], s[1] - 2 * s[2]) for s in WIDE_SCHEMES}
    assert b[(125, -1, -1)] == (127, 1) and table_form((125, -1, -1))
    assert b[(126, -1, -1)] == (128, 1) and not table_form((126, -1, -1))
    assert b[(1, -130, -1)] == (3, -128) and table_form((1, -130, -1))
    assert b[(1, -131, -1)] == (3, -129) and not table_form((1, -131, -1))
    assert not table_form((-5, -200, 3)) and not table_form(CAP_SCHEME)
    assert [s for s in WIDE_SCHEMES if table_form(s)] == [(125, -1, -1), (1, -130, -1), (2, -3, 1), (7, -5, 3),
                                                          (1, 1, -1), (5, 0, 0), (9, -4, 2), (-1, -3, -2)]
    assert sum(s[2] > 0 for s in WIDE_SCHEMES) == 4 and sum(s[0] <= s[1] for s in WIDE_SCHEMES) == 1
    assert sum(s[0] < 0 for s in WIDE_SCHEMES) == 2
    assert len(set(WIDE_SCHEMES)) == len(WIDE) == 12
    assert all(max(abs(v) for v in s) <= CAP for s in WIDE_SCHEMES)


# ------------------------------------------------------------------ the checkers on these inputs
ALL_SCHEMES = WIDE_SCHEMES + [(1, -1, -1)]


@pytest.mark.parametrize("scheme", ALL_SCHEMES)
def test_gotoh_with_gap_open_0_is_the_oracle(scheme):
    for n1, n2 in [(70, 40), (5, 5)]:
        a, b = rand_pair(n1 + n2, n1, n2)
        assert nw_gotoh.score(a, b, scheme, 0) == oracle.score(a, b, scheme)
        np.testing.assert_array_equal(nw_gotoh.fill(a, b, scheme, 0)[0], oracle.fill(a, b, scheme))


@pytest.mark.parametrize("scheme", ALL_SCHEMES)
def test_walk_rescores_to_the_corner(scheme):
    for n1, n2 in [(70, 40), (5, 5), (40, 70)]:
        a, b = rand_pair(n1 + 3 * n2, n1, n2)
        t = oracle.fill(a, b, scheme)
        ops = walk(a, b, t, scheme)
        assert path_score(a, b, ops, scheme) == t[-1, -1] == nwhip.ops_score(a, b, ops, scheme)
        for go in (-1, -11, -1000003):
            tables = nw_gotoh.fill(a, b, scheme, go)
            ops = nw_gotoh.walk(a, b, scheme, go, tables)
            assert nw_gotoh.path_score_affine(a, b, ops, scheme, go) == tables[0][-1, -1]
            assert nwhip.ops_score_affine(a, b, ops, scheme, go) == tables[0][-1, -1]


@pytest.mark.parametrize("case", sorted(AFFINE_EDGES))
def test_gotoh_at_the_edges_stays_exact(case):
    """The fill a row at a time against the cell recurrence with Python integers, with
    gap_open near -2^28 / 3."""
    scheme, go, _ = AFFINE_EDGES[case]
    for n1, n2 in [(70, 40), (5, 5)]:
        a, b = rand_pair(n1 * n2, n1, n2)
        for x, y in zip(nw_gotoh.fill(a, b, scheme, go), nw_gotoh.fill_cells(a, b, scheme, go)):
            fin = y > nw_gotoh.NEG // 2
            np.testing.assert_array_equal(x[fin], y[fin])
        ops = nw_gotoh.walk(a, b, scheme, go)
        assert nw_gotoh.path_score_affine(a, b, ops, scheme, go) == nw_gotoh.score(a, b, scheme, go)


@pytest.mark.parametrize("scheme", [s for s in ALL_SCHEMES if -128 <= s[0] <= 127 and -128 <= s[1] <= 127])
def test_identity_matrix_checker_is_gotoh(scheme):
    mat = identity_matrix([1, 2, 3, 4], scheme[0], scheme[1])
    for (n1, n2), go in [((70, 40), -11), ((5, 5), -1000003), ((40, 70), go_edge((1, -1, -1), *BIG))]:
        a, b = rand_pair(n1 + 5 * n2, n1, n2)
        assert gm.score(a, b, mat.scores, mat.index, scheme[2], go) == nw_gotoh.score(a, b, scheme, go)
        np.testing.assert_array_equal(gm.walk(a, b, mat.scores, mat.index, scheme[2], go),
                                      nw_gotoh.walk(a, b, scheme, go))


@pytest.mark.parametrize("case", sorted(MATRIX_EDGES))
def test_matrix_checker_at_the_edges_stays_exact(case):
    ge, go, _ = MATRIX_EDGES[case]
    mat = edge_matrix()
    for n1, n2 in [(70, 40), (5, 5)]:
        a, b = rand_pair(n1 * n2 + 1, n1, n2, 20)
        tables = gm.fill(a, b, mat.scores, mat.index, ge, go)
        for x, y in zip(tables, gm.fill_cells(a, b, mat.scores, mat.index, ge, go)):
            fin = y > gm.MINF // 2
            np.testing.assert_array_equal(x[fin], y[fin])
        ops = gm.walk(a, b, mat.scores, mat.index, ge, go, tables)
        assert gm.path_score(a, b, ops, mat.scores, mat.index, ge, go) == tables[0][-1, -1]


# ------------------------------------------------------------------ the edges are edges
def _edge_pairs(shape):
    return [rand_pair(1, *shape), rand_pair(2, *MID)] if shape == BIG else [rand_pair(1, *shape)]


def test_scheme_edge_is_the_parameter_limit():
    """Every entry with a scheme takes (4095, -4095, -4095) and refuses 4096 in any place; the
    linear bound at that scheme is 50 times away for 513 x 130, and the m at which it would
    bind is refused with every pair, also a 5 x 5 one."""
    pairs = _edge_pairs(BIG)
    a, b = pairs[0]
    assert lin_sum(CAP_SCHEME, *BIG) * 50 < LIMIT
    calls = [lambda s: nwhip.score_batch(pairs, s), lambda s: nwhip.align_batch(pairs, s),
             lambda s: nwhip.score_batch_affine(pairs, s, -11), lambda s: nwhip.align_batch_affine(pairs, s, -11),
             lambda s: nwhip.score_sweep(a, b, s), lambda s: nwhip.align_ckpt(a, b, s, block_rows=64),
             lambda s: nwhip.align(a, b, s)]
    for f in calls:
        assert status_of(f, CAP_SCHEME) in VALID
        assert status_of(f, (-CAP, CAP, CAP)) in VALID
        for k in range(3):
            for v in (CAP + 1, -CAP - 1):
                s = list(CAP_SCHEME)
                s[k] = v
                assert status_of(f, tuple(s)) == nwhip.NW_ERR_ARG
    mat = edge_matrix()
    for f in (nwhip.score_batch_matrix, nwhip.align_batch_matrix):
        p20 = [rand_pair(3, *BIG, 20)]
        assert status_of(f, p20, mat, -CAP, -11) in VALID
        assert status_of(f, p20, mat, CAP, -11) in VALID
        assert status_of(f, p20, mat, -CAP - 1, -11) == status_of(f, p20, mat, CAP + 1, -11) == nwhip.NW_ERR_ARG
    # the range formula's own m: beyond the limit, so refused although the bound holds
    for (n1, n2), plist in [(BIG, pairs), ((5, 5), [rand_pair(4, 5, 5)])]:
        m = (LIMIT - 1) // (n1 + n2 + 2) // 2
        assert lin_sum((m, -m, -m), n1, n2) < LIMIT <= lin_sum((m + 1, -m - 1, -m - 1), n1, n2) and m > CAP
        assert status_of(nwhip.score_batch, plist, (m, -m, -m)) == nwhip.NW_ERR_ARG
        assert status_of(nwhip.align_batch, plist, (m, -m, -m)) == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("case", sorted(AFFINE_EDGES))
def test_affine_edges_are_edges(case):
    scheme, go, shape = AFFINE_EDGES[case]
    assert aff_sum(scheme, go, *shape) < LIMIT <= aff_sum(scheme, go - 1, *shape)
    pairs = _edge_pairs(shape)
    for f in (nwhip.score_batch_affine, nwhip.align_batch_affine):
        assert status_of(f, pairs, scheme, go) in VALID
        assert status_of(f, pairs, scheme, go - 1) == nwhip.NW_ERR_ARG
        # two more characters in the largest pair tip it too (the floor of / 3 may leave room for one)
        longer = [rand_pair(5, shape[0] + 2, shape[1])] + pairs[1:]
        assert status_of(f, longer, scheme, go) == nwhip.NW_ERR_ARG
    if case == "go_at_the_edge":
        assert go == -89478055


@pytest.mark.parametrize("case", sorted(MATRIX_EDGES))
def test_matrix_edges_are_edges(case):
    ge, go, shape = MATRIX_EDGES[case]
    mat = edge_matrix()
    assert aff_sum((0, 0, ge), go, *shape, mat_abs=12) < LIMIT <= aff_sum((0, 0, ge), go - 1, *shape, mat_abs=12)
    if case == "ge_at_its_limit":
        # every table byte s - 2 ge is far outside int8: the kernel adds -2 ge itself
        assert (mat.scores - 2 * ge).min() > 127
    pairs = [rand_pair(1, *shape, 20), rand_pair(2, *MID, 20)]
    for f in (nwhip.score_batch_matrix, nwhip.align_batch_matrix):
        assert status_of(f, pairs, mat, ge, go) in VALID
        assert status_of(f, pairs, mat, ge, go - 1) == nwhip.NW_ERR_ARG
        longer = [rand_pair(5, shape[0], shape[1] + 2, 20)] + pairs[1:]
        assert status_of(f, longer, mat, ge, go) == nwhip.NW_ERR_ARG
