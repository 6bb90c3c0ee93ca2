"""CPU: the matrices, gap costs and pairs of tests/test_local_range.py, and the checker
of tests/nw_local.py on them, so that a failure on the device points at a kernel.

Every other device test of the batched local alignment draws (ge, go) from (-1, -11),
(-3, 0), (-2, -3), (-2, -11) or a linear +-1 / +-2 scheme, matrix entries from -8..11 (or
5 / -4, 100 / -100), and a matrix of negative expected score.  Here:
  * EDGE20 (127 and -128 in every byte position of a lane's profile dword), POS20 (no
    entry below 1: H is never floored, every path ends on row 0 / column 0), ZERO4
    (diagonal steps of 0: direction code 3 against code 0) and NONPOS4 (nothing aligns);
  * ge = 0 (F + ge == ho; with go = 0 every E and F ties with an H), ge = -4095, and
    gap_open at the last value the range bound takes for the batch's longest pair,
        3 |go| + (max(M, |ge|) + |ge|) * (n1 + n2 + 2) < 2^28
    (test_scheme_range_host.go_edge: the bound restated, never taken from the library);
  * periodic pairs with 98 to 258 equal maxima: two in the columns of one lane on one
    row, over all strips, down one column over four row blocks;
  * 200 pairs for the one-thread-per-ticket walk and for chunks of more than 64 pairs.
Each condition that makes a case mean something is a function here, judged from the
checker alone; the GPU module asserts the same functions before it compares anything.
"""
import functools

import numpy as np
import pytest

import nw_local as nl
import nwhip
import test_batch_local as tbl
from nw_gotoh_matrix import sub_table
from test_batch import _rand
from test_batch_host import VALID
from test_batch_local_host import SHAPES
from test_scheme_range_host import CAP, LIMIT, TINY, aff_sum, go_edge, rand_pair, status_of

LETTERS20, LETTERS4 = list(range(1, 21)), [1, 2, 3, 4]


# ------------------------------------------------------------------ matrices
@functools.lru_cache(maxsize=None)
def matrix(name):
    """Seeded and asymmetric over the bytes 1..alpha."""
    if name == "EDGE20":  # 105..127 on the diagonal, -128..-90 off it
        rng = np.random.default_rng(1200)
        sc = rng.integers(-128, -89, (20, 20))
        sc[np.arange(20), np.arange(20)] = rng.integers(105, 128, 20)
        sc[3, 3], sc[7, 7], sc[11, 11] = 127, 127, 127
        sc[2, 9], sc[9, 2], sc[15, 4] = -128, -128, -128
        sc[4, 15] = -90
        assert sc.mean() < -50
        m = nwhip.SubMatrix(LETTERS20, sc)
    elif name == "POS20":
        rng = np.random.default_rng(1201)
        sc = rng.integers(1, 128, (20, 20))
        sc[0, 5], sc[5, 0], sc[6, 6] = 127, 1, 127
        m = nwhip.SubMatrix(LETTERS20, sc)
    elif name == "ZERO4":  # 4 or 0 on the diagonal, -3 or 0 off it
        sc = np.array([[4, -3, 0, -3], [-3, 4, -3, -3], [-3, 0, 0, -3], [0, -3, -3, 4]])
        m = nwhip.SubMatrix(LETTERS4, sc)
    elif name == "NONPOS4":
        rng = np.random.default_rng(1203)
        sc = rng.integers(-8, 0, (4, 4))
        sc[0, 0], sc[2, 2], sc[1, 3] = 0, 0, 0
        m = nwhip.SubMatrix(LETTERS4, sc)
    elif name == "UNI4":  # the hand-made cases: 5 / -4
        return nwhip.SubMatrix.uniform(LETTERS4, *tbl.UNI)
    else:
        raise KeyError(name)
    assert (m.scores != m.scores.T).any()
    return m


MATRICES = ["EDGE20", "POS20", "ZERO4", "NONPOS4"]


def mat_abs(name):
    return int(np.abs(matrix(name).scores).max())


# ------------------------------------------------------------------ costs
def longest(pairs):
    """(n1, n2) of the pair with the largest n1 + n2: the one the range bound binds on."""
    return max(((a.size, b.size) for a, b in pairs), key=lambda s: s[0] + s[1])


def edge_open(name, ge, shape):
    """The last gap_open matrix_range_ok takes for a pair of `shape` under matrix `name`."""
    return go_edge((0, 0, ge), *shape, mat_abs=mat_abs(name))


def costs(name, pairs):
    """The six (ge, go) of a batch: the two edges are that batch's own."""
    shape = longest(pairs)
    return [(0, 0), (0, -7), (-CAP, 0), (-CAP, -11), (-1, edge_open(name, -1, shape)),
            (-CAP, edge_open(name, -CAP, shape))]


N_COSTS = 6
EDGE_COSTS = (4, 5)  # their places in costs()


# ------------------------------------------------------------------ pairs
@functools.lru_cache(maxsize=None)
def equal_pair():
    """Two equal sequences of 300 letters: under EDGE20 the diagonal alone is worth more
    than 2^15."""
    a = _rand(np.random.default_rng(1210), 300, 20)
    return a, a.copy()


@functools.lru_cache(maxsize=None)
def score_batch():
    return tbl.score_pairs(20) + (equal_pair(),)


@functools.lru_cache(maxsize=None)
def ops_batch():
    """tests/test_batch_local.py ops_pairs() without its 1500 x 1100 pair, and the equal pair."""
    return tuple(p for p in tbl.ops_pairs() if p[0].size != 1500) + (equal_pair(),)


@functools.lru_cache(maxsize=None)
def tiny_pairs():
    """1 x 1 .. 5 x 5, a 5 x 5 pair last, over 20 letters (tests/test_scheme_range.py's)."""
    return tuple(rand_pair(10 + k, n1, n2, 20) for k, (n1, n2) in enumerate(TINY + [(5, 5)]))


ZERO_SHAPES = [(257, 65), (513, 130), (5, 63)]
ZERO_COSTS = [(-1, -11), (0, 0), (-3, 0)]


@functools.lru_cache(maxsize=None)
def zero_pairs():
    """Planted 4-letter pairs: a segment of s1 stands in s2 with substitutions and indels."""
    rng = np.random.default_rng(1211)
    return (tbl.planted(rng, 257, 65, 4, 180, 50, 8, [("d", 2), ("i", 1)], 0.1),
            tbl.planted(rng, 513, 130, 4, 230, 100, 15, [("i", 3), ("d", 4), ("d", 1)], 0.1),
            tbl.planted(rng, 5, 63, 4, 0, 5, 30, (), 0.0))


def _periodic(n, first):
    """first, 3 - first, first, .. of n letters (the letters 1 and 2)."""
    s = np.full(n, first, np.int8)
    s[1::2] = 3 - first
    return s


# name -> (n1, n2, the first letter of s1 and of s2, how the maxima lie)
PERIODIC = {
    "row": (520, 6, (1, 1), "row"), "row_offset": (520, 6, (2, 1), "row"),
    "column": (6, 200, (1, 1), "column"), "column_offset": (6, 200, (1, 2), "column"),
    "both": (520, 200, (1, 1), "row"), "both_offset": (520, 200, (2, 1), "row"),
}
PERIODIC_COST = (-1, -11)


@functools.lru_cache(maxsize=None)
def periodic_pairs():
    return tuple((_periodic(n1, f1), _periodic(n2, f2)) for n1, n2, (f1, f2), _ in PERIODIC.values())


def lane_of(j):
    """(strip, lane, byte) of column j >= 1: 256 columns a strip, four a lane."""
    return (j - 1) // 256, ((j - 1) % 256) // 4, (j - 1) % 4


def periodic_facts(name):
    """The maxima of a periodic pair from the checker's H: (maxima as (i, j) in row-major
    order, the score).  Asserts what the case is there for."""
    n1, n2, _, kind = PERIODIC[name]
    a, b = periodic_pairs()[list(PERIODIC).index(name)]
    m = matrix("UNI4")
    H = nl.fill(a, b, m.scores, m.index, *PERIODIC_COST)[0]
    top = [(int(i), int(j)) for i, j in np.argwhere(H == H.max())]
    assert H.max() == 5 * min(n1, n2) and len(top) >= 50
    assert nl.best(H) == (int(H.max()), *top[0])
    offset = name.endswith("offset")
    if kind == "row":
        # all on the last row, every second column, in every strip; two of them in the four
        # columns of one lane
        assert all(i == n2 for i, _ in top) and top[0] == (n2, n2 + offset)
        assert [j for _, j in top] == list(range(n2 + offset, n1 + 1, 2))
        assert len({lane_of(j)[0] for _, j in top}) == 3 == (n1 + 255) // 256
        lanes = [lane_of(j)[:2] for _, j in top]
        assert len(set(lanes)) < len(lanes)
        assert {lane_of(j)[2] for _, j in top} == ({1, 3} if (n2 + offset) % 2 == 0 else {0, 2})
    else:
        # all in the last column, every second row, over four row blocks
        assert all(j == n1 for _, j in top) and top[0] == (n1 + offset, n1)
        assert [i for i, _ in top] == list(range(n1 + offset, n2 + 1, 2))
        assert len({i // 64 for i, _ in top}) == 4
    return top, int(H.max())


@functools.lru_cache(maxsize=None)
def crowd():
    """200 pairs over 4 letters, shuffled: 190 with both sides drawn from 0..12 and ten of about
    300 x 70 (the recipe of tests/test_scheme_range.py crowd, a seed of its own)."""
    rng = np.random.default_rng(1287)
    sizes = [(int(rng.integers(0, 13)), int(rng.integers(0, 13))) for _ in range(190)]
    sizes += [(int(rng.integers(280, 321)), int(rng.integers(60, 81))) for _ in range(10)]
    pairs = [(_rand(rng, n1, 4), _rand(rng, n2, 4)) for n1, n2 in sizes]
    return tuple(pairs[i] for i in rng.permutation(len(pairs)))


CROWD_COST = (-1, -3)


def tickets(pairs):
    """The indices of the pairs with cells, longest first (the library's stable order)."""
    live = [k for k, (a, b) in enumerate(pairs) if a.size and b.size]
    return sorted(live, key=lambda k: -pairs[k][0].size * pairs[k][1].size)


# ------------------------------------------------------------------ the checker's results, once
def _mat_of(mat):
    return matrix(mat) if isinstance(mat, str) else mat


def want_alignments(pairs, mat, ge, go):
    """Per pair ((score, end_i, end_j), begin, ops, tables) from the checker."""
    m = _mat_of(mat)
    out = []
    for a, b in pairs:
        tables = nl.fill(a, b, m.scores, m.index, ge, go)
        ops, begin = nl.walk(a, b, m.scores, m.index, ge, go, tables)
        out.append((nl.best(tables[0]), begin, ops, tables))
    return out


@functools.lru_cache(maxsize=None)
def want_hits(batch, name, ge, go):
    pairs = {"score": score_batch, "ops": ops_batch, "tiny": tiny_pairs, "zero": zero_pairs}[batch]()
    m = matrix(name)
    return np.array([tbl.want_hit(a, b, m.scores, m.index, ge, go) for a, b in pairs], np.int32)


def path_cells(begin, ops):
    """The cell each op arrives at, walking from `begin`."""
    i, j = begin
    out = []
    for op in ops.tolist():
        i += op != 2
        j += op != 1
        out.append((i, j))
    return out


def open_ties(want, ge, go):
    """(lefts, ups) on the walked paths at which opening ties with extending: E == H_left + go
    + ge == E_left + ge (F likewise) -- "opening wins" decides the state after that op."""
    lefts = ups = 0
    for _, begin, ops, (H, E, F) in want:
        for op, (i, j) in zip(ops.tolist(), path_cells(begin, ops)):
            if op == 2 and E[i, j - 1] + ge == H[i, j - 1] + go + ge:
                lefts += 1
            if op == 1 and F[i - 1, j] + ge == H[i - 1, j] + go + ge:
                ups += 1
    return lefts, ups


def zero_diagonal_stops(pairs, mat, want):
    """Paths whose begin cell, an inner one, has H = 0 by a diagonal step (H_diag + s == 0): a
    walk that tested the diagonal before the stop would go on from there."""
    m = _mat_of(mat)
    n = 0
    for (a, b), (_, (i, j), ops, (H, _, _)) in zip(pairs, want):
        if ops.size and i > 0 and j > 0:
            assert H[i, j] == 0
            n += H[i - 1, j - 1] + sub_table(a, b, m.scores, m.index)[i - 1, j - 1] == 0
    return int(n)


def gap_ops(want):
    return sum(int((ops != 0).sum()) for _, _, ops, _ in want)


def idle_lanes_outscore(pairs, mat, ge, go):
    """The pairs for which the table over s1 continued with its last letter by n2 columns (what
    the lanes past n1 compute) holds a value above the pair's own best."""
    m = _mat_of(mat)
    n = 0
    for a, b in pairs:
        wide = np.concatenate([a, np.full(b.size, a[-1], np.int8)])
        own = nl.fill(a, b, m.scores, m.index, ge, go)[0].max()
        n += nl.fill(wide, b, m.scores, m.index, ge, go)[0][:, a.size + 1:].max() > own
    return int(n)


# ------------------------------------------------------------------ the matrices are what they say
def test_the_matrices_sit_where_they_say():
    e, p, z, n = (matrix(k).scores for k in MATRICES)
    off = ~np.eye(20, dtype=bool)
    assert e.max() == 127 and e.min() == -128 and e[off].max() <= -90 and e.diagonal().min() >= 105 and e.mean() < 0
    assert p.min() == 1 and p.max() == 127
    off4 = ~np.eye(4, dtype=bool)
    assert set(z.ravel().tolist()) == {-3, 0, 4} and (z.diagonal() == 0).any() and (z[off4] == 0).any()
    assert z.mean() < 0 and (z.diagonal() == 4).sum() == 3
    assert n.max() == 0 and n.min() >= -8 and (n.diagonal() == 0).any() and (n[off4] == 0).any() and (n < 0).sum() >= 12
    assert [mat_abs(k) for k in MATRICES] == [128, 127, 4, 8]


@pytest.mark.parametrize("batch", ["score", "ops"])
def test_both_int8_ends_in_every_byte_of_a_lane(batch):
    """build_profile packs the scores of a lane's columns 4l .. 4l + 3 against one row letter
    into one dword, column k in byte k.  From the letters of the columns and rows: 127 and
    -128 stand in each of the four positions on some pair of the batch."""
    m = matrix("EDGE20")
    pairs = score_batch() if batch == "score" else ops_batch()
    seen = {(v, k): 0 for v in (127, -128) for k in range(4)}
    for a, b in pairs:
        if a.size and b.size:
            sub = sub_table(a, b, m.scores, m.index)
            for v, k in seen:
                seen[v, k] += int((sub[:, k::4] == v).sum())
    assert min(seen.values()) >= 20, seen


def test_the_equal_pair_scores_above_int16():
    a, b = equal_pair()
    m = matrix("EDGE20")
    assert tbl.want_hit(a, b, m.scores, m.index, -1, -11)[0] > 32767 + 500
    assert tbl.want_hit(a, b, m.scores, m.index, -1, -11)[1:] == (300, 300)


# ------------------------------------------------------------------ the edges are edges
class _Calls:
    def __init__(self, pairs, name):
        self.pairs, self.mat = list(pairs), matrix(name)

    def both(self, ge, go):
        return (status_of(nwhip.score_batch_local, self.pairs, self.mat, ge, go),
                status_of(nwhip.align_batch_local, self.pairs, self.mat, ge, go))


@pytest.mark.parametrize("batch", ["score", "ops", "tiny"])
@pytest.mark.parametrize("name", ["EDGE20", "POS20"])
def test_gap_open_edges_are_edges(name, batch):
    """go_edge is accepted and go_edge - 1 refused, by the library's own status, for both
    entries; the shapes of a batch stand in for it (the refusal comes before any cell)."""
    pairs = {"score": score_batch, "ops": ops_batch, "tiny": tiny_pairs}[batch]()
    shape = longest(pairs)
    assert shape == {"score": (513, 130), "ops": (520, 200), "tiny": (5, 5)}[batch]
    # letters do not matter to a refusal: one pair of the longest shape and a small one
    c = _Calls([rand_pair(1, *shape, 20), rand_pair(2, 5, 3, 20)], name)
    for ge in (-1, -CAP):
        go = edge_open(name, ge, shape)
        m = max(mat_abs(name), -ge)
        assert 3 * -go + (m - ge) * (sum(shape) + 2) < LIMIT <= 3 * (1 - go) + (m - ge) * (sum(shape) + 2)
        assert aff_sum((0, 0, ge), go, *shape, mat_abs=mat_abs(name)) < LIMIT
        st = c.both(ge, go)
        assert st[0] in VALID and st[1] in VALID
        assert c.both(ge, go - 1) == (nwhip.NW_ERR_ARG, nwhip.NW_ERR_ARG)
    assert -90_000_000 < edge_open(name, -1, shape) < edge_open(name, -CAP, shape) < -86_000_000
    for go in (0, -11):
        assert c.both(-CAP - 1, go) == (nwhip.NW_ERR_ARG, nwhip.NW_ERR_ARG)  # ge = -4096
        st = c.both(-CAP, go)
        assert st[0] in VALID and st[1] in VALID


def test_costs_lists():
    for name, pairs in [("EDGE20", score_batch()), ("POS20", ops_batch()), ("EDGE20", tiny_pairs())]:
        cs = costs(name, pairs)
        assert len(cs) == N_COSTS and cs[:4] == [(0, 0), (0, -7), (-4095, 0), (-4095, -11)]
        assert [cs[k][0] for k in EDGE_COSTS] == [-1, -4095] and all(cs[k][1] < -86_000_000 for k in EDGE_COSTS)


# ------------------------------------------------------------------ the checker on these inputs
@pytest.mark.parametrize("name", MATRICES)
def test_checker_row_fill_equals_the_literal_fill(name):
    """nl.fill against nl.fill_cells (Python integers, cell by cell) for every matrix x cost
    of the device module, shapes up to 64 x 70."""
    m = matrix(name)
    alpha = m.n
    rng = np.random.default_rng(1220 + alpha)
    positive = 0
    for n1, n2 in SHAPES:
        a, b = _rand(rng, n1, alpha), _rand(rng, n2, alpha)
        if n1 >= 17:
            b[2:2 + min(n1, n2) // 2] = a[1:1 + min(n1, n2) // 2]  # something to align
        for ge, go in costs(name, [(a, b)]) + ZERO_COSTS:
            got = nl.fill(a, b, m.scores, m.index, ge, go)
            want = nl.fill_cells(a, b, m.scores, m.index, ge, go)
            for x, y in zip(got, want):
                fin = y > nl.MINF // 2
                np.testing.assert_array_equal(x[fin], y[fin], err_msg=f"{name} {n1} x {n2} ge {ge} go {go}")
                assert (x[~fin] < nl.MINF // 2).all()
            positive += got[0].max() > 0
            ops, begin = nl.walk(a, b, m.scores, m.index, ge, go, want)
            sc, ei, ej = nl.best(want[0])
            assert nl.path_score(a, b, ops, begin, m.scores, m.index, ge, go) == (sc, (ei, ej))
            assert nwhip.ops_score_matrix(a, b, ops, m, ge, go, begin=begin) == sc
    # (the three shapes with a shared segment at the least)
    assert positive == 0 if name == "NONPOS4" else positive >= 3 * (N_COSTS + len(ZERO_COSTS))


def test_zero_matrix_stops_before_a_diagonal_of_zero():
    """ZERO4: on the device module's own pairs some path begins at an inner cell whose H = 0
    came by a diagonal step (H_diag + s == 0): the walk stops there only because the stop is
    tested first.  NONPOS4 on the same pairs: zero-scoring diagonals, and nothing aligned."""
    pairs = zero_pairs()
    assert [(a.size, b.size) for a, b in pairs] == ZERO_SHAPES
    for ge, go in ZERO_COSTS:
        want = want_alignments(pairs, "ZERO4", ge, go)
        # (with free gaps every path runs back to row 0 / column 0)
        assert zero_diagonal_stops(pairs, "ZERO4", want) >= (ge < 0), (ge, go)
        assert all(hit[0] > 0 for hit, _, _, _ in want)
        for (a, b), (hit, begin, ops, _) in zip(pairs, want_alignments(pairs, "NONPOS4", ge, go)):
            n = matrix("NONPOS4")
            assert (sub_table(a, b, n.scores, n.index) == 0).sum() >= 5
            assert hit == (0, 0, 0) and begin == (0, 0) and ops.size == 0


@pytest.mark.parametrize("name", ["EDGE20", "POS20"])
def test_free_gaps_tie_on_the_walked_paths(name):
    """(0, 0): E == H_left and F == H_up on ops of the walked paths."""
    want = want_alignments(ops_batch(), name, 0, 0)
    lefts, ups = open_ties(want, 0, 0)
    assert lefts >= 1 and ups >= 1, (lefts, ups)


@pytest.mark.parametrize("name", ["EDGE20", "POS20"])
def test_no_gap_is_worth_gap_open_at_the_edge(name):
    pairs = ops_batch()
    for k in EDGE_COSTS:
        ge, go = costs(name, pairs)[k]
        want = want_alignments(pairs, name, ge, go)
        assert gap_ops(want) == 0 and sum(ops.size for _, _, ops, _ in want) > 400


def test_positive_matrix_paths_run_from_boundary_to_boundary():
    pairs = ops_batch()
    for ge, go in costs("POS20", pairs)[:4]:
        for (a, b), (hit, begin, ops, _) in zip(pairs, want_alignments(pairs, "POS20", ge, go)):
            assert hit[0] > 0 and (hit[1] == b.size or hit[2] == a.size) and 0 in begin and ops.size


def test_tiny_pairs_idle_lanes_would_win():
    pairs = tiny_pairs()
    assert [(a.size, b.size) for a, b in pairs] == TINY + [(5, 5)] and longest(pairs) == (5, 5)
    # (a pair of one row has no cell below its own; of the others, those whose best is not on row n2)
    assert idle_lanes_outscore(pairs, "POS20", -1, -11) >= 3


@pytest.mark.parametrize("name", sorted(PERIODIC))
def test_periodic_pairs_tie_where_they_say(name):
    top, score = periodic_facts(name)
    n1, n2 = PERIODIC[name][:2]
    assert len(top) == {"row": 258, "row_offset": 257, "column": 98, "column_offset": 97, "both": 161,
                        "both_offset": 160}[name]
    assert score == 5 * min(n1, n2)


def crowd_facts():
    """The crowd's conditions; returns (the checker's alignments, the tickets)."""
    pairs = crowd()
    order = tickets(pairs)
    assert len(pairs) == 200 and 128 < len(order) < 190
    assert any(a.size == 0 and b.size for a, b in pairs) and any(b.size == 0 and a.size for a, b in pairs)
    want = want_alignments(pairs, "UNI4", *CROWD_COST)
    walked = [want[k][2].size >= 3 for k in order]
    assert sum(walked[64:128]) >= 10 and sum(walked[128:]) >= 3, (sum(walked[64:128]), sum(walked[128:]))
    return want, order


def test_crowd_fills_three_blocks_of_the_walk():
    want, order = crowd_facts()
    sizes = [crowd()[k][0].size * crowd()[k][1].size for k in order]
    assert sizes == sorted(sizes, reverse=True) and sizes[9] > 15000 and sizes[10] <= 144
