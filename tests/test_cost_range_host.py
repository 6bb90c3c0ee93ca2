"""CPU: the gap costs, bands, `ends`, matrices and pairs of tests/test_cost_range.py, and the
checkers of the four newest batch families on them (tests/nw_semi.py, nw_banded.py, nw_gotoh2.py,
nw_banded2.py), so that a failure on the device points at a kernel.

Every other device test of the semi-global, banded, two-piece and banded two-piece entries draws
(ge, go) from (-1, -11), (-2, -3), (-3, 0), (-2, -11), two-piece costs with |v| <= 24 and one int8-span
case with ge1 in {-1, -64, 0, 1}.  Here:
  * COSTS: ge = 0 (with go = 0 every E and F ties with an H), a positive extension of 1 and of 4095
    (inside a band the path then follows a band edge), ge = -4095, and gap_open at the last value the
    range bound takes for the batch's longest pair,
        3 |go| + (max(M, |ge|) + |ge|) * (n1 + n2 + 2) < 2^28
    (test_scheme_range_host.go_edge: the bound restated, never taken from the library), beside ge =
    -1, -4095 and +4095;
  * PIECES: two-piece costs whose piece-2 values drift by dge = ge2 - ge1 = +4094, -8190 and +8190 a
    step, zero pieces, and openings at the edge of the two-piece bound
        3 max|go_t| + (max(M, A) + A) * (n1 + n2 + 2) < 2^28,  A = max |ge_t|
    with both pieces alive (crossing at 50 and at 40) and with the edge piece dominated;
  * bands 0, 3, 64 and a covering one (0..2 for the pairs of 1 x 1 .. 5 x 5); `ends` 0, 3, 12, 15, 6, 9;
  * the matrix of tests/test_batch_dual_host.py (entries -8..12) and, for two costs per family
    (ge = 0: the table bytes are the entries; ge = -1 with the openings at the edge: the wide form),
    EDGE20 of tests/test_local_range_host.py (127 and -128 in every byte of a profile dword);
  * 200 pairs for the one-thread-per-ticket walks and for chunks of more than 64 pairs.
Each condition that makes a case mean something is a function here, judged from the checker alone;
the GPU module asserts the same functions before it looks at the device's result.
"""
import collections
import functools

import numpy as np
import pytest

import nw_banded as nb
import nw_banded2 as b2
import nw_gotoh2 as g2
import nw_gotoh_matrix as gm
import nw_semi as ns
import nwhip
import test_batch_dual_host as tdh
import test_local_range_host as tlh
from test_batch import _rand, ops_pairs, score_pairs
from test_batch_host import VALID
from test_batch_semi_host import _brute as semi_brute
from test_scheme_range_host import CAP, LIMIT, TINY, go_edge, rand_pair, status_of

COVER = 10 ** 6
BANDS = [0, 3, 64, COVER]
TINY_BANDS = [0, 1, 2, 3, COVER]
SCORE_ENDS = [0, 3, 12, 15, 6, 9]
OPS_ENDS = [3, 12, 9]   # every NW_ENDS_* bit; 12 and 9 run the kernel that tracks column n1
SMALL = [(5, 3), (3, 5), (17, 9), (40, 33)]   # the literal fills' shapes


def matrix(name="M20"):
    """M20: tests/test_batch_dual_host.py matrix(20), entries -8..12; EDGE20: tests/test_local_range_host.py's."""
    return tdh.matrix(20) if name == "M20" else tlh.matrix(name)


def mat_abs(name):
    return int(np.abs(matrix(name).scores).max())


# ------------------------------------------------------------------ pairs
@functools.lru_cache(maxsize=None)
def ops20():
    """tests/test_batch.py ops_pairs()' sizes re-drawn over 20 letters (tests/test_batch_dual.py ops_pairs20)."""
    rng = np.random.default_rng(78)
    return tuple((_rand(rng, a.size, 20), _rand(rng, b.size, 20)) for a, b in ops_pairs())


SQUARE = [(300, 300), (257, 256), (256, 257), (130, 130)]


@functools.lru_cache(maxsize=None)
def band_ops():
    """ops20(), the transposed pairs of those with more than 60 rows and columns, 513 x 130 both
    ways, and the near-square pairs SQUARE (last): there |n2 - n1| adds nothing to the band, and a
    path that is all gaps crosses it from edge to edge."""
    extra = [rand_pair(1303, 513, 130, 20), rand_pair(1304, 130, 513, 20)]
    extra += [rand_pair(1400 + k, n1, n2, 20) for k, (n1, n2) in enumerate(SQUARE)]
    return ops20() + tuple((b, a) for a, b in ops20() if a.size > 60 and b.size > 60) + tuple(extra)


@functools.lru_cache(maxsize=None)
def dual_score():
    """score_pairs(20) and 300 x 270 / 270 x 300: a side difference of 30, below both crossings
    of the edge pieces, next to the differences of 125 and more of the grid."""
    return score_pairs(20) + (rand_pair(1301, 300, 270, 20), rand_pair(1302, 270, 300, 20))


@functools.lru_cache(maxsize=None)
def crowd():
    """200 pairs over 20 letters, shuffled: 190 with both sides drawn from 0..12 and ten of about
    300 x 70 (the recipe of tests/test_scheme_range.py crowd, a seed of its own)."""
    rng = np.random.default_rng(1310)
    sizes = [(int(rng.integers(0, 13)), int(rng.integers(0, 13))) for _ in range(190)]
    sizes += [(int(rng.integers(280, 321)), int(rng.integers(60, 81))) for _ in range(10)]
    pairs = [(_rand(rng, n1, 20), _rand(rng, n2, 20)) for n1, n2 in sizes]
    return tuple(pairs[i] for i in rng.permutation(len(pairs)))


BATCHES = {"score": lambda: score_pairs(20), "ops": ops20, "band_ops": band_ops, "dual_score": dual_score,
           "tiny": tlh.tiny_pairs, "crowd": crowd}
LONGEST = {"score": (513, 130), "ops": (600, 200), "band_ops": (600, 200), "dual_score": (513, 130), "tiny": (5, 5),
           "crowd": None}


def pairs_of(batch):
    return BATCHES[batch]()


def longest(batch):
    return tlh.longest(pairs_of(batch))


# ------------------------------------------------------------------ costs
N_COSTS = 9
GO_EDGE = (6, 7, 8)       # their places in costs()
POSITIVE = (2, 3, 8)      # ge > 0
HUGGING = (3,)            # a positive extension above every matrix entry and no opening: (4095, 0)
# Not of the nine: a positive extension WITH an opening, for the banded entries.  The best path is
# all gaps in as few runs as the band lets it make: it crosses the band from edge to edge.
ZIGZAG = (CAP, -11)
ZIGZAG_PIECES = (-11, CAP, -7, CAP - 1)   # piece 2 for runs of 1 to 3, piece 1 from 4 on
HUG_PIECES = (0, CAP, -7, CAP - 1)        # (4095, 0) and a dominated piece 2: the two-piece band the same way


def costs(batch, name="M20"):
    """The nine (ge, go) of a batch: the three edges are that batch's own."""
    shape, m = longest(batch), mat_abs(name)
    return [(0, 0), (0, -7), (1, 0), (CAP, 0), (-CAP, 0), (-CAP, -11)] + \
        [(ge, go_edge((0, 0, ge), *shape, mat_abs=m)) for ge in (-1, -CAP, CAP)]


def dual_edge(a, shape, m=12):
    """The largest max |go_t| the two-piece bound takes for a pair of `shape` with A = a."""
    g = (LIMIT - 1 - (max(m, a) + a) * (sum(shape) + 2)) // 3
    assert dual_sum(g, a, shape, m) < LIMIT <= dual_sum(g + 1, a, shape, m)
    return g


def dual_sum(g, a, shape, m=12):
    return 3 * g + (max(m, a) + a) * (sum(shape) + 2)


N_PIECES = 10
CROSSING = (0, 1, 2, 3, 4, 6, 7)   # their places in pieces(): two pieces, each the better one somewhere
MIXED = (3, 4)                     # piece_mix holds: single paths priced by both pieces
OPEN_EDGE = (6, 7, 8, 9)           # an opening at the edge of the bound


def pieces(batch, name="M20"):
    """The ten (go1, ge1, go2, ge2) of a batch; g and h are the batch's own edges beside A = 2 and
    A = 4095."""
    shape, m = longest(batch), mat_abs(name)
    g, h = dual_edge(2, shape, m), dual_edge(CAP, shape, m)
    return [(0, -CAP, -81900, -1),             # dge = +4094; piece 2 from a run of 21 on
            (-40950, CAP, 0, -CAP),            # dge = -8190; piece 1 (a positive extension) from 6 on
            (0, -CAP, -40950, CAP),            # dge = +8190; piece 2 from 6 on
            (0, 0, -7, 1),                     # piece 2 from 8 on
            (-3, 0, 0, -2),                    # piece 2 for a run of 1, piece 1 from 2 on
            (0, 0, 0, 0),                      # equal zero pieces: everything ties
            (-g, -1, -g + 50, -2),             # both openings at the edge, crossing at 50
            (-h + 4094 * 40, -CAP, -h, -1),    # the same beside 4095, crossing at 40
            (-g, -2, -24, -1),                 # piece 1 at the edge and dominated
            (-4, -2, -g, -1)]                  # piece 2 at the edge and dominated


def kw(pc, w=None):
    """The Python entries' keywords of (go1, ge1, go2, ge2), and of the band."""
    k = dict(gap_open=pc[0], gap=pc[1], gap_open2=pc[2], gap2=pc[3])
    if w is not None:
        k["band"] = w
    return k


# ------------------------------------------------------------------ the checkers' results, once
Semi = collections.namedtuple("Semi", "hit begin ops ties tied_ends")
Glob = collections.namedtuple("Glob", "score ops ties")


def _run_ties(ops, cells, H, run, open_ext):
    """(lefts, ups) among `ops` at which the run value one cell back plus the extension equals
    H there plus opening and extension: "opening wins" decides the state after that op.
    run: {op: (table, ge)}; cells: the cell each op arrives at."""
    lefts = ups = 0
    for op, (i, j) in zip(ops.tolist(), cells):
        if op == 2 and run[2][0][i, j - 1] + run[2][1] == H[i, j - 1] + open_ext:
            lefts += 1
        if op == 1 and run[1][0][i - 1, j] + run[1][1] == H[i - 1, j] + open_ext:
            ups += 1
    return lefts, ups


@functools.lru_cache(maxsize=None)
def semi_want(batch, name, ge, go, ends, walks=True):
    """Per pair Semi(hit (score, i, j), begin, ops, (lefts, ups) tied, the number of admissible
    end cells that hold the score); without `walks` the hit and tied_ends alone."""
    m = matrix(name)
    out = []
    for a, b in pairs_of(batch):
        tables = ns.fill(a, b, m.scores, m.index, ge, go, ends)
        H = tables[0]
        hit = ns.end_cell(H, ends)
        tied = sum(H[i, j] == hit[0] for i, j in ns.end_cells(a.size, b.size, ends))
        if not walks:
            out.append(Semi(hit, None, None, None, tied))
            continue
        ops, begin = ns.walk(a, b, m.scores, m.index, ge, go, ends, tables)
        assert ns.path_score(a, b, ops, begin, m.scores, m.index, ge, go) == (hit[0], hit[1:])
        cells = tlh.path_cells(begin, ops)
        ties = _run_ties(ops, cells, H, {2: (tables[1], ge), 1: (tables[2], ge)}, go + ge)
        out.append(Semi(hit, begin, ops, ties, tied))
    return tuple(out)


def semi_hits(batch, name, ge, go, ends):
    return np.array([w.hit for w in semi_want(batch, name, ge, go, ends, False)], np.int32)


@functools.lru_cache(maxsize=None)
def banded_want(batch, name, ge, go, w):
    m = matrix(name)
    out = []
    for a, b in pairs_of(batch):
        tables = nb.fill(a, b, m.scores, m.index, ge, go, w)
        ops = nb.walk(a, b, m.scores, m.index, ge, go, w, tables=tables)
        sc = int(tables[0][-1, -1])
        assert nb.path_score(a, b, ops, m.scores, m.index, ge, go) == sc
        ties = _run_ties(ops, nb.path_vertices(ops)[1:], tables[0], {2: (tables[1], ge), 1: (tables[2], ge)}, go + ge)
        out.append(Glob(sc, ops, ties))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def dual_want(batch, name, pc, w=None):
    """Two-piece, unbanded (w None: tests/nw_gotoh2.py) or in a band (tests/nw_banded2.py)."""
    m = matrix(name)
    out = []
    for a, b in pairs_of(batch):
        if w is None:
            tabs = g2.fill(a, b, m.scores, m.index, pc)
            ops = g2.walk(a, b, m.scores, m.index, pc, tabs)
        else:
            tabs = b2.fill(a, b, m.scores, m.index, pc, w)
            ops = b2.walk(a, b, m.scores, m.index, pc, w, tables=tabs)
        sc = int(tabs[0][-1, -1])
        assert g2.path_score(a, b, ops, m.scores, m.index, pc) == sc
        # (the ties of piece 1's run values: under equal pieces the walk takes piece 1's states)
        ties = _run_ties(ops, nb.path_vertices(ops)[1:], tabs[0], {2: (tabs[1], pc[1]), 1: (tabs[2], pc[1])},
                         pc[0] + pc[1])
        out.append(Glob(sc, ops, ties))
    return tuple(out)


def scores_of(want):
    return np.array([w.score for w in want], np.int32)


# ------------------------------------------------------------------ the conditions
def piece_use(batch, pc, name="M20"):
    """(pairs priced by piece 1 alone, pairs priced by piece 2 alone, pairs of more than 60 rows
    and columns, those of them whose score is neither piece's own): the two-piece score against
    tests/nw_gotoh_matrix.py under each piece by itself."""
    m = matrix(name)
    want = scores_of(dual_want(batch, name, pc))
    one = np.array([gm.score(a, b, m.scores, m.index, pc[1], pc[0]) for a, b in pairs_of(batch)])
    two = np.array([gm.score(a, b, m.scores, m.index, pc[3], pc[2]) for a, b in pairs_of(batch)])
    big = np.array([a.size > 60 and b.size > 60 for a, b in pairs_of(batch)])
    mixed = (want != one) & (want != two)
    return int(((want == one) & (want != two)).sum()), int(((want == two) & (want != one)).sum()), int(big.sum()), \
        int((mixed & big).sum())


def both_pieces_count(k, pc):
    """Condition 1 for the crossing cost at place k of pieces("dual_score")."""
    if k in MIXED:
        big, mixed = tdh.piece_mix(20, pc)
        assert 3 * mixed >= big > 0, (pc, big, mixed)
    else:
        one, two, _, _ = piece_use("dual_score", pc)
        assert one >= 1 and two >= 1, (pc, one, two)


def runs_of(ops):
    """[(op, length)] of the maximal runs of ups and of lefts."""
    out, last = [], 0
    for op in ops.tolist():
        if op and op == last:
            out[-1][1] += 1
        elif op:
            out.append([op, 1])
        last = op
    return [tuple(r) for r in out]


def edge_vertices(a, b, ops, w):
    """(path vertices on diagonal dlo, on diagonal dhi) of a global path inside the band w."""
    dlo, dhi = nb.limits(a.size, b.size, w)
    d = [i - j for i, j in nb.path_vertices(ops)]
    return d.count(dlo), d.count(dhi)


def band_edge_decides(batch, want, w):
    """Condition 2 under (4095, 0): every pair with more than max(60, 2 w) rows and columns has at
    least 50 path vertices on a band edge (the shapes of 64 and 65 rows fall short at w = 64: their
    path reaches the edge 1 or 2 vertices before the boundary).  Returns the counts (min, max)."""
    side = max(60, 2 * w)
    on = [max(edge_vertices(a, b, x.ops, w)) for (a, b), x in zip(pairs_of(batch), want)
          if a.size > side and b.size > side]
    assert len(on) >= 12 and min(on) >= 50, (w, sorted(on)[:4])
    return min(on), max(on)


def both_edges_decide(score, walk, w):
    """Condition 2 under ZIGZAG / ZIGZAG_PIECES on the near-square pairs: moving dlo in by one
    diagonal changes the checker's score, and moving dhi in by one does; the 300 x 300 path has
    50 vertices on each edge.  score(a, b, dlo, dhi), walk(a, b) -> ops: the family's checker."""
    pairs = band_ops()[-len(SQUARE):]
    assert [(a.size, b.size) for a, b in pairs] == SQUARE
    touch = []
    for a, b in pairs:
        dlo, dhi = nb.limits(a.size, b.size, w)
        sc = score(a, b, dlo, dhi)
        assert score(a, b, dlo + 1, dhi) != sc and score(a, b, dlo, dhi - 1) != sc, (a.size, b.size)
        touch.append(edge_vertices(a, b, walk(a, b), w))
    assert min(touch[0]) >= 50 and min(min(t) for t in touch) >= 20, touch
    return touch


def ties_decide(want):
    """Condition 3, first part: lefts and ups at which the run value ties with the extension."""
    lefts, ups = sum(x.ties[0] for x in want), sum(x.ties[1] for x in want)
    assert lefts >= 10 and ups >= 10, (lefts, ups)
    return lefts, ups


def end_ties_decide(want, pairs):
    """Condition 3, second part: a pair with three or more equal-scoring admissible end cells
    (end_cell takes the first in row-major order, by its definition).  Returns the largest count."""
    most = max(x.tied_ends for x, (a, b) in zip(want, pairs) if a.size and b.size)
    assert most >= 3, most
    return most


def interior_ends(want, pairs, ends):
    """Condition 4: the pairs that end strictly inside the last row or the last column."""
    n = 0
    for x, (a, b) in zip(want, pairs):
        _, i, j = x.hit
        n += (ends & 2 and i == b.size and 0 < j < a.size) or (ends & 8 and j == a.size and 0 < i < b.size)
    return int(n)


def tickets(pairs):
    """The indices of the pairs with cells, longest first (the library's stable order)."""
    return tlh.tickets(pairs)


def crowd_walks(want):
    """Condition 5: (tickets 64..127, tickets from 128) whose path has three ops or more."""
    order = tickets(crowd())
    walked = [want[k].ops.size >= 3 for k in order]
    mid, far = sum(walked[64:128]), sum(walked[128:])
    assert len(crowd()) == 200 and 128 < len(order) < 190
    assert mid >= 10 and far >= 10, (mid, far)
    return mid, far


def semi_idle_lanes_outscore(pairs, name, ge, go, ends):
    """The pairs for which the table over s1 continued with its last letter (what the lanes past
    n1 compute) holds, on the last row, a value above the pair's own end cell's."""
    m = matrix(name)
    n = 0
    for a, b in pairs:
        wide = np.concatenate([a, np.full(12, a[-1], np.int8)])
        own = ns.end_cell(ns.fill(a, b, m.scores, m.index, ge, go, ends)[0], ends)[0]
        n += ns.fill(wide, b, m.scores, m.index, ge, go, ends)[0][-1, a.size + 1:].max() > own
    return int(n)


CROWD_SEMI = [((0, -7), 3), ((-CAP, -11), 12)]   # ((ge, go), ends)
CROWD_BANDED = [((1, 0), 3), ((-CAP, 0), 0)]     # ((ge, go), w)
CROWD_DUAL = [(-3, 0, 0, -2), (0, -CAP, -40950, CAP)]
CROWD_DUAL_BAND = 3


# ------------------------------------------------------------------ the lists sit where they say
def test_cost_lists():
    for batch in ("score", "ops", "tiny"):
        cs = costs(batch)
        assert len(cs) == N_COSTS and cs[:6] == [(0, 0), (0, -7), (1, 0), (4095, 0), (-4095, 0), (-4095, -11)]
        assert [cs[k][0] for k in GO_EDGE] == [-1, -4095, 4095] and all(cs[k][1] < -86_000_000 for k in GO_EDGE)
        assert [k for k, (ge, _) in enumerate(cs) if ge > 0] == list(POSITIVE)
        assert longest(batch) == LONGEST[batch]
    assert [costs("score")[k][1] for k in GO_EDGE] == [-89_475_690, -87_717_635, -87_717_635]
    assert mat_abs("M20") == 12 and mat_abs("EDGE20") == 128


def test_piece_lists():
    for batch in ("dual_score", "ops", "tiny"):
        ps = pieces(batch)
        assert len(ps) == N_PIECES and len(set(ps)) == N_PIECES
        assert [p[3] - p[1] for p in ps[:3]] == [4094, -8190, 8190]
        assert all(p[0] <= 0 and p[2] <= 0 and abs(p[1]) <= CAP and abs(p[3]) <= CAP for p in ps)
        for k, pc in enumerate(ps):
            one, two = tdh.crossover(pc)
            if k in CROSSING:
                assert one.size and two.size, pc
            else:
                assert pc[:2] == pc[2:] or one.size == 0 or two.size == 0, pc
        # where the pieces cross: the last run length of the piece that prices the short runs (a
        # tie -- at 5, 5, 7, 50 and 40 -- counts for piece 1)
        first = lambda pc: (tdh.crossover(pc)[0] if tdh.crossover(pc)[0][0] == 1 else tdh.crossover(pc)[1])[-1]
        assert [first(ps[k]) for k in CROSSING] == [20, 4, 5, 7, 1, 49, 40]
        for k in OPEN_EDGE:
            assert min(ps[k][0], ps[k][2]) < -86_000_000
    g, h = dual_edge(2, (513, 130)), dual_edge(CAP, (513, 130))
    assert (g, h) == (89_475_475, 87_717_635)


# ------------------------------------------------------------------ the edges are edges
def _both(score, align, pairs, mat, *a, **k):
    return status_of(score, pairs, mat, *a, **k), status_of(align, pairs, mat, *a, **k)


REFUSED = (nwhip.NW_ERR_ARG, nwhip.NW_ERR_ARG)


@pytest.mark.parametrize("batch", ["score", "ops", "tiny"])
@pytest.mark.parametrize("name", ["M20", "EDGE20"])
def test_gap_open_edges_are_edges(name, batch):
    """go_edge is accepted and go_edge - 1 refused, by the library's own status, by the score and
    the align entry of the semi-global and the banded family; ge = +-4096 is refused.  (The
    letters do not matter to a refusal: one pair of the longest shape and a small one.)"""
    shape, mat, m = longest(batch), matrix(name), mat_abs(name)
    pairs = [rand_pair(1, *shape, 20), rand_pair(2, 5, 3, 20)]
    calls = [lambda ge, go: _both(nwhip.score_batch_semi, nwhip.align_batch_semi, pairs, mat, ge, go, 3),
             lambda ge, go: _both(nwhip.score_batch_semi, nwhip.align_batch_semi, pairs, mat, ge, go, 15),
             lambda ge, go: _both(nwhip.score_batch_banded, nwhip.align_batch_banded, pairs, mat, ge, go, 3)]
    for k in GO_EDGE:
        ge, go = costs(batch, name)[k]
        a = max(m, abs(ge)) + abs(ge)
        assert 3 * -go + a * (sum(shape) + 2) < LIMIT <= 3 * (1 - go) + a * (sum(shape) + 2)
        for f in calls:
            st = f(ge, go)
            assert st[0] in VALID and st[1] in VALID
            assert f(ge, go - 1) == REFUSED
    for f in calls:
        for ge in (CAP + 1, -CAP - 1):
            assert f(ge, 0) == f(ge, -11) == REFUSED
        for ge in (CAP, -CAP):
            st = f(ge, -11)
            assert st[0] in VALID and st[1] in VALID


@pytest.mark.parametrize("batch", ["dual_score", "ops", "tiny"])
@pytest.mark.parametrize("name", ["M20", "EDGE20"])
def test_two_piece_edges_are_edges(name, batch):
    """Each cost with an opening at the edge is accepted by the four two-piece entries and refused
    with that opening one lower; ge2 = +-4096 is refused."""
    shape, mat = longest(batch), matrix(name)
    pairs = [rand_pair(1, *shape, 20), rand_pair(2, 5, 3, 20)]
    calls = [lambda pc: _both(nwhip.score_batch_dual, nwhip.align_batch_dual, pairs, mat, **kw(pc)),
             lambda pc: _both(nwhip.score_batch_dual_banded, nwhip.align_batch_dual_banded, pairs, mat, **kw(pc, 3))]
    ps = pieces(batch, name)
    for k in OPEN_EDGE:
        pc = ps[k]
        low = min(pc[0], pc[2])
        assert dual_sum(-low, max(abs(pc[1]), abs(pc[3])), shape, mat_abs(name)) < LIMIT
        worse = tuple(v - 1 if v == low and t in (0, 2) else v for t, v in enumerate(pc))
        assert worse != pc
        for f in calls:
            st = f(pc)
            assert st[0] in VALID and st[1] in VALID
            assert f(worse) == REFUSED
    for f in calls:
        assert f((0, -CAP, -40950, CAP + 1)) == f((0, -CAP, -40950, -CAP - 1)) == REFUSED
        for pc in ps[:6]:
            st = f(pc)
            assert st[0] in VALID and st[1] in VALID


# ------------------------------------------------------------------ the checkers on these inputs
def _same_tables(got, want, minf):
    for x, y in zip(got, want):
        fin = y > minf // 2
        np.testing.assert_array_equal(x[fin], y[fin])
        assert (x[~fin] < minf // 2).all()


@pytest.mark.parametrize("k", range(N_COSTS))
def test_semi_checker_fill_equals_the_literal_fill(k):
    m = matrix()
    for n1, n2 in SMALL:
        a, b = rand_pair(1320 + n1, n1, n2, 20)
        ge, go = costs("score")[k]
        for ends in SCORE_ENDS:
            got = ns.fill(a, b, m.scores, m.index, ge, go, ends)
            _same_tables(got, ns.fill_cells(a, b, m.scores, m.index, ge, go, ends), ns.MINF)
            ops, begin = ns.walk(a, b, m.scores, m.index, ge, go, ends, got)
            sc, ei, ej = ns.end_cell(got[0], ends)
            assert ns.path_score(a, b, ops, begin, m.scores, m.index, ge, go) == (sc, (ei, ej))
            assert nwhip.ops_score_matrix(a, b, ops, m, ge, go, begin=begin) == sc


@pytest.mark.parametrize("k", range(N_COSTS))
def test_banded_checker_fill_equals_the_literal_fill(k):
    m = matrix()
    for n1, n2 in SMALL:
        a, b = rand_pair(1330 + n1, n1, n2, 20)
        ge, go = costs("score")[k]
        for w in (0, 3, COVER):
            got = nb.fill(a, b, m.scores, m.index, ge, go, w)
            _same_tables(got, nb.fill_cells(a, b, m.scores, m.index, ge, go, w), nb.MINF)
            ops = nb.walk(a, b, m.scores, m.index, ge, go, w, tables=got)
            assert nb.path_score(a, b, ops, m.scores, m.index, ge, go) == got[0][-1, -1]
            assert nwhip.ops_score_matrix(a, b, ops, m, ge, go) == got[0][-1, -1]
        np.testing.assert_array_equal(nb.fill(a, b, m.scores, m.index, ge, go, COVER)[0],
                                      gm.fill(a, b, m.scores, m.index, ge, go)[0])


@pytest.mark.parametrize("k", range(N_PIECES))
def test_two_piece_checkers_fill_equals_the_literal_fill(k):
    m = matrix()
    for n1, n2 in SMALL:
        a, b = rand_pair(1340 + n1, n1, n2, 20)
        pc = pieces("dual_score")[k]
        got = g2.fill(a, b, m.scores, m.index, pc)
        _same_tables(got, g2.fill_cells(a, b, m.scores, m.index, pc), gm.MINF)
        ops = g2.walk(a, b, m.scores, m.index, pc, got)
        assert g2.path_score(a, b, ops, m.scores, m.index, pc) == got[0][-1, -1] == nwhip.ops_score_dual(a, b, ops, m, **kw(pc))
        for w in (0, 3, COVER):
            got = b2.fill(a, b, m.scores, m.index, pc, w)
            _same_tables(got, b2.fill_cells(a, b, m.scores, m.index, pc, w), b2.MINF)
            ops = b2.walk(a, b, m.scores, m.index, pc, w, tables=got)
            assert b2.path_score(a, b, ops, m.scores, m.index, pc) == got[0][-1, -1]
        np.testing.assert_array_equal(got[0], g2.fill(a, b, m.scores, m.index, pc)[0])   # (w = COVER)


def test_checkers_are_the_definition_on_the_tiny_pairs():
    """Brute force over the path definitions, sides <= 5, for every cost that is not at the go-edge
    (there one opening is worth -87 million or more and every path is "diagonals and one run")."""
    m = matrix()
    pairs = tlh.tiny_pairs()
    assert [(a.size, b.size) for a, b in pairs] == TINY + [(5, 5)]
    above = 0
    for k, (ge, go) in enumerate(costs("tiny")):
        if k in GO_EDGE:
            continue
        for a, b in pairs:
            for ends in SCORE_ENDS:
                H = ns.fill(a, b, m.scores, m.index, ge, go, ends)[0]
                best = semi_brute(a, b, m, ge, go, ends)
                if ge <= 0:
                    assert ns.end_cell(H, ends)[0] == best, (ge, go, ends)
                else:
                    # A free end is skipped, not priced, also where pricing it would gain: under a
                    # positive extension the table (include/nw_hip.h: a free boundary holds 0) is not
                    # the best over all paths, which may run along a free boundary and be paid for it.
                    assert ns.end_cell(H, ends)[0] <= best, (ge, go, ends)
                    above += ns.end_cell(H, ends)[0] < best
                    assert ends != 0 or ns.end_cell(H, ends)[0] == best
            for w in TINY_BANDS[:3]:
                want = b2.brute(a, b, m.scores, m.index, (go, ge, go, ge), w)
                assert nb.score(a, b, m.scores, m.index, ge, go, w) == want, (ge, go, w)
    assert above >= 10
    for k, pc in enumerate(pieces("tiny")):
        if k in OPEN_EDGE:
            continue
        for a, b in pairs:
            assert g2.score(a, b, m.scores, m.index, pc) == g2.brute(a, b, m.scores, m.index, pc), pc
            for w in TINY_BANDS[:3]:
                assert b2.score(a, b, m.scores, m.index, pc, w) == b2.brute(a, b, m.scores, m.index, pc, w), (pc, w)


@pytest.mark.parametrize("k", GO_EDGE)
def test_walk_scores_at_the_edges_on_the_largest_pair(k):
    """513 x 130 under the go-edge costs: the direct sum over the checker's walk is the table's
    score for every checker (the want functions assert it for every pair they are asked for)."""
    pairs = [p for p in score_pairs(20) if p[0].size == 513 and p[1].size == 130]
    assert len(pairs) == 1
    (a, b), m = pairs[0], matrix()
    ge, go = costs("score")[k]
    for ends in (3, 12, 15):
        t = ns.fill(a, b, m.scores, m.index, ge, go, ends)
        ops, begin = ns.walk(a, b, m.scores, m.index, ge, go, ends, t)
        sc, ei, ej = ns.end_cell(t[0], ends)
        assert ns.path_score(a, b, ops, begin, m.scores, m.index, ge, go) == (sc, (ei, ej))
    for w in (3, 64):
        ops = nb.walk(a, b, m.scores, m.index, ge, go, w)
        assert nb.path_score(a, b, ops, m.scores, m.index, ge, go) == nb.score(a, b, m.scores, m.index, ge, go, w)
    for pc in [pieces("dual_score")[j] for j in OPEN_EDGE]:
        assert g2.path_score(a, b, g2.walk(a, b, m.scores, m.index, pc), m.scores, m.index, pc) == \
            g2.score(a, b, m.scores, m.index, pc)
        assert b2.path_score(a, b, b2.walk(a, b, m.scores, m.index, pc, 3), m.scores, m.index, pc) == \
            b2.score(a, b, m.scores, m.index, pc, 3)


# ------------------------------------------------------------------ the conditions hold
@pytest.mark.parametrize("k", CROSSING)
def test_both_pieces_count(k):
    pc = pieces("dual_score")[k]
    both_pieces_count(k, pc)
    one, two, big, mixed = piece_use("dual_score", pc)
    assert big == 18
    if k in MIXED:
        assert 3 * mixed >= big
    else:
        # no path is priced by both pieces: either piece's own pairs are what shows that it counts
        assert mixed == 0 and min(one, two) >= 3 and one + two >= 30
        if k in OPEN_EDGE:   # one opening outweighs a pair: one run at the most, and a run has one piece
            assert all(len(runs_of(x.ops)) <= 1 for x in dual_want("dual_score", "M20", pc))


@pytest.mark.parametrize("w", [3, 64])
@pytest.mark.parametrize("k", HUGGING)
def test_the_band_edge_decides(k, w):
    ge, go = costs("band_ops")[k]
    lo, hi = band_edge_decides("band_ops", banded_want("band_ops", "M20", ge, go, w), w)
    assert (lo, hi) == {3: (62, 298), 64: (67, 237)}[w]
    band_edge_decides("band_ops", dual_want("band_ops", "M20", HUG_PIECES, w), w)


@pytest.mark.parametrize("w", [3, 64])
@pytest.mark.parametrize("k", [k for k in POSITIVE if k not in HUGGING])
def test_the_other_positive_extensions_touch_no_band_edge(k, w):
    """Why HUGGING is (4095, 0) alone: under (1, 0) an extension does not outweigh a substitution
    score, and under (4095, go_edge) a second run costs 87 million, so no path of a pair whose band
    is widened by |n2 - n1| has a vertex on either band edge.  Condition 2 cannot be asked of them.
    Only the near-square pairs under (1, 0) at w = 3 wander to the edges, both of them, 7 to 59
    vertices a pair: short of the 50 on all but one."""
    ge, go = costs("band_ops")[k]
    want = banded_want("band_ops", "M20", ge, go, w)
    on = {(a.size, b.size): edge_vertices(a, b, x.ops, w) for (a, b), x in zip(band_ops(), want)
          if a.size > 60 and b.size > 60}
    assert len(on) == 24
    square = {s: on.pop(s) for s in SQUARE}
    assert all(t == (0, 0) for t in on.values()), on
    if (ge, go, w) == (1, 0, 3):
        assert [square[s] for s in SQUARE] == [(59, 11), (23, 12), (19, 19), (28, 7)]
    else:
        assert all(t == (0, 0) for t in square.values()), square


def test_both_band_edges_decide():
    m = matrix()
    ge, go = ZIGZAG
    t = both_edges_decide(lambda a, b, dlo, dhi: nb.score(a, b, m.scores, m.index, ge, go, dlo=dlo, dhi=dhi),
                          lambda a, b: nb.walk(a, b, m.scores, m.index, ge, go, 3), 3)
    assert t[0] == (50, 50)
    both_edges_decide(lambda a, b, dlo, dhi: b2.score(a, b, m.scores, m.index, ZIGZAG_PIECES, dlo=dlo, dhi=dhi),
                      lambda a, b: b2.walk(a, b, m.scores, m.index, ZIGZAG_PIECES, 3), 3)
    one, two = tdh.crossover(ZIGZAG_PIECES)
    assert two.tolist() == [1, 2, 3] and one[0] == 4


def test_ties_decide():
    for ends in OPS_ENDS:
        ties_decide(semi_want("ops", "M20", 0, 0, ends))
    ties_decide(banded_want("band_ops", "M20", 0, 0, 3))
    ties_decide(dual_want("ops", "M20", (0, 0, 0, 0)))
    ties_decide(dual_want("band_ops", "M20", (0, 0, 0, 0), 3))
    for ends in SCORE_ENDS[1:]:
        want = semi_want("score", "M20", 0, 0, ends, False)
        assert end_ties_decide(want, score_pairs(20)) >= 3
        for x, (a, b) in zip(want, score_pairs(20)):   # the first of the equal cells, row-major
            t = ns.fill(a, b, matrix().scores, matrix().index, 0, 0, ends)[0]
            first = min((i, j) for i, j in ns.end_cells(a.size, b.size, ends) if t[i, j] == x.hit[0])
            assert x.hit[1:] == first


@pytest.mark.parametrize("k", GO_EDGE)
def test_interior_end_cells_at_the_go_edge(k):
    ge, go = costs("score")[k]
    for ends in SCORE_ENDS[1:]:
        assert interior_ends(semi_want("score", "M20", ge, go, ends, False), score_pairs(20), ends) >= 1, ends
    ge, go = costs("ops")[k]
    for ends in OPS_ENDS:
        assert interior_ends(semi_want("ops", "M20", ge, go, ends), ops20(), ends) >= 1, ends


def test_crowd_fills_three_blocks_of_every_walk():
    pairs = crowd()
    assert any(a.size == 0 and b.size for a, b in pairs) and any(b.size == 0 and a.size for a, b in pairs)
    sizes = [pairs[k][0].size * pairs[k][1].size for k in tickets(pairs)]
    assert sizes == sorted(sizes, reverse=True) and sizes[9] > 15000 and sizes[10] <= 144
    for (ge, go), ends in CROWD_SEMI:
        crowd_walks(semi_want("crowd", "M20", ge, go, ends))
    for (ge, go), w in CROWD_BANDED:
        crowd_walks(banded_want("crowd", "M20", ge, go, w))
    for pc in CROWD_DUAL:
        crowd_walks(dual_want("crowd", "M20", pc))
        crowd_walks(dual_want("crowd", "M20", pc, CROWD_DUAL_BAND))


def test_tiny_pairs_idle_lanes_would_win():
    """The semi-global strip's lanes past n1 outscore the pair's own end cell on some pair, under a
    free end of s1, for the costs that reward or do not charge an extension."""
    pairs = tlh.tiny_pairs()
    cs = costs("tiny")
    for k in (0, 2, 3, 8):
        assert sum(semi_idle_lanes_outscore(pairs, "M20", *cs[k], ends) for ends in (3, 15, 6)) >= 1, cs[k]
