"""CPU: the scheme lists, the pairs and the conditions of tests/test_fill_range.py, so that a
failure on the device points at a kernel.

The strip fill (csrc/nw_strips.h), the panel fill (csrc/nw_rows.hip) and the band launches
around them (halo, feed and edge kernels, the row-scan finisher csrc/nw_finish.hip) took
their schemes from (1, 0, -1), (1, -1, -1), (2, -1, -2) and a handful more.  The lists here
leave that box on every side the launches distinguish.

Restated in Python and never taken from the library:
    table_form(scheme, off)  both table bytes match - off, mismatch - off fit int8; off is
                             2 gap in the w form (NW, and SW in the strips), gap for SW in the
                             panels (the u form)
    unit_kind(scheme)        match - mismatch == 1: the strips' add-with-carry compare form
    runs_tables(...)         tables iff table_form, no FLAG_NO_PROFILE and at most 7 letters
    sw_half_corner(...)      the cells of a (2, 4) half-word fill that may reach 2^16

The conditions, judged from the oracle alone for every (scheme, pair) the device module runs
(a case that fails gets another seed, SEEDS):
  1. who wins cells.  BOTH: a diagonal step strictly beats both gap steps on matching and on
     mismatching cells (with a mismatch worth a match, or nearly, gap steps then win nothing:
     (1, 1, -1), and (100, 99, -50) in a local table).  MATCH: on matching cells only -- a mismatching diagonal never wins,
     two gap steps cost no more -- and gap steps strictly win cells too.  TIES: positive gap
     with match <= 2 gap, the all-gaps path wins every cell, t = gap (i + j) throughout and
     only the tie order is tested.  ZERO (Smith-Waterman): no positive score, the table is 0.
  2. a wrong byte shows.  Outside TIES / ZERO the table differs from the table under
     (match + 1, mismatch, gap) and, for a non-zero gap, under (match, mismatch, -gap); under
     BOTH also from (match, mismatch - 1, gap), while under MATCH that table is the same one
     (asserted: the mismatch byte cannot be seen in values, as DESIGN 6g says of
     (1, -130, -1)).  An entry on the compare side of a byte edge differs from the table of
     its WRAPPED scheme -- the scores its bytes would stand for had they been packed into
     int8 tables after all (128 reads as -128, -129 as 127): that is what a launch computes
     which takes the table form one step too far, also where the neighbour across the edge
     has the same table.
  3. Smith-Waterman: the best score is positive outside ZERO, and oracle.sw_best is the first
     row-major cell holding the maximum.
"""
import functools

import numpy as np
import pytest

import nwhip
import oracle
from test_scheme_range_host import CAP, WIDE_SCHEMES

NO_PROFILE = 2  # include/nw_hip.h NW_FLAG_NO_PROFILE, restated
MAX_PERM = 7    # csrc/nw_internal.h kMaxPerm, restated
HALF_FIX_MAX = 64  # csrc/nw_internal.h kHalfFixMax, restated


# ------------------------------------------------------------------ the rules, restated
def fits_i8(x):
    return -128 <= x <= 127


def table_form(scheme, off):
    return fits_i8(scheme[0] - off) and fits_i8(scheme[1] - off)


def table_bytes(scheme, off):
    return scheme[0] - off, scheme[1] - off


def nw_off(scheme):
    return 2 * scheme[2]


def sw_off(scheme, panels):
    return scheme[2] if panels else 2 * scheme[2]


def unit_kind(scheme):
    return scheme[0] - scheme[1] == 1


def runs_tables(scheme, off, flags, letters):
    return table_form(scheme, off) and not (flags & NO_PROFILE) and letters <= MAX_PERM


def sw_half_corner(scheme, n1, n2):
    """(cells, K): the corner i, j >= K = ceil(2^16 / max(match, mismatch)) of an n1 x n2 table."""
    m = max(scheme[0], scheme[1])
    if m <= 0:
        return 0, None
    k = -(-65536 // m)
    return max(0, n2 - k + 1) * max(0, n1 - k + 1), k


def wrapped(scheme, off):
    """The scheme whose scores are this one's table bytes taken modulo 2^8 into int8."""
    w = [((v - off + 128) & 255) - 128 + off for v in scheme[:2]]
    return w[0], w[1], scheme[2]


# ------------------------------------------------------------------ the lists
LARGE_GAP = [(-4000, -4095, -2047), (4001, 3906, 2000)]  # tables under a gap of thousands
NW_WIDE = WIDE_SCHEMES + LARGE_GAP

UNIT_TABLE = [(0, -1, -3), (5, 4, -1), (1, 0, 0), (9, 8, 2)]    # SUB_UNIT only when tables are off
UNIT_COMPARE = [(64, 63, -32), (100, 99, -50), (4095, 4094, -4095)]  # SUB_UNIT is the default path
UNIT_TIES = [(-3, -4, 2), (-64, -65, 32), (-4094, -4095, 4095)]
NOT_UNIT = [(2, 0, -1), (0, 1, -1)]                             # match - mismatch = 2 and -1
NW_UNIT = UNIT_TABLE + UNIT_COMPARE + UNIT_TIES + NOT_UNIT
NW_ALL = NW_WIDE + NW_UNIT

SW_STRIP_EDGES = [(125, -1, -1), (126, -1, -1), (1, -130, -1), (1, -131, -1)]
SW_PANEL_EDGES = [(126, -1, -1), (127, -1, -1), (1, -129, -1), (1, -130, -1)]
SW_ZERO = [(-1, -3, -2), (-4000, -4095, -4095)]
SW_WIDE = SW_STRIP_EDGES + [s for s in SW_PANEL_EDGES if s not in SW_STRIP_EDGES] + \
    [(5, 0, 0), (2, 1, -1), (1, 1, -1), (7, -5, -3), (100, 99, -50), (CAP, -CAP, -CAP)] + SW_ZERO

# the bands' subset: both positive gaps that decide values, gap 0, +-4095, the unit kind as the
# default path and behind FLAG_NO_PROFILE, a large gap of either sign, both byte edges
BAND_SCHEMES = [(7, -5, 3), (9, -4, 2), (5, 0, 0), (CAP, -CAP, -CAP), (64, 63, -32), (-4000, -4095, -2047),
                (1, -130, -1), (126, -1, -1), (4001, 3906, 2000), (0, -1, -3)]

# condition 1: who wins cells
NW_TIES = [(2, -3, 1), (-5, -200, 3)] + UNIT_TIES
NW_MATCH = [(1, -130, -1), (1, -131, -1), (7, -5, 3), (9, -4, 2), (5, 0, 0), (1, 0, 0)] + LARGE_GAP
NW_BOTH = [s for s in NW_ALL if s not in NW_TIES + NW_MATCH]
SW_MATCH = [(1, -129, -1), (1, -130, -1), (1, -131, -1), (5, 0, 0)]
SW_BOTH = [s for s in SW_WIDE if s not in SW_MATCH + SW_ZERO]


# ------------------------------------------------------------------ the pairs
STRIP, PANEL, TALL = (600, 200), (1100, 130), (300, 1000)      # (n1, n2)
ROWS_A, ROWS_B, COLS, TB_B, FINISH = (1000, 777), (640, 130), (3000, 300), (97, 1025), (300, 587)
FILL_SIZES = [STRIP, PANEL, TALL]
BAND_SIZES = [ROWS_A, ROWS_B, COLS, TB_B, FINISH]
ALPHAS = [4, 20]
# seeds that differ from the default (100 alpha + n1 + 7 n2), and what the default failed
SEEDS = {}


def mutated_window(rng, s1, n2, alpha):
    """n2 letters: a window of s1 (s1 repeated where it is the shorter) with about 2.5 % of its
    letters dropped, 2.5 % doubled, and then 10 % replaced by another letter of 1..alpha."""
    m = n2 + n2 // 8 + 8
    if s1.size >= m:
        start = int(rng.integers(0, s1.size - m + 1))
        src = s1[start:start + m]
    else:
        src = np.resize(np.roll(s1, -int(rng.integers(0, s1.size))), m)
    count = (rng.random(m) >= 0.025).astype(np.int64) + (rng.random(m) < 0.025)
    s2 = np.repeat(src, count)[:n2].copy()
    assert s2.size == n2
    sub = rng.random(n2) < 0.10
    s2[sub] = (s2[sub] - 1 + rng.integers(1, alpha, int(sub.sum()))) % alpha + 1
    return s2


@functools.lru_cache(maxsize=None)
def pair(alpha, shape):
    """(s1, s2) over the bytes 1..alpha: s1 uniform, s2 = mutated_window of it."""
    n1, n2 = shape
    rng = np.random.default_rng(SEEDS.get((alpha, n1, n2), 100 * alpha + n1 + 7 * n2))
    s1 = rng.integers(1, alpha + 1, n1).astype(np.int8)
    s2 = mutated_window(rng, s1, n2, alpha)
    for a in (s1, s2):
        a.setflags(write=False)
    return s1, s2


@functools.lru_cache(maxsize=None)
def nw_table(alpha, shape, scheme):
    t = oracle.fill(*pair(alpha, shape), scheme)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def sw_table(alpha, shape, scheme):
    t = oracle.sw_fill(*pair(alpha, shape), scheme)
    t.setflags(write=False)
    return t


# the half-word cases: (s1, s2, scheme)
def half_identical(n1, n2):
    """One letter throughout: t[i][j] = 4095 min(i, j) under (4095, -4095, -4095)."""
    return np.full(n1, 3, np.int8), np.full(n2, 3, np.int8), (CAP, -CAP, -CAP)


def half_never_match(n):
    """Disjoint letters under (3, 4095, -1): every step a mismatch worth 4095."""
    return np.full(n, 1, np.int8), np.full(n, 2, np.int8), (3, CAP, -1)


# ------------------------------------------------------------------ who wins cells
def wins(s1, s2, t, scheme, sw=False):
    """(matching cells a diagonal strictly wins, mismatching ones, cells a gap step strictly wins)."""
    m, mm, g = scheme
    t = t.astype(np.int64)
    eq = s2[:, None] == s1[None, :]
    d = t[:-1, :-1] + np.where(eq, m, mm)
    gaps = np.maximum(t[:-1, 1:], t[1:, :-1]) + g
    if sw:
        d, gaps = np.maximum(d, 0), np.maximum(gaps, 0)  # a step that only ties the floor wins nothing
    return int((eq & (d > gaps)).sum()), int((~eq & (d > gaps)).sum()), int((gaps > d).sum())


@functools.lru_cache(maxsize=None)
def check_nw(alpha, shape, scheme):
    """Conditions 1 and 2 for an NW fill of this pair (judged once: the device module asks again
    before every fill)."""
    s1, s2 = pair(alpha, shape)
    t = nw_table(alpha, shape, scheme)
    m, mm, g = scheme
    dm, dx, gw = wins(s1, s2, t, scheme)
    what = f"{scheme} {alpha} {shape}: {dm} {dx} {gw}"
    if scheme in NW_TIES:
        n2, n1 = s2.size, s1.size
        assert (t == g * (np.arange(n2 + 1)[:, None] + np.arange(n1 + 1)[None, :])).all() and dm == dx == 0, what
        return
    other = lambda s: oracle.fill(s1, s2, s)  # noqa: E731
    assert dm > 0, what
    assert (t != other((m + 1, mm, g))).any(), what
    if g != 0:
        assert (t != other((m, mm, -g))).any(), what
    if scheme in NW_MATCH:
        assert dx == 0 and gw > 0 and (t == other((m, mm - 1, g))).all(), what
    else:
        assert scheme in NW_BOTH and dx > 0 and (t != other((m, mm - 1, g))).any(), what
    if not table_form(scheme, 2 * g):
        assert (t != other(wrapped(scheme, 2 * g))).any(), what


@functools.lru_cache(maxsize=None)
def check_sw(alpha, shape, scheme):
    """Conditions 1 to 3 for an SW fill of this pair."""
    s1, s2 = pair(alpha, shape)
    t = sw_table(alpha, shape, scheme)
    m, mm, g = scheme
    best = oracle.sw_best(s1, s2, scheme)
    what = f"{scheme} {alpha} {shape}: {best}"
    if scheme in SW_ZERO:
        assert not t.any() and best == (0, 0, 0), what
        return
    dm, dx, gw = wins(s1, s2, t, scheme, sw=True)
    what += f" {dm} {dx} {gw}"
    first = int(np.argmax(t))  # the first row-major maximum
    assert best[0] == t.max() > 0 and best[1:] == divmod(first, t.shape[1]), what
    other = lambda s: oracle.sw_fill(s1, s2, s)  # noqa: E731
    assert dm > 0, what
    assert (t != other((m + 1, mm, g))).any(), what
    if scheme in SW_MATCH:
        assert dx == 0 and gw > 0 and (t == other((m, mm - 1, g))).all(), what
    else:
        assert scheme in SW_BOTH and dx > 0 and (t != other((m, mm - 1, g))).any(), what
    for off in (2 * g, g):  # strips, panels
        if not table_form(scheme, off):
            assert (t != other(wrapped(scheme, off))).any(), what


# ================================================================== tests
def test_the_lists_sit_where_they_say():
    assert len(set(NW_ALL)) == len(NW_ALL) == 26 and len(set(SW_WIDE)) == len(SW_WIDE) == 14
    assert all(max(abs(v) for v in s) <= CAP for s in NW_ALL + SW_WIDE) and all(s[2] <= 0 for s in SW_WIDE)
    nb = {s: table_bytes(s, nw_off(s)) for s in NW_ALL}
    # the large gaps: thousands a step in the w form, small bytes
    assert nb[(-4000, -4095, -2047)] == (94, -1) and nb[(4001, 3906, 2000)] == (1, -94)
    assert all(table_form(s, nw_off(s)) for s in LARGE_GAP)
    # the unit kind
    assert all(unit_kind(s) for s in UNIT_TABLE + UNIT_COMPARE + UNIT_TIES) and not any(unit_kind(s) for s in NOT_UNIT)
    assert [s[0] - s[1] for s in NOT_UNIT] == [2, -1]
    assert [s for s in NW_WIDE if unit_kind(s)] == []  # the wide list never reaches SUB_UNIT
    assert [nb[s] for s in UNIT_TABLE] == [(6, 5), (7, 6), (1, 0), (5, 4)]
    assert all(table_form(s, nw_off(s)) for s in UNIT_TABLE + NOT_UNIT)
    assert [nb[s] for s in UNIT_COMPARE] == [(128, 127), (200, 199), (12285, 12284)]
    assert not any(table_form(s, nw_off(s)) for s in UNIT_COMPARE)
    # SUB_UNIT's addend mismatch - 2 gap: positive, zero, negative, large
    assert sorted(nb[s][1] for s in UNIT_TABLE + UNIT_COMPARE + UNIT_TIES) == [-12285, -129, -8, 0, 4, 5, 6, 127, 199,
                                                                              12284]
    assert [nb[s] for s in UNIT_TIES] == [(-7, -8), (-128, -129), (-12284, -12285)]
    assert [table_form(s, nw_off(s)) for s in UNIT_TIES] == [True, False, False]
    assert all(s[2] > 0 and s[0] <= 2 * s[2] for s in NW_TIES)
    assert sorted(s[2] for s in UNIT_TABLE) == [-3, -1, 0, 2]
    # Smith-Waterman: the two families' edges, and each entry's side for the other family
    st = {s: table_bytes(s, sw_off(s, False)) for s in SW_WIDE}
    pn = {s: table_bytes(s, sw_off(s, True)) for s in SW_WIDE}
    assert [st[s] for s in SW_STRIP_EDGES] == [(127, 1), (128, 1), (3, -128), (3, -129)]
    assert [table_form(s, sw_off(s, False)) for s in SW_STRIP_EDGES] == [True, False, True, False]
    assert [table_form(s, sw_off(s, True)) for s in SW_STRIP_EDGES] == [True, True, False, False]
    assert [pn[s] for s in SW_PANEL_EDGES] == [(127, 0), (128, 0), (2, -128), (2, -129)]
    assert [table_form(s, sw_off(s, True)) for s in SW_PANEL_EDGES] == [True, False, True, False]
    assert [table_form(s, sw_off(s, False)) for s in SW_PANEL_EDGES] == [False, False, True, True]
    assert pn[(-4000, -4095, -4095)] == (95, 0) and st[(-4000, -4095, -4095)] == (4190, 4095)
    assert [s for s in SW_WIDE if table_form(s, sw_off(s, True)) != table_form(s, sw_off(s, False))] == \
        [(126, -1, -1), (1, -130, -1), (-4000, -4095, -4095)]
    assert all(max(s[0], s[1]) <= 0 for s in SW_ZERO) and all(max(s[0], s[1]) > 0 for s in SW_BOTH + SW_MATCH)
    # the bands' subset holds what it must, and both forms and both kinds
    must = [(7, -5, 3), (9, -4, 2), (5, 0, 0), (CAP, -CAP, -CAP), (64, 63, -32), (-4000, -4095, -2047), (1, -130, -1),
            (126, -1, -1)]
    assert set(must) <= set(BAND_SCHEMES) <= set(NW_ALL) and len(BAND_SCHEMES) == 10
    assert not set(BAND_SCHEMES) & set(NW_TIES)
    assert sum(table_form(s, nw_off(s)) for s in BAND_SCHEMES) == 7 and sum(unit_kind(s) for s in BAND_SCHEMES) == 2
    # every scheme is in exactly one class
    assert sorted(NW_TIES + NW_MATCH + NW_BOTH) == sorted(NW_ALL) and set(NW_MATCH) <= set(NW_ALL)
    assert sorted(SW_ZERO + SW_MATCH + SW_BOTH) == sorted(SW_WIDE)
    # a mismatching diagonal can beat two gap steps only where mismatch > 2 gap
    assert all(s[1] <= 2 * s[2] for s in NW_MATCH + SW_MATCH) and all(s[1] > 2 * s[2] for s in NW_BOTH + SW_BOTH)


def test_wrapped_is_what_int8_tables_would_hold():
    assert wrapped((126, -1, -1), -2) == (-130, -1, -1)   # 128 reads as -128
    assert wrapped((1, -131, -1), -2) == (1, 125, -1)     # -129 reads as 127
    assert wrapped((127, -1, -1), -1) == (-129, -1, -1) and wrapped((1, -130, -1), -1) == (1, 126, -1)
    assert wrapped((64, 63, -32), -64) == (-192, 63, -32)
    for s in NW_ALL + SW_WIDE:
        for off in (2 * s[2], s[2]):
            assert (wrapped(s, off) == s) == table_form(s, off)
            assert table_form(wrapped(s, off), off)


def test_form_rule():
    for s in NW_ALL:
        off = nw_off(s)
        assert runs_tables(s, off, 0, 4) == table_form(s, off)
        assert not runs_tables(s, off, NO_PROFILE, 4) and not runs_tables(s, off, 0, 20) and not runs_tables(s, off, 0, 8)
        assert runs_tables(s, off, 0, 7) == table_form(s, off)
    # the unit kind is what runs: never under tables
    assert [s for s in NW_UNIT if unit_kind(s) and not runs_tables(s, nw_off(s), 0, 4)] == UNIT_COMPARE + UNIT_TIES[1:]
    # every pair holds the letters it says: 4 -> tables may run, 20 -> compares
    for alpha in ALPHAS:
        for shape in FILL_SIZES + BAND_SIZES:
            s1, s2 = pair(alpha, shape)
            nd = np.unique(s1).size  # (the 97 columns of TB_B hold 19 of the 20)
            assert (nd == 4 if alpha == 4 else MAX_PERM < nd <= 20) and s1.min() >= 1 and s1.max() <= alpha
            assert s2.min() >= 1 and s2.max() <= alpha and (s1.size, s2.size) == shape


def test_generator_keeps_matches_in_charge():
    """s2 follows s1: along the best global path about 85 % of the diagonal steps match, far
    from the 1 / alpha of independent letters."""
    for alpha in ALPHAS:
        for shape in [STRIP, PANEL, ROWS_A]:
            s1, s2 = pair(alpha, shape)
            local = oracle.sw_best(s1, s2, (1, -1, -1))[0]
            assert local > 0.6 * min(shape), (alpha, shape, local)


def test_half_word_corner_rule():
    assert sw_half_corner((CAP, -CAP, -CAP), 24, 24) == (64, 17) and sw_half_corner((CAP, -CAP, -CAP), 25, 24) == (72, 17)
    assert sw_half_corner((3, CAP, -1), 24, 24) == (64, 17) and sw_half_corner((3, 3, -1), 24, 24)[0] == 0
    assert sw_half_corner((100, -100, -1), 660, 660) == (25, 656) and sw_half_corner((100, -100, -1), 700, 700)[0] == 45 * 45
    assert sw_half_corner((-1, -3, -2), 10 ** 6, 10 ** 6) == (0, None)
    # at 600 x 200 every entry but the largest has an empty corner
    assert [s for s in SW_WIDE if sw_half_corner(s, *STRIP)[0] > HALF_FIX_MAX] == [(CAP, -CAP, -CAP)]
    assert all(sw_half_corner(s, *STRIP)[0] == 0 for s in SW_WIDE if s != (CAP, -CAP, -CAP))
    # the 64 cells of the corner are all at or beyond 2^16, and nothing outside it is
    s1, s2, scheme = half_identical(24, 24)
    t = oracle.sw_fill(s1, s2, scheme)
    assert (t[17:, 17:] >= 65536).all() and t[17:, 17:].size == HALF_FIX_MAX and t.max() == 24 * CAP
    t[17:, 17:] = 0
    assert t.max() < 65536
    s1, s2, scheme = half_identical(25, 24)
    assert (oracle.sw_fill(s1, s2, scheme)[17:, 17:] >= 65536).all()
    s1, s2, scheme = half_never_match(24)
    t = oracle.sw_fill(s1, s2, scheme)
    assert not (s1[None, :] == s2[:, None]).any() and (t[17:, 17:] >= 65536).all() and (t[:17].max() < 65536)
    # with m = match the bound would see no corner here
    assert sw_half_corner((3, 3, -1), 24, 24)[0] == 0


@pytest.mark.parametrize("shape", FILL_SIZES)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_nw_conditions_fills(alpha, shape):
    for scheme in NW_ALL:
        check_nw(alpha, shape, scheme)


@pytest.mark.parametrize("shape", FILL_SIZES)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_sw_conditions_fills(alpha, shape):
    for scheme in SW_WIDE:
        check_sw(alpha, shape, scheme)


@pytest.mark.parametrize("shape", BAND_SIZES)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_nw_conditions_bands(alpha, shape):
    for scheme in BAND_SCHEMES:
        check_nw(alpha, shape, scheme)


def test_unit_neighbours_compute_other_tables():
    """Taken for the unit kind, a scheme with match - mismatch = 2 or -1 would score a match as
    mismatch + 1: that table differs from its own."""
    for alpha in ALPHAS:
        for shape in FILL_SIZES:
            for m, mm, g in NOT_UNIT:
                assert (nw_table(alpha, shape, (m, mm, g)) != oracle.fill(*pair(alpha, shape), (mm + 1, mm, g))).any()


def test_no_entry_is_refused_by_contract():
    """nw_params takes every scheme here, also for Smith-Waterman, and the w-form range bound is
    far away at these sizes: valid arguments reach the device (or its absence)."""
    from test_batch_host import VALID
    from test_scheme_range_host import lin_sum, status_of
    assert all(lin_sum(s, 3000, 1025) * 8 < 2 ** 28 for s in NW_ALL + SW_WIDE)
    a, b = pair(4, STRIP)
    for s in NW_ALL:
        assert status_of(nwhip.fill, a[:70], b[:40], s) in VALID
    for s in SW_WIDE:
        assert status_of(nwhip.sw_align, a[:70], b[:40], s) in VALID
