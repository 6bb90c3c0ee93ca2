"""GPU: the strip fill, the panel fill and the band launches around them over the scheme range
(tests/test_fill_range_host.py: the lists, the restated rules, the pairs and the conditions
that make a wrong byte, addend, offset or sign visible).

Every fill runs in each form it admits -- v_perm tables (4 letters), compares behind
NW_FLAG_NO_PROFILE, compares because s1 holds 20 letters -- and every comparison is exact:
oracle.fill, oracle.sw_fill, oracle.sw_best, oracle.sw_traceback.  A test is one scheme; it
runs every shape and form, collects what differs and fails with the whole list.
"""
import sys

import numpy as np
import pytest

import nwhip
import oracle
import test_tbands as tt
from conftest import PKG
from test_fill_range_host import (BAND_SCHEMES, COLS, FINISH, HALF_FIX_MAX, NO_PROFILE, NW_ALL, PANEL, ROWS_A, ROWS_B,
                                  STRIP, SW_WIDE, TALL, TB_B, check_nw, check_sw, half_identical, half_never_match,
                                  nw_table, pair, sw_half_corner, sw_table)
from test_gpu_parity import STRIP_SHAPES
from test_panels import PANEL_SHAPES, alloc_aligned_table
from test_scheme_range_host import CAP
from test_sw import SW_SHAPES

sys.path.insert(0, PKG)
import nw_bands  # noqa: E402

pytestmark = pytest.mark.gpu

assert NO_PROFILE == nwhip.FLAG_NO_PROFILE
FORMS = [(4, 0), (4, nwhip.FLAG_NO_PROFILE), (20, 0)]  # (letters, flags): tables where the bytes allow; compares twice
S, P = nwhip.KERNEL_STRIPS, nwhip.KERNEL_PANELS
POISON = -0x5A5A5A5


def sid(s):
    return ",".join(map(str, s))


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    return _t


@pytest.fixture(scope="module")
def ctx(torch):
    c = nwhip.Context(0)
    yield c
    c.close()


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the host module's pairs are read-only)


def differs(got, want):
    """'' when equal, else how many cells differ and the first of them."""
    if got.shape == want.shape and np.array_equal(got, want):
        return ""
    if got.shape != want.shape:
        return f"shape {got.shape} for {want.shape}"
    at = tuple(int(x) for x in np.argwhere(got != want)[0])
    return f"{int((got != want).sum())} cells, first {at}: {got[at]} for {want[at]}"


def report(bad):
    assert not bad, f"{len(bad)} differ:\n" + "\n".join(bad)


# ------------------------------------------------------------------ NW fills
def nw_host_fills(bad, alpha, flags, size, scheme, shapes, kernel):
    s1, s2 = pair(alpha, size)
    want = nw_table(alpha, size, scheme)
    for sh in shapes:
        t, r = nwhip.fill(s1, s2, scheme, substrips=sh[0], strip_waves=sh[1], flags=flags, kernel=kernel)
        assert (r.substrips, r.strip_waves, r.kernel) == (sh[0], sh[1], kernel)
        d = differs(t, want)
        if d or r.score != want[-1, -1]:
            bad.append(f"{size} {alpha} letters, flags {flags}, shape {sh}: {d}; score {r.score} for {want[-1, -1]}")


def nw_aligned_fills(bad, torch, ctx, alpha, flags, size, scheme, shapes, kernel):
    """Origin column 0: a 256-byte aligned base sweeps the boundary column with the strips."""
    s1, s2 = pair(alpha, size)
    want = nw_table(alpha, size, scheme)
    d1, d2 = dev(torch, s1), dev(torch, s2)
    for sh in shapes:
        tab = alloc_aligned_table(torch, s1.size, s2.size)
        tab.fill_(POISON)
        r = ctx.fill(d1, d2, tab, scheme, substrips=sh[0], strip_waves=sh[1], flags=flags, kernel=kernel)
        assert r.status == 0
        d = differs(tab[:s2.size + 1, :s1.size + 1].cpu().numpy(), want)
        if d or r.score != want[-1, -1]:
            bad.append(f"{size} {alpha} letters, flags {flags}, shape {sh}, aligned base: {d}; score {r.score}")


@pytest.mark.parametrize("scheme", NW_ALL, ids=sid)
def test_strip_fill_nw(torch, ctx, scheme):
    """600 x 200: three strips of 256 columns (ten of 64), four row blocks, a partial last strip;
    every shape of STRIP_SHAPES, and (4, 1) and (2, 2) from origin column 0."""
    bad = []
    for alpha, flags in FORMS:
        check_nw(alpha, STRIP, scheme)
        nw_host_fills(bad, alpha, flags, STRIP, scheme, STRIP_SHAPES, S)
        nw_aligned_fills(bad, torch, ctx, alpha, flags, STRIP, scheme, [(4, 1), (2, 2)], S)
    report(bad)


@pytest.mark.parametrize("scheme", NW_ALL, ids=sid)
def test_panel_fill_nw(scheme):
    """1100 x 130: two panels at (4, 4), five at (4, 1); 300 x 1000 at (4, 1) and (1, 4): sixteen
    turns of the panels' 64-row rings."""
    bad = []
    for alpha, flags in FORMS:
        check_nw(alpha, PANEL, scheme)
        check_nw(alpha, TALL, scheme)
        nw_host_fills(bad, alpha, flags, PANEL, scheme, PANEL_SHAPES, P)
        nw_host_fills(bad, alpha, flags, TALL, scheme, [(4, 1), (1, 4)], P)
    report(bad)


# ------------------------------------------------------------------ SW fills
def sw_fills(bad, torch, ctx, alpha, flags, size, scheme, shapes, kernel):
    """Table, best cell and the traceback from it."""
    s1, s2 = pair(alpha, size)
    n1, n2 = s1.size, s2.size
    want = sw_table(alpha, size, scheme)
    best = oracle.sw_best(s1, s2, scheme)
    wops, bi, bj = oracle.sw_traceback(s1, s2, want, best[1:], scheme)
    d1, d2 = dev(torch, s1), dev(torch, s2)
    for sh in shapes:
        what = f"{size} {alpha} letters, flags {flags}, shape {sh}: "
        tab = nwhip.Context.alloc_table(n1, n2)
        tab.fill_(POISON)
        r = ctx.fill(d1, d2, tab, scheme, substrips=sh[0], strip_waves=sh[1], mode=nwhip.MODE_SW, kernel=kernel,
                     flags=flags)
        assert r.status == 0 and (r.substrips, r.strip_waves, r.kernel) == (sh[0], sh[1], kernel)
        d = differs(tab[:n2 + 1, :n1 + 1].cpu().numpy(), want)
        if d:
            bad.append(what + d)
        if (r.score, r.end_i, r.end_j) != best:
            bad.append(what + f"best cell {(r.score, r.end_i, r.end_j)} for {best}")
        if d:
            continue  # (a traceback wants a table of these parameters)
        al, ops = ctx.sw_traceback(d1, d2, tab, best[1:], scheme)
        if not np.array_equal(ops, wops) or (al.begin_i, al.begin_j, al.score) != (bi, bj, best[0]):
            bad.append(what + f"traceback: {ops.size} ops to {(al.begin_i, al.begin_j)}, score {al.score}; "
                              f"{wops.size} to {(bi, bj)}, score {best[0]}")


@pytest.mark.parametrize("scheme", SW_WIDE, ids=sid)
def test_strip_fill_sw(torch, ctx, scheme):
    """The strips hold Smith-Waterman cells in the w form too: table bytes s - 2 gap."""
    bad = []
    for alpha, flags in FORMS:
        check_sw(alpha, STRIP, scheme)
        sw_fills(bad, torch, ctx, alpha, flags, STRIP, scheme, [sh for sh in SW_SHAPES if sh != (2, 4)], S)
    report(bad)


@pytest.mark.parametrize("scheme", SW_WIDE, ids=sid)
def test_panel_fill_sw(torch, ctx, scheme):
    """The panels' u form: table bytes s - gap, the prefix tables' floor, z_j = -gap j."""
    bad = []
    for alpha, flags in FORMS:
        check_sw(alpha, PANEL, scheme)
        check_sw(alpha, TALL, scheme)
        sw_fills(bad, torch, ctx, alpha, flags, PANEL, scheme, PANEL_SHAPES, P)
        sw_fills(bad, torch, ctx, alpha, flags, TALL, scheme, [(4, 1), (1, 4)], P)
    report(bad)


# ------------------------------------------------------------------ the half-word shape
@pytest.mark.parametrize("scheme", SW_WIDE, ids=sid)
def test_half_word_fill_sw(torch, ctx, scheme):
    """(2, 4) at 600 x 200, two strips of 512 columns: every entry whose corner is empty; the one
    whose corner is 184 x 584 cells is refused."""
    cells, _ = sw_half_corner(scheme, *STRIP)
    assert (cells > HALF_FIX_MAX) == (scheme == (CAP, -CAP, -CAP))
    bad = []
    for alpha, flags in FORMS:
        check_sw(alpha, STRIP, scheme)
        if cells <= HALF_FIX_MAX:
            sw_fills(bad, torch, ctx, alpha, flags, STRIP, scheme, [(2, 4)], S)
            continue
        s1, s2 = pair(alpha, STRIP)
        tab = nwhip.Context.alloc_table(s1.size, s2.size)
        with pytest.raises(nwhip.NwError) as e:
            ctx.fill(dev(torch, s1), dev(torch, s2), tab, scheme, substrips=2, strip_waves=4, mode=nwhip.MODE_SW,
                     flags=flags)
        assert e.value.status == nwhip.NW_ERR_UNSUPPORTED
    report(bad)


def half_case(torch, ctx, s1, s2, scheme, shape):
    n1, n2 = s1.size, s2.size
    d1, d2 = dev(torch, s1), dev(torch, s2)
    tab = nwhip.Context.alloc_table(n1, n2)
    tab.fill_(POISON)
    r = ctx.fill(d1, d2, tab, scheme, substrips=shape[0], strip_waves=shape[1], mode=nwhip.MODE_SW)
    want = oracle.sw_fill(s1, s2, scheme)
    np.testing.assert_array_equal(tab[:n2 + 1, :n1 + 1].cpu().numpy(), want)
    best = oracle.sw_best(s1, s2, scheme)
    assert (r.score, r.end_i, r.end_j) == best
    al, ops = ctx.sw_traceback(d1, d2, tab, best[1:], scheme)
    wops, bi, bj = oracle.sw_traceback(s1, s2, want, best[1:], scheme)
    np.testing.assert_array_equal(ops, wops)
    assert (al.begin_i, al.begin_j, al.score) == (bi, bj, best[0])
    return r


def test_half_word_corner_of_64_cells(torch, ctx):
    """kHalfFixMax met at 64: 24 x 24 of one letter under (4095, -4095, -4095), K = 17, the corner
    8 x 8 cells, each at or beyond 2^16 -- accepted, and exact after the fix-up."""
    s1, s2, scheme = half_identical(24, 24)
    assert sw_half_corner(scheme, 24, 24) == (HALF_FIX_MAX, 17)
    assert (oracle.sw_fill(s1, s2, scheme)[17:, 17:] >= 65536).all()
    r = half_case(torch, ctx, s1, s2, scheme, (2, 4))
    assert (r.substrips, r.strip_waves, r.score) == (2, 4, 24 * CAP)


def test_half_word_corner_of_72_cells(torch, ctx):
    """25 x 24: 72 cells, refused; the automatic shape fills the same pair exactly."""
    s1, s2, scheme = half_identical(25, 24)
    assert sw_half_corner(scheme, 25, 24)[0] == 72
    tab = nwhip.Context.alloc_table(25, 24)
    with pytest.raises(nwhip.NwError) as e:
        ctx.fill(dev(torch, s1), dev(torch, s2), tab, scheme, substrips=2, strip_waves=4, mode=nwhip.MODE_SW)
    assert e.value.status == nwhip.NW_ERR_UNSUPPORTED
    r = half_case(torch, ctx, s1, s2, scheme, (0, 0))
    assert (r.substrips, r.strip_waves) != (2, 4)


def test_half_word_corner_from_the_mismatch(torch, ctx):
    """(3, 4095, -1) on letters that never match: the bound's max(match, mismatch).  The corner is
    the same 64 cells (with match alone there would be none), 25 x 25 is refused."""
    s1, s2, scheme = half_never_match(24)
    assert sw_half_corner(scheme, 24, 24) == (HALF_FIX_MAX, 17) and sw_half_corner((3, 3, -1), 24, 24)[0] == 0
    r = half_case(torch, ctx, s1, s2, scheme, (2, 4))
    assert r.score == 24 * CAP
    s1, s2, scheme = half_never_match(25)
    with pytest.raises(nwhip.NwError) as e:
        ctx.fill(dev(torch, s1), dev(torch, s2), nwhip.Context.alloc_table(25, 25), scheme, substrips=2, strip_waves=4,
                 mode=nwhip.MODE_SW)
    assert e.value.status == nwhip.NW_ERR_UNSUPPORTED


# ------------------------------------------------------------------ bands on one device
def band_rows(bad, lb, n1, want, what):
    for r, (rows, start) in enumerate(lb.layout):
        d = differs(lb.tables[r][:rows, :n1 + 1].cpu().numpy(), want[start:start + rows])
        if d:
            bad.append(f"{what}, band {r}: {d}")


@pytest.mark.parametrize("scheme", BAND_SCHEMES, ids=sid)
def test_row_bands(torch, scheme):
    """LocalBands, both kernel families: a band's last row leaves as w-form halo granules and is
    the next band's row 0."""
    bad = []
    for (n1, n2), nb in [(ROWS_A, 3), (ROWS_B, 4)]:
        for kernel in (S, P):
            lb = nw_bands.LocalBands(n1, n2, nb, kernel=kernel)
            try:
                for alpha, flags in FORMS:
                    check_nw(alpha, (n1, n2), scheme)
                    s1, s2 = pair(alpha, (n1, n2))
                    want = nw_table(alpha, (n1, n2), scheme)
                    for t in lb.tables:
                        t.fill_(POISON)
                    score = lb.fill(dev(torch, s1), dev(torch, s2), scheme, flags=flags)
                    what = f"{(n1, n2, nb)} kernel {kernel}, {alpha} letters, flags {flags}"
                    band_rows(bad, lb, n1, want, what)
                    if score != want[-1, -1]:
                        bad.append(f"{what}: score {score} for {want[-1, -1]}")
            finally:
                lb.close()
    report(bad)


@pytest.mark.parametrize("scheme", BAND_SCHEMES, ids=sid)
def test_column_bands(torch, scheme):
    """LocalColBands at 3000 x 300 in three bands: strips (2, 2) and (4, 1), panels (4, 1) and the
    automatic shape.  A band's local column 0 is rebuilt from the feed as w + gap (i + start)."""
    n1, n2 = COLS
    bad = []
    for kernel, sh in [(S, (2, 2)), (S, (4, 1)), (P, (4, 1)), (P, (0, 0))]:
        lb = nw_bands.LocalColBands(n1, n2, 3, substrips=sh[0], strip_waves=sh[1], kernel=kernel)
        try:
            assert len(lb.layout) == 3 and all(start > 0 for _, _, start, _ in lb.layout[1:])
            for alpha, flags in FORMS:
                check_nw(alpha, COLS, scheme)
                s1, s2 = pair(alpha, COLS)
                want = nw_table(alpha, COLS, scheme)
                for t in lb.tables:
                    t.fill_(POISON)
                score = lb.fill(dev(torch, s1), dev(torch, s2), scheme, flags=flags)
                what = f"kernel {kernel} shape {sh}, {alpha} letters, flags {flags}"
                for r, (_, _, start, ncols) in enumerate(lb.layout):
                    d = differs(lb.tables[r][:n2 + 1, :ncols].cpu().numpy(), want[:, start:start + ncols])
                    if d:
                        bad.append(f"{what}, band {r}: {d}")
                if score != want[-1, -1]:
                    bad.append(f"{what}: score {score} for {want[-1, -1]}")
        finally:
            lb.close()
    report(bad)


@pytest.mark.parametrize("scheme", BAND_SCHEMES, ids=sid)
def test_horizontal_strip_bands(torch, scheme):
    """LocalTBands: the strip kernel on the transposed band, its row 0 and column 0 from
    launch_tband_edges (gap (i + start))."""
    bad = []
    for (n1, n2), nb in [(ROWS_A, 3), (TB_B, 4)]:
        for sh in tt.SHAPES:
            tb = nw_bands.LocalTBands(n1, n2, nb, shape=sh)
            try:
                assert all(start > 0 for _, start in tb.layout[1:])
                for alpha, flags in FORMS:
                    check_nw(alpha, (n1, n2), scheme)
                    s1, s2 = pair(alpha, (n1, n2))
                    want = nw_table(alpha, (n1, n2), scheme)
                    for t in tb.tables:
                        t.fill_(POISON)
                    score = tb.fill(dev(torch, s1), dev(torch, s2), scheme, flags=flags)
                    what = f"{(n1, n2, nb)} shape {sh}, {alpha} letters, flags {flags}"
                    band_rows(bad, tb, n1, want, what)
                    if score != want[-1, -1]:
                        bad.append(f"{what}: score {score} for {want[-1, -1]}")
            finally:
                tb.close()
    report(bad)


@pytest.mark.parametrize("scheme", BAND_SCHEMES, ids=sid)
def test_finisher_rows(torch, scheme):
    """Two bands of 293 rows on one worker each: two strips, so the last 37 rows of each are the
    row-scan finisher's (its own (a == b ? match : mismatch) - 2 gap, w = t - gap (i + j) from the
    strips' last row and back), the second band below a halo; and the feed the first publishes."""
    n1, n2 = FINISH
    R = 256 + 37
    assert n2 == 2 * R + 1
    split = [(R + 1, 0), (R + 1, R)]
    bad = []
    for alpha, flags in FORMS:
        check_nw(alpha, FINISH, scheme)
        s1, s2 = (np.array(a) for a in pair(alpha, FINISH))  # (copies: the pairs are read-only)
        want = nw_table(alpha, FINISH, scheme)
        for sh in tt.SHAPES:
            what = f"shape {sh}, {alpha} letters, flags {flags}"
            tabs, pub = tt._tband_chain(torch, s1, s2, 2, scheme, 1, flags=flags, row_split=split, shape=sh)
            for r, (rows, start) in enumerate(split):
                d = differs(tabs[r], want[start:start + rows])
                if d:
                    bad.append(f"{what}, band {r}: {d}")
            vals = (pub[0] & 0xFFFFFFFF).astype(np.uint32).view(np.int32).astype(np.int64)
            d = differs(vals + scheme[2] * (np.arange(n1 + 1) + R), want[R].astype(np.int64))
            if d or not np.all((pub[0] >> 32) == 5):
                bad.append(f"{what}, feed: {d}")
    report(bad)


# ------------------------------------------------------------------ one context through the kinds
def test_one_context_through_the_kinds(torch):
    """One context, one pair (1100 x 130, 4 letters): the unit kind, the generic compares, tables,
    Smith-Waterman in both forms, the unit kind again, across strips and panels.  A launch that
    kept the previous scheme's table bytes, offset or kernel choice shows in the next table."""
    s1, s2 = pair(4, PANEL)
    n1, n2 = s1.size, s2.size
    d1, d2 = dev(torch, s1), dev(torch, s2)
    NW, SW = nwhip.MODE_NW, nwhip.MODE_SW
    steps = [("unit", (64, 63, -32), NW, S, (2, 2), 0), ("generic", (126, -1, -1), NW, P, (4, 4), 0),
             ("tables", (125, -1, -1), NW, S, (4, 1), 0), ("tables", (125, -1, -1), NW, P, (4, 1), 0),
             ("sw tables", (126, -1, -1), SW, P, (4, 4), 0), ("sw compares", (126, -1, -1), SW, S, (2, 2), 0),
             ("sw tables", (1, -130, -1), SW, S, (1, 4), 0), ("sw compares", (1, -130, -1), SW, P, (2, 4), 0),
             ("unit", (CAP, CAP - 1, -CAP), NW, S, (1, 2), 0), ("tables", (9, 8, 2), NW, P, (2, 2), 0),
             ("unit behind the flag", (9, 8, 2), NW, S, (2, 2), nwhip.FLAG_NO_PROFILE),
             ("sw zero", (-4000, -4095, -4095), SW, P, (4, 4), 0), ("unit", (64, 63, -32), NW, S, (2, 2), 0)]
    c = nwhip.Context(0)
    bad = []
    try:
        for name, scheme, mode, kernel, sh, flags in steps:
            (check_sw if mode == SW else check_nw)(4, PANEL, scheme)
            want = (sw_table if mode == SW else nw_table)(4, PANEL, scheme)
            tab = nwhip.Context.alloc_table(n1, n2)
            tab.fill_(POISON)
            r = c.fill(d1, d2, tab, scheme, substrips=sh[0], strip_waves=sh[1], mode=mode, kernel=kernel, flags=flags)
            assert r.status == 0 and (r.substrips, r.strip_waves, r.kernel) == (sh[0], sh[1], kernel)
            d = differs(tab[:n2 + 1, :n1 + 1].cpu().numpy(), want)
            if d:
                bad.append(f"{name} {scheme} kernel {kernel} {sh}: {d}")
            if mode == SW and (r.score, r.end_i, r.end_j) != oracle.sw_best(s1, s2, scheme):
                bad.append(f"{name} {scheme} kernel {kernel} {sh}: best cell {(r.score, r.end_i, r.end_j)}")
            if mode == NW and r.score != want[-1, -1]:
                bad.append(f"{name} {scheme} kernel {kernel} {sh}: score {r.score}")
    finally:
        c.close()
    report(bad)
