"""Global alignment with on-device traceback (nw_align / nw_traceback, nw_sw.hip's
global kind of the windowed traceback).

The checker is the plain Python walk of tests/nw_walk.py over oracle.fill: from
(n2, n1) to (0, 0), diag > up > left, forced moves along row 0 / column 0.  The
device ops must equal it exactly -- for every table base and fill kernel, for
narrow bands and short rounds (paths that leave the band, rounds that end in
mid-table), aimed at (0, 0) and on the diagonal.  References are computed once
per (shape, scheme) and shared.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import nwhip
import oracle
from conftest import ROOT, bdna_path
from nw_walk import walk

SCHEMES = [(1, 0, -1), (1, -1, -1), (2, -1, -2), (2, -1, 0)]
SHAPES = [(1, 1, 4), (1, 300, 4), (300, 1, 4), (63, 64, 4), (64, 64, 4), (65, 63, 4), (257, 513, 4),
          (1500, 1100, 4), (1000, 300, 20), (2000, 2000, 2)]


@functools.lru_cache(maxsize=None)
def case(n1, n2, alpha, scheme):
    """(s1, s2, the walk's ops) of the random pair of this shape (read-only)."""
    rng = np.random.default_rng(n1 + 7 * n2 + alpha)
    s1 = rng.integers(1, alpha + 1, n1).astype(np.int8)
    s2 = rng.integers(1, alpha + 1, n2).astype(np.int8)
    ops = walk(s1, s2, oracle.fill(s1, s2, scheme), scheme)
    for a in (s1, s2, ops):
        a.setflags(write=False)
    return s1, s2, ops


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


def aligned_table(torch, n1, n2):
    """A table on a 256-byte aligned base (the strips then sweep from column 0)."""
    rows, pitch = nwhip.table_rows(n2), nwhip.table_pitch(n1)
    flat = torch.empty(rows * pitch + 64, dtype=torch.int32, device="cuda")
    shift = (-(flat.data_ptr() // 4)) % 64
    return flat[shift:shift + rows * pitch].view(rows, pitch)


def check(al, ops, want, n1, n2, score=None):
    np.testing.assert_array_equal(ops, want)
    assert (al.begin_i, al.begin_j, al.end_i, al.end_j, al.n_ops) == (0, 0, n2, n1, len(want))
    if score is not None:
        assert al.score == score


def fill_and_trace(torch, ctx, n1, n2, alpha, scheme, tab=None, fill_kw=None, **tb_kw):
    s1, s2, want = case(n1, n2, alpha, scheme)
    d1, d2 = torch.from_numpy(s1.copy()).cuda(), torch.from_numpy(s2.copy()).cuda()
    if tab is None:
        tab = nwhip.Context.alloc_table(n1, n2)
    r = ctx.fill(d1, d2, tab, scheme, **(fill_kw or {}))
    al, ops, stats = ctx.traceback(d1, d2, tab, scheme, **tb_kw)
    check(al, ops, want, n1, n2, r.score)
    assert nwhip.ops_score(s1, s2, ops, scheme) == r.score
    return stats


# ------------------------------------------------------------------ 1. ops equal the walk's
@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n1,n2,alpha", SHAPES)
def test_traceback_vs_walk(torch, ctx, n1, n2, alpha, scheme):
    stats = fill_and_trace(torch, ctx, n1, n2, alpha, scheme)
    assert (stats.band, stats.max_windows) == (256, min(512, n2 // 64 + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n1,n2,alpha", [(257, 513, 4), (1500, 1100, 4)])
def test_traceback_aligned_base(torch, ctx, n1, n2, alpha, scheme):
    tab = aligned_table(torch, n1, n2)
    tab.fill_(-0x5A5A5A5)
    fill_and_trace(torch, ctx, n1, n2, alpha, scheme, tab=tab)


@pytest.mark.gpu
def test_traceback_of_a_panel_fill(torch, ctx):
    fill_and_trace(torch, ctx, 2049, 333, 4, (1, 0, -1),
                   fill_kw=dict(kernel=nwhip.KERNEL_PANELS, substrips=4, strip_waves=4))


# ------------------------------------------------------------------ 2. window geometry
@pytest.mark.gpu
@pytest.mark.parametrize("no_aim", [False, True])
@pytest.mark.parametrize("band,maxwin", [(1, 4096), (3, 1), (17, 3), (128, 2), (128, 4096)])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("n1,n2,alpha", [(1500, 1100, 4), (300, 1000, 4), (1000, 300, 20), (2000, 2000, 2)])
def test_traceback_window_geometry(torch, ctx, n1, n2, alpha, scheme, band, maxwin, no_aim):
    """Narrow bands and short rounds through nw_tb_opts: paths that leave the band,
    entries that the aim's step pushes out of it and rounds that end in mid-table
    restart re-centred; aimed or not, the ops are the walk's."""
    stats = fill_and_trace(torch, ctx, n1, n2, alpha, scheme, band=band, max_windows=maxwin, no_aim=no_aim)
    assert (stats.band, stats.max_windows) == (band, min(maxwin, n2 // 64 + 1))
    assert stats.rounds >= 1 and stats.windows >= stats.rounds


# ------------------------------------------------------------------ 3. aim
@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [20, 4])
def test_aim_follows_a_slope_2_path(torch, ctx, alpha):
    """s2 = every second character of s1: the path follows the line from (n2, n1) to
    (0, 0), slope 2.  Rounds aimed at (0, 0) keep it inside their 128-column band
    (the CPU model: 1 round); diagonal rounds lose it every two windows (8 rounds)."""
    n1, n2, scheme = 2000, 1000, (1, -1, -1)
    s1 = np.random.default_rng(n1 + 7 * n2 + alpha).integers(1, alpha + 1, n1).astype(np.int8)
    s2 = s1[::2].copy()
    want = walk(s1, s2, oracle.fill(s1, s2, scheme), scheme)
    d1, d2 = torch.from_numpy(s1).cuda(), torch.from_numpy(s2).cuda()
    tab = nwhip.Context.alloc_table(n1, n2)
    ctx.fill(d1, d2, tab, scheme)
    al, ops, aimed = ctx.traceback(d1, d2, tab, scheme, band=128, max_windows=4096)
    check(al, ops, want, n1, n2)
    al, ops, diagonal = ctx.traceback(d1, d2, tab, scheme, band=128, max_windows=4096, no_aim=True)
    check(al, ops, want, n1, n2)
    print(f"rounds: aimed {aimed.rounds} ({aimed.windows} windows), no_aim {diagonal.rounds} ({diagonal.windows})")
    assert aimed.rounds <= 2
    assert diagonal.rounds >= 4


@pytest.mark.gpu
def test_identical_square_is_one_round(torch, ctx):
    n, scheme = 2000, (1, 0, -1)
    s = np.random.default_rng(n).integers(1, 5, n).astype(np.int8)
    d = torch.from_numpy(s).cuda()
    tab = nwhip.Context.alloc_table(n, n)
    r = ctx.fill(d, d, tab, scheme)
    al, ops, stats = ctx.traceback(d, d, tab, scheme)
    assert (stats.rounds, stats.windows, stats.tail_ops) == (1, 32, 0)
    assert al.n_ops == n and not ops.any() and al.score == r.score == n


# ------------------------------------------------------------------ 4. nwhip.align
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "t", "debug", "smid"])
@pytest.mark.parametrize("scheme", [(1, 0, -1), (1, -1, -1), (2, -1, -2)])
def test_align_bdna(torch, pair, name, scheme):
    s1, s2 = pair(name)
    al, ops, _ = nwhip.align(s1, s2, scheme)
    assert al.score == oracle.score(s1, s2, scheme)
    assert nwhip.ops_score(s1, s2, ops, scheme) == al.score
    check(al, ops, walk(s1, s2, oracle.fill(s1, s2, scheme), scheme), s1.size, s2.size)


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", [(0, 5), (5, 0), (0, 0)])
def test_align_empty_sequences(torch, n1, n2):
    s1, s2 = np.arange(1, n1 + 1, dtype=np.int8), np.arange(1, n2 + 1, dtype=np.int8)
    al, ops, stats = nwhip.align(s1, s2, (1, 0, -3))
    check(al, ops, walk(s1, s2, None, (1, 0, -3)), n1, n2, -3 * max(n1, n2))
    assert stats.rounds == 0 and stats.tail_ops == max(n1, n2)


@pytest.mark.gpu
def test_align_default_geometry_16k(torch):
    n1, n2, scheme = 16384, 12288, (1, 0, -1)
    s1, s2 = nwhip.synth(1, n1), nwhip.synth(2, n2)
    t = oracle.fill(s1, s2, scheme)
    al, ops, stats = nwhip.align(s1, s2, scheme)
    check(al, ops, walk(s1, s2, t, scheme), n1, n2, int(t[n2, n1]))
    assert (stats.band, stats.max_windows) == (256, 193)


# ------------------------------------------------------------------ 5. corrupted table
@pytest.mark.gpu
def test_corrupted_table_is_reported(torch, ctx):
    n1, n2, scheme = 300, 200, (1, 0, -1)
    s1, s2, want = case(n1, n2, 4, scheme)
    d1, d2 = torch.from_numpy(s1.copy()).cuda(), torch.from_numpy(s2.copy()).cuda()
    tab = nwhip.Context.alloc_table(n1, n2)
    ctx.fill(d1, d2, tab, scheme)
    tab[n2, n1] += 1000
    with pytest.raises(nwhip.NwError) as e:
        ctx.traceback(d1, d2, tab, scheme)
    assert e.value.status == nwhip.NW_ERR_TABLE
    # a whole row in mid-table, met in a later round (one 64-row window per round)
    ctx.fill(d1, d2, tab, scheme)
    tab[100, :] += 1000
    with pytest.raises(nwhip.NwError) as e:
        ctx.traceback(d1, d2, tab, scheme, band=17, max_windows=1)
    assert e.value.status == nwhip.NW_ERR_TABLE
    # the context is still good
    r = ctx.fill(d1, d2, tab, scheme)
    al, ops, _ = ctx.traceback(d1, d2, tab, scheme)
    check(al, ops, want, n1, n2, r.score)


# ------------------------------------------------------------------ 6. stream
@pytest.mark.gpu
def test_fill_and_traceback_on_a_side_stream(torch, ctx):
    """Fill (launch only) and traceback on one non-default stream with no
    synchronisation between them: the traceback is ordered after the fill."""
    n1, n2, scheme = 1500, 1100, (1, -1, -1)
    s1, s2, want = case(n1, n2, 4, scheme)
    d1, d2 = torch.from_numpy(s1.copy()).cuda(), torch.from_numpy(s2.copy()).cuda()
    tab = nwhip.Context.alloc_table(n1, n2)
    tab.fill_(-0x5A5A5A5)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ctx.fill(d1, d2, tab, scheme, stream=side, sync=False)
    al, ops, _ = ctx.traceback(d1, d2, tab, scheme, stream=side)
    check(al, ops, want, n1, n2)
    assert ctx.status(side) == nwhip.NW_OK


# ------------------------------------------------------------------ 7. CLI
@pytest.mark.gpu
def test_cli_writes_gapped_rows(torch, pair, tmp_path):
    exe = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")
    o1, o2 = str(tmp_path / "a.bdna"), str(tmp_path / "b.bdna")
    r = subprocess.run([exe, bdna_path("small1.bdna"), bdna_path("small2.bdna"), o1, o2, "--scheme", "2,-1,-2"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m = re.fullmatch(r"(\d+)\nScore: (-?\d+)\n", r.stdout)
    assert m, r.stdout
    s1, s2 = pair("small")
    r1, r2 = np.fromfile(o1, dtype=np.int8), np.fromfile(o2, dtype=np.int8)
    assert r1.size == r2.size
    np.testing.assert_array_equal(r1[r1 != 0], s1)
    np.testing.assert_array_equal(r2[r2 != 0], s2)
    assert not np.any((r1 == 0) & (r2 == 0))
    cols = np.where((r1 == 0) | (r2 == 0), -2, np.where(r1 == r2, 2, -1))
    assert int(cols.sum()) == int(m.group(2)) == oracle.score(s1, s2, (2, -1, -2))


def test_cli_argument_errors():
    """Argument and missing-file errors are nw_driver's; no device needed."""
    exe = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")
    r = subprocess.run([exe, "only-one"], capture_output=True, text=True)
    assert r.returncode == 1 and "incorrect number of arguments" in r.stdout
    r = subprocess.run([exe, "a", "b", "c"], capture_output=True, text=True)
    assert r.returncode == 1 and "incorrect number of arguments" in r.stdout
    r = subprocess.run([exe, "/nonexistent/a", "/nonexistent/b"], capture_output=True, text=True)
    assert r.returncode == 1 and "ERROR: no such file /nonexistent/a" in r.stdout
    r = subprocess.run([exe, bdna_path("small1.bdna"), "/nonexistent/b"], capture_output=True, text=True)
    assert r.returncode == 1 and "ERROR: no such file /nonexistent/b" in r.stdout
    r = subprocess.run([exe, "a", "b", "--scheme", "1,2"], capture_output=True, text=True)
    assert r.returncode == 1 and "--scheme" in r.stdout
