"""The windowed traceback (nw_tb_windows / nw_tb_chain / nw_tb_emit, run_traceback;
csrc/nw_sw.hip) over the SHAPE of the path, in its three kinds: global (nw_traceback),
local (nw_sw_traceback) and block (nw_traceback_block, nw_align_ckpt).

The cases are tests/test_path_geometry_host.py's: runs of hundreds of lefts and ups, a
window holding all the moves a window can, paths along row 0, column 0 and column n1, one
round of 66 windows.  Every comparison is exact: the ops against the plain walks, and the
work done -- rounds, windows launched, tail ops -- against tests/nw_windows.py's
rounds_model, which restates run_traceback from the checker's ops alone.  Each test
asserts its case's conditions from checker and model before it looks at the device.
"""
import re

import numpy as np
import pytest

import nwhip
import oracle
import test_path_geometry_host as h
from nw_windows import cells


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
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def same_stats(stats, m, band, max_windows):
    got = (stats.rounds, stats.windows, stats.tail_ops, stats.band, stats.max_windows)
    assert got == (m.rounds, m.windows, m.tail_ops, band, max_windows), (got, m[:3])


# ------------------------------------------------------------------ 1. global
@pytest.mark.gpu
@pytest.mark.parametrize("geom", list(h.GEOMS))
@pytest.mark.parametrize("name", h.GLOBAL_CASES)
def test_global_path(torch, ctx, name, geom):
    assert h.conditions(name)
    s1, s2, want, score = h.case(name)
    n1, n2 = s1.size, s2.size
    scheme = h.CASES[name][1]
    band, maxwin, no_aim = h.GEOMS[geom]
    m = h.model(name, geom)
    d1, d2 = dev(torch, s1), dev(torch, s2)
    tab = nwhip.Context.alloc_table(n1, n2)
    r = ctx.fill(d1, d2, tab, scheme)
    assert r.score == score
    al, ops, stats = ctx.traceback(d1, d2, tab, scheme, band=band, max_windows=maxwin, no_aim=no_aim)
    np.testing.assert_array_equal(ops, want)
    assert (al.begin_i, al.begin_j, al.end_i, al.end_j, al.n_ops, al.score) == (0, 0, n2, n1, want.size, score)
    assert nwhip.ops_score(s1, s2, ops, scheme) == score
    same_stats(stats, m, band, min(maxwin, n2 // 64 + 1))


# ------------------------------------------------------------------ 2. local
DEBUG_LINE = re.compile(r"nw_sw_traceback: (\d+) moves, (\d+) rounds, (\d+) windows \(band (\d+)\)")


@pytest.mark.gpu
@pytest.mark.parametrize("geom", list(h.LOCAL_GEOMS))
@pytest.mark.parametrize("name", sorted(h.LOCAL_CASES))
def test_local_path(torch, ctx, monkeypatch, capfd, name, geom):
    assert h.local_conditions(name)
    s1, s2, want, begin, end, score = h.local_case(name)
    scheme = h.LOCAL_CASES[name][1]
    band, maxwin = h.LOCAL_GEOMS[geom]
    m = h.local_model(name, geom)
    if geom == "default":
        monkeypatch.delenv("NW_TB_BAND", raising=False)
        monkeypatch.delenv("NW_TB_MAXWIN", raising=False)
    else:
        monkeypatch.setenv("NW_TB_BAND", str(band))
        monkeypatch.setenv("NW_TB_MAXWIN", str(maxwin))
    monkeypatch.setenv("NW_TB_DEBUG", "1")
    d1, d2 = dev(torch, s1), dev(torch, s2)
    tab = nwhip.Context.alloc_table(s1.size, s2.size)
    r = ctx.fill(d1, d2, tab, scheme, mode=nwhip.MODE_SW)
    assert (r.score, r.end_i, r.end_j) == (score, *end)
    capfd.readouterr()
    al, ops = ctx.sw_traceback(d1, d2, tab, end, scheme)
    err = capfd.readouterr().err
    np.testing.assert_array_equal(ops, want)
    assert (al.begin_i, al.begin_j, al.end_i, al.end_j, al.score, al.n_ops) == (*begin, *end, score, want.size)
    lines = DEBUG_LINE.findall(err)
    assert len(lines) == 1, err
    assert tuple(map(int, lines[0])) == (want.size, m.rounds, m.windows, band)


# ------------------------------------------------------------------ 3. block
@pytest.mark.gpu
@pytest.mark.parametrize("no_aim", [False, True])
@pytest.mark.parametrize("name", sorted(h.ALONE))
def test_block_alone(torch, ctx, name, no_aim):
    """One block from row0 = 640 to the table's last row, filled from the oracle's row 640:
    its ops are the walk's from where the walk leaves row 640, and its rounds aim along the
    line of the whole table."""
    s1, s2, want, score = h.case(name)
    scheme = h.CASES[name][1]
    n1 = s1.size
    row0, rows = h.ALONE[name]
    i, j = cells(want)
    lo = int(np.flatnonzero(i == row0)[-1])
    m = h.block_model(want, (1, row0, rows, n1, lo, want.size), 256, 512, not no_aim)
    t0 = oracle.rows(s1, s2, scheme, [row0])[0]
    d1, d2 = dev(torch, s1), dev(torch, s2[row0:])
    halo = torch.from_numpy((np.int64(nwhip.CKPT_TAG) << 32) | (t0.astype(np.int64) & 0xFFFFFFFF)).cuda()
    tab = nwhip.Context.alloc_table(n1, rows)
    tab.fill_(-0x5A5A5A5)
    ctx.fill_band(d1, d2, tab, halo_in=halo, tag=nwhip.CKPT_TAG, scheme=scheme, row0=row0)
    al, ops, stats = ctx.traceback_block(d1, d2, tab, row0, scheme, no_aim=no_aim)
    np.testing.assert_array_equal(ops, want[lo:])
    assert (al.begin_i, al.begin_j, al.end_i, al.end_j) == (row0, int(j[lo]), row0 + rows, n1)
    assert al.score == score and al.n_ops == want.size - lo
    same_stats(stats, m, 256, min(512, rows // 64 + 1))
    assert ctx.status() == nwhip.NW_OK


@pytest.mark.gpu
@pytest.mark.parametrize("K", h.BLOCK_ROWS)
@pytest.mark.parametrize("name", h.BLOCK_CASES)
def test_align_ckpt_path(torch, name, K):
    assert h.block_conditions(name, K)
    s1, s2, want, score = h.case(name)
    scheme = h.CASES[name][1]
    al, ops, stats = nwhip.align_ckpt(s1, s2, scheme, block_rows=K)
    np.testing.assert_array_equal(ops, want)
    assert (al.begin_i, al.begin_j, al.end_i, al.end_j, al.n_ops) == (0, 0, s2.size, s1.size, want.size)
    assert al.score == score == nwhip.ops_score(s1, s2, ops, scheme)
    assert (stats.blocks, stats.block_rows) == (-(-s2.size // K), K)
    assert (stats.rounds, stats.windows) == h.ckpt_model(name, K)
