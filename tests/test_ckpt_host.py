"""CPU: the host side of the checkpointed alignment (nw_ckpt_plan, nw_score,
nw_align_ckpt, nw_traceback_block, nw_ckpt_sweep_async; include/nw_hip.h).

The planner's rule over a grid of sizes and budgets, every argument refusal --
which the library checks before any HIP call, so it answers without a device --
the struct sizes, and tb_shift's row offset (with row0 = 0 today's values).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import nwhip
from conftest import ROOT

_i8p = ctypes.POINTER(ctypes.c_int8)
_u8p = ctypes.POINTER(ctypes.c_uint8)
GB = 10 ** 9
MiB = 1 << 20


def _gpu_visible():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ planner
def _plan(n1, n2, mem):
    st = nwhip.NwCkptStats()
    rc = nwhip.lib().nw_ckpt_plan(n1, n2, mem, ctypes.byref(st))
    return rc, st


def _min_budget(n1, n2):
    """The smallest budget the planner accepts (bisection on its status)."""
    lo, hi = 0, 1 << 50
    assert _plan(n1, n2, hi)[0] == nwhip.NW_OK
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _plan(n1, n2, mid)[0] == nwhip.NW_OK:
            hi = mid
        else:
            lo = mid
    return hi


PLAN_SIZES = [(524288, 524288), (1000, 700), (262144, 262144), (524288, 131072), (131072, 524288), (16384, 12288),
              (5, 300), (300, 5), (1, 1), (70000, 200), (63, 64), (64, 65)]
PLAN_BUDGETS = [230 * GB, 288 * GB, 32 * GB, GB, 100 * MiB, 16 * MiB, 12 * MiB, 11 * MiB, 10 * MiB, MiB, 4096, 0]


@pytest.mark.parametrize("n1,n2", PLAN_SIZES)
def test_planner_rule(n1, n2):
    need64 = _min_budget(n1, n2)
    kmax = max(64, ceil_div(n2, 64) * 64)
    seen_ok = seen_oom = False
    for mem in PLAN_BUDGETS + [need64, need64 - 1, need64 + 1, 2 * need64, 3 * need64]:
        rc, st = _plan(n1, n2, mem)
        if mem < need64:
            assert rc == nwhip.NW_ERR_OOM, (mem, need64)  # below the smallest need
            seen_oom = True
            continue
        seen_ok = True
        assert rc == nwhip.NW_OK
        K = st.block_rows
        assert K % 64 == 0 and 64 <= K <= kmax
        assert st.peak_bytes <= mem
        assert st.blocks == max(1, ceil_div(n2, K))
        assert st.ckpt_bytes == nwhip.ckpt_bytes(n1, n2, K) == (st.blocks - 1) * (n1 + 1) * 8
        assert st.block_bytes >= 4 * (min(K, n2) + 1) * (n1 + 1)
        assert st.peak_bytes >= st.block_bytes + st.ckpt_bytes + n1 + n2
        assert st.peak_bytes == nwhip.ckpt_peak_bytes(n1, n2, K)
        if K < kmax:
            # K + 64 does not fit, nor does any larger block (sampled up to the whole table)
            assert nwhip.ckpt_peak_bytes(n1, n2, K + 64) > mem
            for k2 in sorted({min(kmax, K + 64 * m) for m in (2, 3, 5, 17, 100, 1000)} | {kmax}):
                assert nwhip.ckpt_peak_bytes(n1, n2, k2) > mem, k2
        else:
            assert st.blocks == 1  # the whole table fits
    assert seen_ok and seen_oom
    # the smallest budget is the K = 64 need (or the whole table when n2 <= 64)
    rc, st = _plan(n1, n2, need64)
    assert rc == nwhip.NW_OK and st.peak_bytes == need64
    assert need64 == min(nwhip.ckpt_peak_bytes(n1, n2, k) for k in range(64, kmax + 1, 64)) or kmax > 64 * 4096
    assert need64 <= nwhip.ckpt_peak_bytes(n1, n2, 64)


def test_planner_named_cases():
    # the 1.1 TB table within 230 GB: a few blocks, linear memory
    rc, st = _plan(524288, 524288, 230 * GB)
    assert rc == nwhip.NW_OK and st.blocks >= 2 and st.block_rows % 64 == 0 and st.peak_bytes <= 230 * GB
    assert st.block_bytes + st.ckpt_bytes < 230 * GB and st.block_bytes > 100 * GB
    # 256k x 256k is the largest table that fits whole
    rc, st = _plan(262144, 262144, 288 * GB)
    assert rc == nwhip.NW_OK and st.blocks == 1
    # 1000 x 700 at 1 MB: below the workspace alone
    assert _plan(1000, 700, 10 ** 6)[0] == nwhip.NW_ERR_OOM
    rc, st = _plan(1000, 700, 12 * MiB)
    assert rc == nwhip.NW_OK and st.blocks >= 2
    # refused arguments
    for a in [(-1, 5, GB), (5, -1, GB), (5, 5, -1), (2 ** 31, 5, GB), (5, 2 ** 31, GB)]:
        assert _plan(*a)[0] == nwhip.NW_ERR_ARG
    assert nwhip.lib().nw_ckpt_plan(5, 5, GB, None) == nwhip.NW_ERR_ARG
    with pytest.raises(nwhip.NwError) as e:
        nwhip.ckpt_plan(1000, 700, 4096)
    assert e.value.status == nwhip.NW_ERR_OOM
    assert nwhip.ckpt_plan(1000, 700, GB).blocks == 1


def test_ckpt_bytes():
    assert nwhip.ckpt_bytes(1000, 700, 64) == 10 * 1001 * 8   # rows 64 .. 640
    assert nwhip.ckpt_bytes(1000, 640, 64) == 9 * 1001 * 8    # row 640 is the last row, not a checkpoint
    assert nwhip.ckpt_bytes(1000, 641, 64) == 10 * 1001 * 8
    assert nwhip.ckpt_bytes(1000, 64, 64) == 0 and nwhip.ckpt_bytes(1000, 5, 128) == 0
    assert nwhip.ckpt_bytes(1000, 700, 0) == 0 and nwhip.ckpt_bytes(-1, 700, 64) == 0


# ------------------------------------------------------------------ C ABI
def test_struct_sizes_match_the_header():
    assert ctypes.sizeof(nwhip.NwCkptOpts) == 32
    assert ctypes.sizeof(nwhip.NwCkptStats) == 80
    assert nwhip.CKPT_TAG == 1
    # the header's fields, in order, are the ctypes fields
    text = open(os.path.join(ROOT, "include", "nw_hip.h")).read()
    for name, cls in [("nw_ckpt_opts", nwhip.NwCkptOpts), ("nw_ckpt_stats", nwhip.NwCkptStats)]:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [re.sub(r"\[.*\]", "", f).strip() for f in decl.split(None, 1)[1].split(",")]
        assert fields == [f[0] for f in cls._fields_]
    assert re.search(r"#define NW_CKPT_TAG 1u", text)


# ------------------------------------------------------------------ refusals
def _seqs(n1, n2):
    return np.ones(max(n1, 1), np.int8), np.ones(max(n2, 1), np.int8)


def _score(n1, n2, p, s1="alloc", out="alloc"):
    a, b = _seqs(n1, n2)
    r = nwhip.NwResult()
    st = nwhip.lib().nw_score(a.ctypes.data_as(_i8p) if s1 == "alloc" else None, n1, b.ctypes.data_as(_i8p), n2,
                              ctypes.byref(p) if p is not None else None, ctypes.byref(r) if out == "alloc" else None)
    return st, r


def _align_ckpt(n1, n2, p, co=None, o=None, ops_cap=None, ops="alloc", out="alloc"):
    a, b = _seqs(n1, n2)
    buf = np.zeros(n1 + n2 + 1, np.uint8)
    al, stats = nwhip.NwAlignment(), nwhip.NwCkptStats()
    st = nwhip.lib().nw_align_ckpt(a.ctypes.data_as(_i8p), n1, b.ctypes.data_as(_i8p), n2,
                                   ctypes.byref(p) if p is not None else None,
                                   ctypes.byref(co) if co is not None else None,
                                   ctypes.byref(o) if o is not None else None,
                                   buf.ctypes.data_as(_u8p) if ops == "alloc" else None,
                                   n1 + n2 if ops_cap is None else ops_cap,
                                   ctypes.byref(al) if out == "alloc" else None, ctypes.byref(stats))
    return st, al, buf, stats


# what the sweep refuses (nw_score, nw_align_ckpt, nw_ckpt_sweep_async): status by case
SWEEP_REFUSALS = {
    "mode_sw": (dict(mode=nwhip.MODE_SW, scheme=(1, -1, -1)), nwhip.NW_ERR_ARG),
    "mode_unknown": (dict(mode=7), nwhip.NW_ERR_ARG),
    "timing_only": (dict(flags=nwhip.FLAG_TIMING_ONLY), nwhip.NW_ERR_ARG),
    "no_finish": (dict(flags=nwhip.FLAG_NO_FINISH), nwhip.NW_ERR_ARG),
    "debug_no_store": (dict(flags=nwhip.FLAG_TIMING_ONLY | nwhip.FLAG_DEBUG_NO_STORE), nwhip.NW_ERR_ARG),
    "debug_drain": (dict(flags=nwhip.FLAG_TIMING_ONLY | nwhip.FLAG_DEBUG_DRAIN), nwhip.NW_ERR_ARG),
    "debug_no_chain": (dict(flags=nwhip.FLAG_DEBUG_NO_CHAIN), nwhip.NW_ERR_ARG),
    "debug_stagger": (dict(flags=nwhip.FLAG_DEBUG_NO_CHAIN | nwhip.FLAG_DEBUG_STAGGER), nwhip.NW_ERR_ARG),
    "no_profile_and_more": (dict(flags=nwhip.FLAG_NO_PROFILE | nwhip.FLAG_NO_FINISH), nwhip.NW_ERR_ARG),
    "unknown_flag": (dict(flags=0x4000), nwhip.NW_ERR_ARG),
    "substrips_3": (dict(substrips=3), nwhip.NW_ERR_ARG),
    "timeout_neg": (dict(timeout_ms=-1), nwhip.NW_ERR_ARG),
    "score_too_large": (dict(scheme=(5000, 0, -1)), nwhip.NW_ERR_ARG),
    "kernel_unknown": (dict(kernel=9), nwhip.NW_ERR_ARG),
    "panels": (dict(kernel=nwhip.KERNEL_PANELS), nwhip.NW_ERR_UNSUPPORTED),
}


@pytest.mark.parametrize("case", sorted(SWEEP_REFUSALS))
def test_sweep_refusals_need_no_device(case):
    kw, want = SWEEP_REFUSALS[case]
    p = nwhip.params(**kw)
    assert _score(4, 3, p)[0] == want
    assert _align_ckpt(4, 3, p)[0] == want
    assert _align_ckpt(400, 300, p, nwhip.NwCkptOpts(64, 0))[0] == want
    st = nwhip.lib().nw_ckpt_sweep_async(None, None, 4, None, 3, ctypes.byref(p), 64, None, None, None)
    assert st == want


def test_range_refusals_need_no_device():
    """w_range_ok: (max|score| + |gap|) * (n1 + n2 + 2) must stay below 2^28."""
    p = nwhip.params((4000, 0, -4000))
    a = np.ones(1, np.int8)
    r = nwhip.NwResult()
    n = 20000  # 8000 * 40002 > 2^28; the buffers are never read
    st = nwhip.lib().nw_score(a.ctypes.data_as(_i8p), n, a.ctypes.data_as(_i8p), n, ctypes.byref(p), ctypes.byref(r))
    assert st == nwhip.NW_ERR_ARG
    st = nwhip.lib().nw_ckpt_sweep_async(None, None, n, None, n, ctypes.byref(p), 64, None, None, None)
    assert st == nwhip.NW_ERR_ARG
    p = nwhip.params()
    for n1, n2 in [(-1, 3), (3, -1), (2 ** 31 - 1, 3), (3, 2 ** 31 - 1)]:
        st = nwhip.lib().nw_score(a.ctypes.data_as(_i8p), n1, a.ctypes.data_as(_i8p), n2, ctypes.byref(p),
                                  ctypes.byref(r))
        assert st == nwhip.NW_ERR_ARG
        st = nwhip.lib().nw_ckpt_sweep_async(None, None, n1, None, n2, ctypes.byref(p), 64, None, None, None)
        assert st == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("K", [0, -64, 1, 63, 65, 100, 32])
def test_block_rows_refusals(K):
    p = nwhip.params()
    st = nwhip.lib().nw_ckpt_sweep_async(None, None, 400, None, 300, ctypes.byref(p), K, None, None, None)
    assert st == nwhip.NW_ERR_ARG
    if K != 0:  # (0 = planned)
        assert _align_ckpt(400, 300, p, nwhip.NwCkptOpts(K, 0))[0] == nwhip.NW_ERR_ARG


def test_sweep_async_refuses_null_and_empty():
    """Valid parameters, but no context / buffers, or a table with no cells."""
    p = nwhip.params()
    f = nwhip.lib().nw_ckpt_sweep_async
    assert f(None, None, 400, None, 300, ctypes.byref(p), 64, None, None, None) == nwhip.NW_ERR_ARG
    assert f(None, None, 0, None, 300, ctypes.byref(p), 64, None, None, None) == nwhip.NW_ERR_ARG
    assert f(None, None, 400, None, 0, ctypes.byref(p), 64, None, None, None) == nwhip.NW_ERR_ARG
    assert f(None, None, 400, None, 300, None, 64, None, None, None) == nwhip.NW_ERR_ARG


ALIGN_REFUSALS = {
    "ops_cap": dict(ops_cap=6),
    "ops_null": dict(ops=None),
    "out_null": dict(out=None),
    "band_neg": dict(o=(-1, 0, 0, 0)),
    "band_257": dict(o=(257, 0, 0, 0)),
    "max_windows_neg": dict(o=(0, -1, 0, 0)),
    "tb_flags_unknown": dict(o=(0, 0, 2, 0)),
    "tb_reserved": dict(o=(0, 0, 0, 1)),
    "mem_neg": dict(co=(0, -1)),
    "block_rows_neg": dict(co=(-64, 0)),
    "block_rows_odd": dict(co=(96, 0)),
    "ckpt_reserved0": dict(co=(0, 0, (1, 0, 0, 0))),
    "ckpt_reserved3": dict(co=(64, 0, (0, 0, 0, 1))),
}


@pytest.mark.parametrize("case", sorted(ALIGN_REFUSALS))
def test_align_ckpt_refusals_need_no_device(case):
    kw = dict(ALIGN_REFUSALS[case])
    o = nwhip.NwTbOpts(*kw.pop("o")) if "o" in kw else None
    co = None
    if "co" in kw:
        c = kw.pop("co")
        co = nwhip.NwCkptOpts(c[0], c[1], (ctypes.c_int32 * 4)(*c[2])) if len(c) > 2 else nwhip.NwCkptOpts(c[0], c[1])
    st, _, _, _ = _align_ckpt(4, 3, nwhip.params(), co, o, **kw)
    assert st == nwhip.NW_ERR_ARG


def test_score_refusals_need_no_device():
    p = nwhip.params()
    assert _score(4, 3, p, out=None)[0] == nwhip.NW_ERR_ARG
    assert _score(4, 3, p, s1=None)[0] == nwhip.NW_ERR_ARG


def test_traceback_block_refusals_need_no_context():
    """nw_traceback_block makes nw_traceback's refusals before it touches its context."""
    out = nwhip.NwAlignment()
    buf = np.zeros(8, np.uint8)
    f = nwhip.lib().nw_traceback_block
    cases = [(nwhip.params(mode=nwhip.MODE_SW, scheme=(1, -1, -1)), None, 7, 64),
             (nwhip.params(), nwhip.NwTbOpts(300, 0, 0, 0), 7, 64),
             (nwhip.params(), nwhip.NwTbOpts(0, -1, 0, 0), 7, 64),
             (nwhip.params(), nwhip.NwTbOpts(0, 0, 2, 0), 7, 64),
             (nwhip.params(), nwhip.NwTbOpts(0, 0, 0, 1), 7, 64),
             (nwhip.params(), None, 6, 64),                                 # ops_cap < n1 + rows
             (nwhip.params(flags=nwhip.FLAG_TIMING_ONLY), None, 7, 64),
             (nwhip.params(flags=nwhip.FLAG_DEBUG_NO_CHAIN), None, 7, 64),
             (nwhip.params(), None, 7, -64),                                # row0 < 0
             (nwhip.params(), None, 7, 2 ** 31),                            # row0 + rows beyond int32
             (nwhip.params(), None, 7, 64)]                                 # valid, but no context / table
    for p, o, cap, row0 in cases:
        st = f(None, None, 4, None, 3, row0, ctypes.byref(p), None, 64, ctypes.byref(o) if o is not None else None,
               None, buf.ctypes.data_as(_u8p), cap, ctypes.byref(out), None)
        assert st == nwhip.NW_ERR_ARG
    st = f(None, None, 4, None, 3, 64, ctypes.byref(nwhip.params()), None, 64, None, None, None, 7,
           ctypes.byref(out), None)
    assert st == nwhip.NW_ERR_ARG  # ops == NULL
    st = f(None, None, 4, None, 3, 64, ctypes.byref(nwhip.params()), None, 64, None, None, buf.ctypes.data_as(_u8p), 7,
           None, None)
    assert st == nwhip.NW_ERR_ARG  # out == NULL


@pytest.mark.parametrize("n1,n2", [(4, 3), (0, 5), (5, 0), (0, 0), (300, 200)])
@pytest.mark.parametrize("defaults", [True, False])
def test_valid_arguments_reach_the_device(n1, n2, defaults):
    """Valid arguments (also p == NULL, NULL options, NO_PROFILE, empty sequences) pass
    the checks: NW_ERR_NODEVICE on a host without a GPU, never a host-computed answer."""
    p = None if defaults else nwhip.params((2, -1, -2), flags=nwhip.FLAG_NO_PROFILE)
    co = None if defaults else nwhip.NwCkptOpts(64, 0)
    o = None if defaults else nwhip.NwTbOpts(256, 1, nwhip.TB_NO_AIM, 0)
    st_s, r = _score(n1, n2, p)
    st_a, al, buf, stats = _align_ckpt(n1, n2, p, co, o)
    if not _gpu_visible():
        assert st_s == nwhip.NW_ERR_NODEVICE and st_a == nwhip.NW_ERR_NODEVICE
        return
    assert st_s == nwhip.NW_OK and st_a == nwhip.NW_OK
    gap = -1 if defaults else -2
    assert r.score == al.score and r.table_bytes == 0 and r.cells == n1 * n2
    if n1 == 0 or n2 == 0:
        n = max(n1, n2)
        assert (al.score, al.n_ops, al.end_i, al.end_j, al.begin_i, al.begin_j) == (gap * n, n, n2, n1, 0, 0)
        assert buf[:n].tolist() == [1 if n2 else 2] * n and stats.blocks == 1


# ------------------------------------------------------------------ tb_shift
def _shift_today(k, i_s, j_s, B, aim):
    """tb_shift as it stood before the row offset (csrc/nw_sw.hip), in Python; C++
    integer division truncates toward zero."""
    if not aim:
        return 0
    num, lim = j_s - i_s, B // 2
    if 64 * abs(num) > lim * i_s:
        return (-k if num < 0 else k) * lim
    q = abs(k * 64 * num) // i_s
    return q if num >= 0 else -q


def test_tb_shift_row_offset():
    f = nwhip.lib().nw_debug_tb_shift
    rng = np.random.default_rng(3)
    cases = [(k, i_s, j_s, B) for k in (0, 1, 2, 7, 511) for i_s in (1, 63, 64, 1000, 524288)
             for j_s in (0, 1, 999, 1000, 1001, 70000, 524288) for B in (1, 3, 17, 256)]
    cases += [(int(rng.integers(0, 600)), int(rng.integers(1, 1 << 20)), int(rng.integers(0, 1 << 20)),
               int(rng.integers(1, 257))) for _ in range(2000)]
    for k, i_s, j_s, B in cases:
        for aim in (0, 1):
            # row0 = 0: today's values, for every argument
            assert f(k, i_s, j_s, B, aim, 0) == _shift_today(k, i_s, j_s, B, aim)
            # a block's round from local (is, js) is the whole table's from (row0 + is, js)
            for row0 in (64, 4096, 1 << 19):
                assert f(k, i_s, j_s, B, aim, row0) == _shift_today(k, i_s + row0, j_s, B, aim)
    # the line from (row0 + is, js) to (0, 0): one window up, it moved 64 * js / (row0 + is) columns
    assert f(1, 64, 3000, 256, 1, 2936) == 64 * (3000 - 3000) // 3000 == 0
    assert f(4, 100, 1500, 256, 1, 2900) == 4 * 64 * (1500 - 3000) // 3000 == -128
