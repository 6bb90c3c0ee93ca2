"""CPU: the host side of the batched alignment (nw_score_batch, nw_align_batch,
nw_score_batch_async, nw_batch_dir_bytes; include/nw_hip.h).

Every argument refusal -- which the library checks before any HIP call, so it
answers without a device -- in its order (NW_ERR_ARG, then NW_ERR_UNSUPPORTED, then
NW_ERR_NODEVICE), the direction-byte count and the struct sizes.
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
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)


def _gpu_visible():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


# the status of a call whose arguments are all valid
VALID = (nwhip.NW_OK,) if _gpu_visible() else (nwhip.NW_ERR_NODEVICE,)


class Call:
    """A three-pair batch (4 x 3, 0 x 2, 5 x 5) whose pieces a case replaces."""

    def __init__(self):
        self.off1 = np.array([0, 4, 4, 9], np.int64)
        self.off2 = np.array([0, 3, 5, 10], np.int64)
        self.s1 = np.ones(9, np.int8)
        self.s2 = np.ones(10, np.int8)
        self.npairs = 3
        self.p = nwhip.params()
        self.o = None
        self.scores = np.zeros(3, np.int32)
        self.ops_off = np.array([0, 7, 9, 19], np.int64)
        self.ops = np.zeros(19, np.uint8)
        self.n_ops = np.zeros(3, np.int64)
        self.null = set()

    def _ptr(self, name, arr, t):
        return None if name in self.null else arr.ctypes.data_as(t)

    def score(self):
        return nwhip.lib().nw_score_batch(
            self._ptr("s1", self.s1, _i8p), self._ptr("off1", self.off1, _i64p), self._ptr("s2", self.s2, _i8p),
            self._ptr("off2", self.off2, _i64p), self.npairs, ctypes.byref(self.p) if self.p is not None else None,
            self._ptr("scores", self.scores, _i32p), None)

    def align(self):
        return nwhip.lib().nw_align_batch(
            self._ptr("s1", self.s1, _i8p), self._ptr("off1", self.off1, _i64p), self._ptr("s2", self.s2, _i8p),
            self._ptr("off2", self.off2, _i64p), self.npairs, ctypes.byref(self.p) if self.p is not None else None,
            ctypes.byref(self.o) if self.o is not None else None, self._ptr("scores", self.scores, _i32p),
            self._ptr("ops", self.ops, _u8p), self._ptr("ops_off", self.ops_off, _i64p),
            self._ptr("n_ops", self.n_ops, _i64p), None)

    def score_async(self):
        """Device pointers are never read before the refusals: host addresses stand in."""
        return nwhip.lib().nw_score_batch_async(
            None, self.s1.ctypes.data, self.off1.ctypes.data, self.s2.ctypes.data, self.off2.ctypes.data,
            self.npairs, int(self.off1[-1]), int(self.off2[-1]), 5,
            ctypes.byref(self.p) if self.p is not None else None, self.scores.ctypes.data, None)


# nw_params every batch entry refuses: status by case (the sweep's refusals)
PARAM_REFUSALS = {
    "mode_sw": (dict(mode=nwhip.MODE_SW, scheme=(1, -1, -1)), nwhip.NW_ERR_ARG),
    "mode_unknown": (dict(mode=7), nwhip.NW_ERR_ARG),
    "timing_only": (dict(flags=nwhip.FLAG_TIMING_ONLY), nwhip.NW_ERR_ARG),
    "no_finish": (dict(flags=nwhip.FLAG_NO_FINISH), nwhip.NW_ERR_ARG),
    "debug_no_chain": (dict(flags=nwhip.FLAG_DEBUG_NO_CHAIN), nwhip.NW_ERR_ARG),
    "no_profile_and_more": (dict(flags=nwhip.FLAG_NO_PROFILE | nwhip.FLAG_NO_FINISH), nwhip.NW_ERR_ARG),
    "unknown_flag": (dict(flags=0x4000), nwhip.NW_ERR_ARG),
    "substrips_3": (dict(substrips=3), nwhip.NW_ERR_ARG),
    "timeout_neg": (dict(timeout_ms=-1), nwhip.NW_ERR_ARG),
    "score_too_large": (dict(scheme=(5000, 0, -1)), nwhip.NW_ERR_ARG),
    "kernel_unknown": (dict(kernel=9), nwhip.NW_ERR_ARG),
    "panels": (dict(kernel=nwhip.KERNEL_PANELS), nwhip.NW_ERR_UNSUPPORTED),
}


@pytest.mark.parametrize("case", sorted(PARAM_REFUSALS))
def test_param_refusals_need_no_device(case):
    kw, want = PARAM_REFUSALS[case]
    c = Call()
    c.p = nwhip.params(**kw)
    assert c.score() == want
    assert c.align() == want
    assert c.score_async() == want


def _neg_pairs(c):
    c.npairs = -1


def _off1_start(c):
    c.off1[0] = 1


def _off2_start(c):
    c.off2[0] = 2


def _off1_decreasing(c):
    c.off1[:] = [0, 4, 3, 9]


def _off2_decreasing(c):
    c.off2[:] = [0, 6, 5, 10]


def _range(c):
    # w_range_ok: (max|score| + |gap|) * (n1 + n2 + 2) must stay below 2^28 -- 8000 * 40002 is not;
    # the sequences are never read
    c.p = nwhip.params((4000, 0, -4000))
    c.off1[:] = [0, 4, 4, 20004]
    c.off2[:] = [0, 3, 5, 20005]
    c.ops_off[:] = [0, 7, 9, 9 + 40000]


def _pair_too_long(c):
    c.off1[:] = [0, 4, 4, 4 + 2 ** 31]
    c.ops_off[:] = [0, 7, 9, 9 + 2 ** 31 + 5]


ARG_REFUSALS = {
    "npairs_neg": _neg_pairs,
    "off1_start": _off1_start,
    "off2_start": _off2_start,
    "off1_decreasing": _off1_decreasing,
    "off2_decreasing": _off2_decreasing,
    "w_range": _range,
    "pair_too_long": _pair_too_long,
    "null_off1": lambda c: c.null.add("off1"),
    "null_off2": lambda c: c.null.add("off2"),
    "null_s1": lambda c: c.null.add("s1"),
    "null_s2": lambda c: c.null.add("s2"),
    "null_scores": lambda c: c.null.add("scores"),
}


@pytest.mark.parametrize("case", sorted(ARG_REFUSALS))
def test_batch_refusals_need_no_device(case):
    c = Call()
    ARG_REFUSALS[case](c)
    assert c.score() == nwhip.NW_ERR_ARG
    assert c.align() == nwhip.NW_ERR_ARG
    # an argument error comes before NW_KERNEL_PANELS' NW_ERR_UNSUPPORTED
    if case != "w_range":
        c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
        assert c.score() == nwhip.NW_ERR_ARG
        assert c.align() == nwhip.NW_ERR_ARG


def _slot_short(c):
    c.ops_off[:] = [0, 6, 8, 18]   # pair 0 needs 4 + 3


def _slot_short_last(c):
    c.ops_off[:] = [0, 7, 9, 18]   # pair 2 needs 5 + 5


def _slot_decreasing(c):
    c.ops_off[:] = [0, 9, 7, 19]


def _mem_neg(c):
    c.o = nwhip.NwBatchOpts(-1)


def _reserved(k):
    def f(c):
        r = [0] * 6
        r[k] = 1
        c.o = nwhip.NwBatchOpts(0, (ctypes.c_int32 * 6)(*r))
    return f


ALIGN_REFUSALS = {
    "slot_short": _slot_short,
    "slot_short_last": _slot_short_last,
    "slot_decreasing": _slot_decreasing,
    "mem_neg": _mem_neg,
    "reserved0": _reserved(0),
    "reserved5": _reserved(5),
    "null_ops": lambda c: c.null.add("ops"),
    "null_ops_off": lambda c: c.null.add("ops_off"),
    "null_n_ops": lambda c: c.null.add("n_ops"),
}


@pytest.mark.parametrize("case", sorted(ALIGN_REFUSALS))
def test_align_batch_refusals_need_no_device(case):
    c = Call()
    ALIGN_REFUSALS[case](c)
    assert c.align() == nwhip.NW_ERR_ARG


def test_async_refusals_need_no_device():
    c = Call()
    f = nwhip.lib().nw_score_batch_async
    a = (c.s1.ctypes.data, c.off1.ctypes.data, c.s2.ctypes.data, c.off2.ctypes.data)
    p = ctypes.byref(c.p)
    sc = c.scores.ctypes.data
    assert f(None, *a, -1, 9, 10, 5, p, sc, None) == nwhip.NW_ERR_ARG    # npairs < 0
    assert f(None, *a, 3, -1, 10, 5, p, sc, None) == nwhip.NW_ERR_ARG    # total1 < 0
    assert f(None, *a, 3, 9, -1, 5, p, sc, None) == nwhip.NW_ERR_ARG     # total2 < 0
    assert f(None, *a, 3, 9, 10, -1, p, sc, None) == nwhip.NW_ERR_ARG    # max_n2 < 0
    assert f(None, *a, 3, 9, 10, 11, p, sc, None) == nwhip.NW_ERR_ARG    # max_n2 > total2
    assert f(None, *a, 3, 9, 10, 5, None, sc, None) == nwhip.NW_ERR_ARG  # p == NULL
    assert f(None, *a, 3, 9, 10, 5, p, sc, None) == nwhip.NW_ERR_ARG     # valid, but no context
    big = nwhip.params((4000, 0, -4000))
    assert f(None, *a, 3, 9, 40000, 40000, ctypes.byref(big), sc, None) == nwhip.NW_ERR_ARG  # w range of max_n2


@pytest.mark.parametrize("defaults", [True, False])
def test_valid_arguments_reach_the_device(defaults):
    """Valid arguments (also p == NULL, NULL options, NO_PROFILE, empty pairs, an empty
    batch) pass the checks: NW_ERR_NODEVICE on a host without a GPU, never a host-computed
    answer -- nw_score's order."""
    c = Call()
    if defaults:
        c.p = None
    else:
        c.p = nwhip.params((2, -1, -2), flags=nwhip.FLAG_NO_PROFILE, waves=3)
        c.o = nwhip.NwBatchOpts(1 << 30)
    assert c.score() in VALID
    assert c.align() in VALID
    c.npairs = 0
    assert c.score() in VALID
    assert c.align() in VALID
    c.null = {"s1", "s2", "off1", "off2", "scores", "ops", "ops_off", "n_ops"}  # npairs = 0: nothing is read
    assert c.score() in VALID
    assert c.align() in VALID
    # only empty pairs: the concatenations may be NULL
    c = Call()
    c.off1[:] = 0
    c.off2[:] = [0, 3, 5, 10]
    c.null = {"s1"}
    assert c.score() in VALID
    assert c.align() in VALID


def test_dir_bytes():
    f = nwhip.batch_dir_bytes
    # an empty side: no cells; negative sizes: -1
    assert f(0, 7) == 0 and f(7, 0) == 0 and f(0, 0) == 0
    assert f(-1, 7) == -1 and f(7, -1) == -1 and f(-1, -1) == -1 and f(-1, 0) == -1
    # whole 64-step iterations (n2 / 64 + 2 of them) of whole 256-column strips, 4096 bytes each
    assert f(1, 1) == 2 * 4096
    assert f(256, 63) == 2 * 4096 and f(257, 63) == 2 * 2 * 4096
    assert f(256, 64) == 3 * 4096 and f(513, 130) == 3 * 4 * 4096
    rng = np.random.default_rng(5)
    sizes = [(1, 1), (3, 1), (255, 64), (256, 65), (257, 130), (600, 200), (1500, 1100), (4096, 4096), (8000, 8000)]
    sizes += [(int(a), int(b)) for a, b in rng.integers(1, 20000, (200, 2))]
    for n1, n2 in sizes:
        got = f(n1, n2)
        assert got >= (n1 * n2 + 3) // 4, (n1, n2)
        assert got % 4096 == 0
        assert got == -(-n1 // 256) * (n2 // 64 + 2) * 4096
    # the padding of a 4096 x 4096 pair: 16 strips x 66 iterations x 64 steps x 64 B = 1.03 x
    assert f(4096, 4096) == 16 * 66 * 4096
    assert f(4096, 4096) <= 1.1 * 4096 * 4096 / 4


def test_struct_sizes_match_the_header():
    assert ctypes.sizeof(nwhip.NwBatchOpts) == 32
    assert ctypes.sizeof(nwhip.NwBatchStats) == 64
    # the header's fields, in order, are the ctypes fields
    text = open(os.path.join(ROOT, "include", "nw_hip.h")).read()
    for name, cls in [("nw_batch_opts", nwhip.NwBatchOpts), ("nw_batch_stats", nwhip.NwBatchStats)]:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [re.sub(r"\[.*\]", "", f).strip() for f in decl.split(None, 1)[1].split(",")]
        assert fields == [f[0] for f in cls._fields_]
    # a C compiler's view of the two sizes
    assert re.search(r"int32_t reserved\[6\];", text)


def test_python_wrappers_build_the_csr_arrays():
    s1, off1, s2, off2 = nwhip.batch_csr([([1, 2, 3], [4]), ([], [1, 1]), (b"\x01\x02", [])])
    assert s1.dtype == np.int8 and s1.tolist() == [1, 2, 3, 1, 2] and off1.tolist() == [0, 3, 3, 5]
    assert s2.tolist() == [4, 1, 1] and off2.tolist() == [0, 1, 3, 3] and off1.dtype == np.int64
    s1, off1, s2, off2 = nwhip.batch_csr([])
    assert s1.size == 0 and off1.tolist() == [0] and off2.tolist() == [0]
    if not _gpu_visible():
        with pytest.raises(nwhip.NwError) as e:
            nwhip.score_batch([([1, 2, 3], [1, 2])])
        assert e.value.status == nwhip.NW_ERR_NODEVICE
        with pytest.raises(nwhip.NwError) as e:
            nwhip.align_batch([([1, 2, 3], [1, 2])])
        assert e.value.status == nwhip.NW_ERR_NODEVICE
