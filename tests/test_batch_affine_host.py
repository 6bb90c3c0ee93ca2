"""CPU: the host side of the batched alignment under affine gap cost
(nw_score_batch_affine, nw_align_batch_affine, nw_score_batch_affine_async,
nw_batch_affine_dir_bytes, nw_ops_score_affine; include/nw_hip.h).

The checker's own two fills against each other, nw_ops_score_affine against the
checker's direct summation, the direction-byte count, and every argument refusal --
checked before any HIP call, so answered without a device -- in the linear entries'
order (NW_ERR_ARG, then NW_ERR_UNSUPPORTED, then NW_ERR_NODEVICE).
"""
import ctypes
import itertools

import numpy as np
import pytest

import nw_gotoh
import nwhip
from nw_walk import walk as linear_walk
from test_batch_host import ALIGN_REFUSALS, ARG_REFUSALS, PARAM_REFUSALS, VALID, Call, _i8p, _i32p, _i64p, _u8p

SCHEMES = [(1, 0, -1), (1, -1, -1), (2, -1, -2), (2, -1, 0)]
SHAPES = [(1, 1), (5, 3), (3, 5), (17, 9), (40, 33), (64, 70)]


def _pair(rng, n1, n2, alpha=4):
    return rng.integers(1, alpha + 1, n1).astype(np.int8), rng.integers(1, alpha + 1, n2).astype(np.int8)


class AffineCall(Call):
    """test_batch_host.Call through the affine entries."""

    def __init__(self, gap_open=-3):
        super().__init__()
        self.go = gap_open

    def score(self):
        return nwhip.lib().nw_score_batch_affine(
            self._ptr("s1", self.s1, _i8p), self._ptr("off1", self.off1, _i64p), self._ptr("s2", self.s2, _i8p),
            self._ptr("off2", self.off2, _i64p), self.npairs, ctypes.byref(self.p) if self.p is not None else None,
            self.go, self._ptr("scores", self.scores, _i32p), None)

    def align(self):
        return nwhip.lib().nw_align_batch_affine(
            self._ptr("s1", self.s1, _i8p), self._ptr("off1", self.off1, _i64p), self._ptr("s2", self.s2, _i8p),
            self._ptr("off2", self.off2, _i64p), self.npairs, ctypes.byref(self.p) if self.p is not None else None,
            self.go, ctypes.byref(self.o) if self.o is not None else None, self._ptr("scores", self.scores, _i32p),
            self._ptr("ops", self.ops, _u8p), self._ptr("ops_off", self.ops_off, _i64p),
            self._ptr("n_ops", self.n_ops, _i64p), None)

    def score_async(self):
        return nwhip.lib().nw_score_batch_affine_async(
            None, self.s1.ctypes.data, self.off1.ctypes.data, self.s2.ctypes.data, self.off2.ctypes.data,
            self.npairs, int(self.off1[-1]), int(self.off2[-1]), 5,
            ctypes.byref(self.p) if self.p is not None else None, self.go, self.scores.ctypes.data, None)


# ------------------------------------------------------------------ the checker itself
@pytest.mark.parametrize("scheme", SCHEMES)
def test_checker_row_fill_equals_the_cell_recurrence(scheme):
    rng = np.random.default_rng(3)
    for (n1, n2), go in itertools.product(SHAPES + [(0, 4), (4, 0), (0, 0)], (0, -1, -3, -11)):
        a, b = _pair(rng, n1, n2)
        for x, y in zip(nw_gotoh.fill(a, b, scheme, go), nw_gotoh.fill_cells(a, b, scheme, go)):
            fin = y > nw_gotoh.NEG // 2
            np.testing.assert_array_equal(x[fin], y[fin])
            assert (x[~fin] < nw_gotoh.NEG // 2).all()


@pytest.mark.parametrize("scheme", SCHEMES)
def test_checker_with_gap_open_0_is_the_linear_walk(scheme):
    rng = np.random.default_rng(4)
    for n1, n2 in SHAPES:
        a, b = _pair(rng, n1, n2)
        ops = nw_gotoh.walk(a, b, scheme, 0)
        np.testing.assert_array_equal(ops, linear_walk(a, b, None, scheme))


# ------------------------------------------------------------------ nw_ops_score_affine
@pytest.mark.parametrize("scheme", SCHEMES)
def test_ops_score_affine_is_the_direct_sum(scheme):
    rng = np.random.default_rng(5)
    for (n1, n2), go in itertools.product(SHAPES + [(0, 4), (4, 0)], (-1, -3, -11)):
        a, b = _pair(rng, n1, n2)
        tables = nw_gotoh.fill(a, b, scheme, go)
        ops = nw_gotoh.walk(a, b, scheme, go, tables)
        want = nw_gotoh.path_score_affine(a, b, ops, scheme, go)
        assert want == tables[0][-1, -1]  # the walk's path is an optimal one
        assert nwhip.ops_score_affine(a, b, ops, scheme, go) == want
        # gap_open = 0: the linear sum
        assert nwhip.ops_score_affine(a, b, ops, scheme, 0) == nwhip.ops_score(a, b, ops, scheme)
    # an up-run directly followed by a left-run is two gaps; so is up, diag, up
    a, b = np.array([1, 2], np.int8), np.array([1, 2, 3], np.int8)
    assert nwhip.ops_score_affine(a, b, [1, 1, 2, 0], (5, -4, -1), -7) == 2 * -7 + 3 * -1 - 4
    b4 = np.array([1, 2, 3, 4], np.int8)
    assert nwhip.ops_score_affine(a, b4, [1, 0, 1, 0], (5, -4, -1), -7) == 2 * -7 + 2 * -1 - 4 - 4
    assert nwhip.ops_score_affine(a, b4, [0, 0, 1, 1], (5, -4, -1), -7) == 5 + 5 - 7 + 2 * -1
    assert nwhip.ops_score_affine(a, b, [], (5, -4, -1), -7, begin=(3, 2)) == 0


def test_ops_score_affine_refusals():
    a, b = np.array([1, 2], np.int8), np.array([1, 2, 3], np.int8)
    for ops in ([3], [0, 0, 0], [2, 2, 2], [1, 1, 1, 1]):
        with pytest.raises(nwhip.NwError) as e:
            nwhip.ops_score_affine(a, b, ops, (1, 0, -1), -3)
        assert e.value.status == nwhip.NW_ERR_ARG
        with pytest.raises(nwhip.NwError):
            nwhip.ops_score(a, b, ops, (1, 0, -1))
    with pytest.raises(nwhip.NwError):
        nwhip.ops_score_affine(a, b, [0], (1, 0, -1), -3, begin=(4, 0))
    f = nwhip.lib().nw_ops_score_affine
    o = np.zeros(1, np.uint8)
    sc = ctypes.c_int64()
    p = nwhip.params()
    args = (a.ctypes.data_as(_i8p), 2, b.ctypes.data_as(_i8p), 3, 0, 0, o.ctypes.data_as(_u8p), 1)
    assert f(*args, None, -3, ctypes.byref(sc)) == nwhip.NW_ERR_ARG
    assert f(*args, ctypes.byref(p), -3, None) == nwhip.NW_ERR_ARG
    assert f(*args, ctypes.byref(p), -3, ctypes.byref(sc)) == nwhip.NW_OK and sc.value == 1


# ------------------------------------------------------------------ direction bytes
def test_affine_dir_bytes():
    f = nwhip.batch_affine_dir_bytes
    assert f(0, 7) == 0 and f(7, 0) == 0 and f(0, 0) == 0
    assert f(-1, 7) == -1 and f(7, -1) == -1 and f(-1, -1) == -1 and f(-1, 0) == -1
    # 4 bits per cell: 8192 bytes per 64-step iteration (n2 / 64 + 2 of them) of a 256-column strip
    assert f(1, 1) == 2 * 8192
    assert f(256, 63) == 2 * 8192
    assert f(257, 64) == 2 * 3 * 8192
    assert f(4096, 4096) == 16 * 66 * 8192
    for n1, n2 in [(1, 1), (256, 63), (257, 64), (4096, 4096), (513, 130), (8000, 8000)]:
        assert f(n1, n2) == 2 * nwhip.batch_dir_bytes(n1, n2)
        assert f(n1, n2) >= (n1 * n2 + 1) // 2


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("case", sorted(PARAM_REFUSALS))
def test_param_refusals_need_no_device(case):
    kw, want = PARAM_REFUSALS[case]
    c = AffineCall()
    c.p = nwhip.params(**kw)
    assert c.score() == want
    assert c.align() == want
    assert c.score_async() == want


@pytest.mark.parametrize("case", sorted(ARG_REFUSALS))
def test_batch_refusals_need_no_device(case):
    c = AffineCall()
    ARG_REFUSALS[case](c)
    assert c.score() == nwhip.NW_ERR_ARG
    assert c.align() == nwhip.NW_ERR_ARG
    if case != "w_range":
        c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
        assert c.score() == nwhip.NW_ERR_ARG
        assert c.align() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("case", sorted(ALIGN_REFUSALS))
def test_align_batch_refusals_need_no_device(case):
    c = AffineCall()
    ALIGN_REFUSALS[case](c)
    assert c.align() == nwhip.NW_ERR_ARG


def test_gap_open_refusals_need_no_device():
    # a positive gap_open, whatever else is valid; before NW_KERNEL_PANELS' NW_ERR_UNSUPPORTED
    for go in (1, 7, 2 ** 31 - 1):
        c = AffineCall(go)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
        c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
    # the stated range: 3 |go| + (max|score| + |gap|) * (n1 + n2 + 2) < 2^28.  The longest pair
    # here is 5 x 5 and the scheme (1, 0, -1): 3 |go| + 2 * 12 < 2^28
    edge = (2 ** 28 - 1 - 24) // 3  # the largest |go| that passes
    assert 3 * edge + 24 < 2 ** 28 <= 3 * (edge + 1) + 24
    c = AffineCall(-edge)
    assert c.score() in VALID and c.align() in VALID
    for go in (-(edge + 1), -(2 ** 30), -(2 ** 31)):
        c = AffineCall(go)
        assert c.score() == nwhip.NW_ERR_ARG
        assert c.align() == nwhip.NW_ERR_ARG
    # the async form checks it for n1 = 0, n2 = max_n2 = 5: 3 |go| + 2 * 7
    edge = (2 ** 28 - 1 - 14) // 3
    assert AffineCall(-edge).score_async() == nwhip.NW_ERR_ARG  # (valid: no context)
    c = AffineCall(-edge)
    c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
    assert c.score_async() == nwhip.NW_ERR_UNSUPPORTED  # the range passed
    c.go = -(edge + 1)
    assert c.score_async() == nwhip.NW_ERR_ARG
    # a pair that passes the linear range check and not the affine one
    c = AffineCall(-(2 ** 26))
    c.p = nwhip.params((100, 0, -100))
    c.off1[:] = [0, 4, 4, 200004]
    c.off2[:] = [0, 3, 5, 200005]
    c.ops_off[:] = [0, 7, 9, 9 + 400000]
    assert 200 * 400002 < 2 ** 28 <= 3 * 2 ** 26 + 200 * 400002
    c.s1, c.s2 = np.ones(200004, np.int8), np.ones(200005, np.int8)
    c.ops = np.zeros(9 + 400000, np.uint8)
    assert c.score() == nwhip.NW_ERR_ARG and c.align() == nwhip.NW_ERR_ARG


def test_async_refusals_need_no_device():
    c = AffineCall()
    f = nwhip.lib().nw_score_batch_affine_async
    a = (c.s1.ctypes.data, c.off1.ctypes.data, c.s2.ctypes.data, c.off2.ctypes.data)
    p = ctypes.byref(c.p)
    sc = c.scores.ctypes.data
    assert f(None, *a, -1, 9, 10, 5, p, -3, sc, None) == nwhip.NW_ERR_ARG    # npairs < 0
    assert f(None, *a, 3, -1, 10, 5, p, -3, sc, None) == nwhip.NW_ERR_ARG    # total1 < 0
    assert f(None, *a, 3, 9, -1, 5, p, -3, sc, None) == nwhip.NW_ERR_ARG     # total2 < 0
    assert f(None, *a, 3, 9, 10, -1, p, -3, sc, None) == nwhip.NW_ERR_ARG    # max_n2 < 0
    assert f(None, *a, 3, 9, 10, 11, p, -3, sc, None) == nwhip.NW_ERR_ARG    # max_n2 > total2
    assert f(None, *a, 3, 9, 10, 5, None, -3, sc, None) == nwhip.NW_ERR_ARG  # p == NULL
    assert f(None, *a, 3, 9, 10, 5, p, -3, sc, None) == nwhip.NW_ERR_ARG     # valid, but no context
    big = nwhip.params((4000, 0, -4000))
    assert f(None, *a, 3, 9, 40000, 40000, ctypes.byref(big), -3, sc, None) == nwhip.NW_ERR_ARG  # range of max_n2


@pytest.mark.parametrize("defaults", [True, False])
def test_valid_arguments_reach_the_device(defaults):
    """Valid arguments (also p == NULL, NULL options, NO_PROFILE, gap_open = 0, empty pairs,
    an empty batch) pass the checks: NW_ERR_NODEVICE on a host without a GPU."""
    c = AffineCall(0 if defaults else -11)
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
    c = AffineCall()
    c.off1[:] = 0
    c.off2[:] = [0, 3, 5, 10]
    c.null = {"s1"}
    assert c.score() in VALID
    assert c.align() in VALID


def test_python_wrappers_without_a_device():
    if VALID == (nwhip.NW_OK,):
        return  # (with a device the wrappers are tests/test_batch_affine.py's)
    for f in (nwhip.score_batch_affine, nwhip.align_batch_affine):
        with pytest.raises(nwhip.NwError) as e:
            f([([1, 2, 3], [1, 2])], (1, -1, -1), -3)
        assert e.value.status == nwhip.NW_ERR_NODEVICE
        with pytest.raises(nwhip.NwError) as e:
            f([([1, 2, 3], [1, 2])], (1, -1, -1), 1)
        assert e.value.status == nwhip.NW_ERR_ARG
