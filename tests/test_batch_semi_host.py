"""CPU: the host side of the batched semi-global alignment (nw_score_batch_semi,
nw_align_batch_semi, nw_score_batch_semi_async, NW_ENDS_*; include/nw_hip.h) and the command
line's --ends.

The checker of tests/nw_semi.py against its own literal fill, against a brute force over the
path definition (for every admissible begin and end cell the global Gotoh score of the
sub-rectangle between them, maximised; all 16 `ends`, sides 0..5, empty sides included) and,
with ends = 0, against tests/nw_gotoh_matrix.py (tables and walk); every refusal of the three
entries and its place in the order -- all answered without a device, NW_ERR_NODEVICE last.
"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import nw_gotoh_matrix as gm
import nw_semi as ns
import nwhip
from conftest import ROOT
from test_batch_host import ALIGN_REFUSALS, ARG_REFUSALS, PARAM_REFUSALS, VALID, Call, _i8p, _i64p, _u8p
from test_batch_matrix_host import _bad_matrices, identity_matrix, random_matrix

SHAPES = [(1, 1), (5, 3), (3, 5), (17, 9), (40, 33), (64, 70)]
COSTS = [(-1, -11), (-2, -3), (-3, 0)]  # (ge, go)
_hp = ctypes.POINTER(nwhip.NwLocalHit)
EXE = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")


def _pair(rng, n1, n2, alpha=4):
    return rng.integers(1, alpha + 1, n1).astype(np.int8), rng.integers(1, alpha + 1, n2).astype(np.int8)


class SemiCall(Call):
    """test_batch_host.Call through the semi-global entries: hits for scores, and `ends`."""

    def __init__(self, gap_open=-3, mat="default", ends=3):
        super().__init__()
        self.go = gap_open
        self.ends = ends
        self.m = identity_matrix([1, 2, 3, 4], 1, 0, other=1).c if isinstance(mat, str) else mat
        self.scores = np.zeros(3, nwhip.LOCAL_HIT_DTYPE)

    def _m(self):
        return ctypes.byref(self.m) if self.m is not None else None

    def _p(self):
        return ctypes.byref(self.p) if self.p is not None else None

    def score(self):
        return nwhip.lib().nw_score_batch_semi(
            self._ptr("s1", self.s1, _i8p), self._ptr("off1", self.off1, _i64p), self._ptr("s2", self.s2, _i8p),
            self._ptr("off2", self.off2, _i64p), self.npairs, self._p(), self._m(), self.go, self.ends,
            self._ptr("scores", self.scores, _hp), None)

    def align(self):
        return nwhip.lib().nw_align_batch_semi(
            self._ptr("s1", self.s1, _i8p), self._ptr("off1", self.off1, _i64p), self._ptr("s2", self.s2, _i8p),
            self._ptr("off2", self.off2, _i64p), self.npairs, self._p(), self._m(), self.go, self.ends,
            ctypes.byref(self.o) if self.o is not None else None, self._ptr("scores", self.scores, _hp),
            self._ptr("ops", self.ops, _u8p), self._ptr("ops_off", self.ops_off, _i64p),
            self._ptr("n_ops", self.n_ops, _i64p), None)

    def score_async(self):
        return nwhip.lib().nw_score_batch_semi_async(
            None, self.s1.ctypes.data, self.off1.ctypes.data, self.s2.ctypes.data, self.off2.ctypes.data,
            self.npairs, int(self.off1[-1]), int(self.off2[-1]), 5, self._p(), self._m(), self.go, self.ends,
            self.scores.ctypes.data, None)


# ------------------------------------------------------------------ the checker itself
@pytest.mark.parametrize("ge", [-1, -2, 0])
def test_checker_row_fill_equals_the_literal_fill(ge):
    rng = np.random.default_rng(51)
    for (n1, n2), go, ends in itertools.product(SHAPES + [(0, 4), (4, 0), (0, 0)], (0, -1, -5, -11), range(16)):
        if (n1, n2) in ((40, 33), (64, 70)) and ends not in (0, 3, 6, 9, 12, 15):
            continue
        mat = random_matrix(rng, 6, -9, 7)
        a, b = _pair(rng, n1, n2, 6)
        got = ns.fill(a, b, mat.scores, mat.index, ge, go, ends)
        want = ns.fill_cells(a, b, mat.scores, mat.index, ge, go, ends)
        for x, y in zip(got, want):
            fin = y > ns.MINF // 2
            np.testing.assert_array_equal(x[fin], y[fin])
            assert (x[~fin] < ns.MINF // 2).all()
        H = got[0]
        assert H[0, 0] == 0
        assert (H[0, 1:] == 0).all() if ends & 1 else (H[0, 1:] == go + ge * np.arange(1, n1 + 1)).all()
        assert (H[1:, 0] == 0).all() if ends & 4 else (H[1:, 0] == go + ge * np.arange(1, n2 + 1)).all()


def _brute(a, b, mat, ge, go, ends):
    """The path definition: the best global Gotoh score of a sub-rectangle between an
    admissible begin cell and an admissible end cell."""
    n1, n2 = len(a), len(b)
    begins = {(0, 0)}
    if ends & 1:
        begins |= {(0, j) for j in range(n1 + 1)}
    if ends & 4:
        begins |= {(i, 0) for i in range(n2 + 1)}
    best = None
    for (bi, bj), (ei, ej) in itertools.product(sorted(begins), ns.end_cells(n1, n2, ends)):
        if bi > ei or bj > ej:
            continue
        sc = gm.score(a[bj:ej], b[bi:ei], mat.scores, mat.index, ge, go)
        best = sc if best is None else max(best, sc)
    return best


@pytest.mark.parametrize("alpha", [2, 4])
@pytest.mark.parametrize("ge,go", COSTS)
def test_checker_is_the_path_definition(ge, go, alpha):
    """All 16 `ends`, sides 0..5 (empty sides included): 576 tables per cost and alphabet,
    3456 in all."""
    rng = np.random.default_rng(52 + alpha)
    mat = random_matrix(rng, alpha, -6, 7)
    cases = 0
    for n1, n2 in itertools.product(range(6), range(6)):
        a, b = _pair(rng, n1, n2, alpha)
        for ends in range(16):
            H = ns.fill_cells(a, b, mat.scores, mat.index, ge, go, ends)[0]
            sc, ei, ej = ns.end_cell(H, ends)
            assert sc == _brute(a, b, mat, ge, go, ends), (n1, n2, ends)
            # the walk's path is one of the definition's and sums to the score
            ops, begin = ns.walk(a, b, mat.scores, mat.index, ge, go, ends)
            assert ns.path_score(a, b, ops, begin, mat.scores, mat.index, ge, go) == (sc, (ei, ej))
            assert begin == (0, 0) or (begin[0] == 0 and ends & 1) or (begin[1] == 0 and ends & 4)
            assert ops.size <= n1 + n2
            cases += 1
    assert cases == 576


def test_ends_0_is_the_global_checker():
    rng = np.random.default_rng(53)
    for (n1, n2), (ge, go) in itertools.product(SHAPES + [(0, 4), (4, 0), (0, 0)], COSTS):
        mat = random_matrix(rng, 20, -8, 6)
        a, b = _pair(rng, n1, n2, 20)
        tables = ns.fill(a, b, mat.scores, mat.index, ge, go, 0)
        want = gm.fill(a, b, mat.scores, mat.index, ge, go)
        for x, y in zip(tables, want):
            fin = y > gm.MINF // 2
            np.testing.assert_array_equal(x[fin], y[fin])
        assert ns.end_cell(tables[0], 0) == (int(want[0][-1, -1]), n2, n1)
        ops, begin = ns.walk(a, b, mat.scores, mat.index, ge, go, 0, tables)
        np.testing.assert_array_equal(ops, gm.walk(a, b, mat.scores, mat.index, ge, go, want))
        assert begin == (0, 0)
        assert nwhip.ops_score_matrix(a, b, ops, mat, ge, go) == want[0][-1, -1]


def test_overlap_scores_are_not_negative_and_the_walks_sum_up():
    rng = np.random.default_rng(54)
    negative = 0
    for (n1, n2), (ge, go), ends in itertools.product(SHAPES, COSTS, range(16)):
        mat = random_matrix(rng, 20, -8, 4)
        a, b = _pair(rng, n1, n2, 20)
        tables = ns.fill(a, b, mat.scores, mat.index, ge, go, ends)
        sc, ei, ej = ns.end_cell(tables[0], ends)
        if ends == 15:
            assert sc >= 0
        negative += sc < 0
        ops, begin = ns.walk(a, b, mat.scores, mat.index, ge, go, ends, tables)
        assert ns.path_score(a, b, ops, begin, mat.scores, mat.index, ge, go) == (sc, (ei, ej))
        assert nwhip.ops_score_matrix(a, b, ops, mat, ge, go, begin=begin) == sc
    assert negative > 50  # (the score may be negative, and is on these matrices)


def test_constants():
    assert (nwhip.ENDS_S1_BEGIN, nwhip.ENDS_S1_END, nwhip.ENDS_S2_BEGIN, nwhip.ENDS_S2_END) == (1, 2, 4, 8)
    assert (nwhip.ENDS_GLOBAL, nwhip.ENDS_S2_IN_S1, nwhip.ENDS_S1_IN_S2, nwhip.ENDS_OVERLAP) == (0, 3, 12, 15)
    with open(os.path.join(ROOT, "include", "nw_hip.h")) as f:
        text = f.read()
    for name, v in [("S1_BEGIN", 1), ("S1_END", 2), ("S2_BEGIN", 4), ("S2_END", 8), ("GLOBAL", 0), ("S2_IN_S1", 3),
                    ("S1_IN_S2", 12), ("OVERLAP", 15)]:
        assert f"NW_ENDS_{name} = {v}" in text
    for sym in ("nw_score_batch_semi_async", "nw_score_batch_semi", "nw_align_batch_semi"):
        assert sym in nwhip.EXPORTS and hasattr(nwhip.lib(), sym)


# ------------------------------------------------------------------ refusals, in their order
def test_mode_must_be_nw():
    for kw in (dict(mode=nwhip.MODE_SW, scheme=(1, -1, -1)), dict(mode=7)):
        c = SemiCall()
        c.p = nwhip.params(**kw)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("case", sorted(PARAM_REFUSALS))
def test_param_refusals_need_no_device(case):
    kw, want = PARAM_REFUSALS[case]
    c = SemiCall()
    c.p = nwhip.params(**kw)
    assert c.score() == want
    assert c.align() == want
    assert c.score_async() == want


def test_gap_open_and_matrix_refusals_need_no_device():
    for go in (1, 7, 2 ** 31 - 1):
        c = SemiCall(go)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
    for m in _bad_matrices() + [None]:
        c = SemiCall(mat=m)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
        c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)  # before NW_ERR_UNSUPPORTED
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
        c = SemiCall(mat=m)
        c.npairs = 0
        c.null = {"s1", "s2", "off1", "off2", "scores", "ops", "ops_off", "n_ops"}
        assert c.score() == c.align() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("ends", [-1, 16, 31, -2 ** 31, 2 ** 31 - 1])
def test_ends_outside_0_to_15_is_refused(ends):
    c = SemiCall(ends=ends)
    assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
    # before NW_KERNEL_PANELS' NW_ERR_UNSUPPORTED, and before the offsets are looked at
    c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
    assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
    c = SemiCall(ends=ends)
    c.npairs = 0
    c.null = {"s1", "s2", "off1", "off2", "scores", "ops", "ops_off", "n_ops"}
    assert c.score() == c.align() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("ends", range(16))
def test_every_ends_from_0_to_15_is_accepted(ends):
    c = SemiCall(ends=ends)
    assert c.score() in VALID and c.align() in VALID
    c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
    assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_UNSUPPORTED


@pytest.mark.parametrize("case", sorted(ARG_REFUSALS))
def test_batch_refusals_need_no_device(case):
    """NULL hits ("null_scores"), bad offsets, the range: NW_ERR_ARG, before PANELS."""
    c = SemiCall()
    ARG_REFUSALS[case](c)
    assert c.score() == nwhip.NW_ERR_ARG
    assert c.align() == nwhip.NW_ERR_ARG
    if case != "w_range":
        c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
        assert c.score() == nwhip.NW_ERR_ARG
        assert c.align() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("case", sorted(ALIGN_REFUSALS))
def test_align_batch_refusals_need_no_device(case):
    c = SemiCall()
    ALIGN_REFUSALS[case](c)
    assert c.align() == nwhip.NW_ERR_ARG
    assert c.score() in VALID  # (the score entry has no slots and no options)


@pytest.mark.parametrize("ends", [0, 3, 15])
def test_range_bound_at_its_edge(ends):
    """The matrix entries' bound unchanged: 3 |go| + (M + |gap|) * (n1 + n2 + 2) < 2^28 with M
    = 128 from one entry of -128; the longest pair of the batch is 5 x 5.  A bad `ends` is
    refused before it: with the range broken too the answer is still NW_ERR_ARG, and a bad
    `ends` alone is refused where the range holds."""
    sc = np.zeros((4, 4), np.int64)
    sc[2, 1] = -128
    m = nwhip.SubMatrix([1, 2, 3, 4], sc, other=1).c
    go = -((2 ** 28 - 1 - 129 * 12) // 3)
    assert 3 * -go + 129 * 12 < 2 ** 28 <= 3 * -go + 129 * 13
    c = SemiCall(go, mat=m, ends=ends)
    assert c.score() in VALID and c.align() in VALID
    c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
    assert c.score() == c.align() == nwhip.NW_ERR_UNSUPPORTED  # the range passed; PANELS comes next
    assert SemiCall(go - 1, mat=m, ends=ends).score() == SemiCall(go - 1, mat=m, ends=ends).align() == nwhip.NW_ERR_ARG
    assert SemiCall(go, mat=m, ends=16).score() == nwhip.NW_ERR_ARG
    c = SemiCall(go, mat=m, ends=ends)  # 6 x 5
    c.off1[:] = [0, 4, 4, 10]
    c.s1 = np.ones(10, np.int8)
    c.ops_off[:] = [0, 7, 9, 20]
    c.ops = np.zeros(20, np.uint8)
    assert c.score() == c.align() == nwhip.NW_ERR_ARG
    # the async form checks n1 = 0, n2 = max_n2 = 5: 3 |go| + 129 * 7
    go = -((2 ** 28 - 1 - 129 * 7) // 3)
    c = SemiCall(go, mat=m, ends=ends)
    c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
    assert c.score_async() == nwhip.NW_ERR_UNSUPPORTED
    c.go = go - 1
    assert c.score_async() == nwhip.NW_ERR_ARG


def test_async_refusals_need_no_device():
    c = SemiCall()
    f = nwhip.lib().nw_score_batch_semi_async
    a = (c.s1.ctypes.data, c.off1.ctypes.data, c.s2.ctypes.data, c.off2.ctypes.data)
    p, m = ctypes.byref(c.p), ctypes.byref(c.m)
    h = c.scores.ctypes.data
    assert f(None, *a, -1, 9, 10, 5, p, m, -3, 3, h, None) == nwhip.NW_ERR_ARG     # npairs < 0
    assert f(None, *a, 3, -1, 10, 5, p, m, -3, 3, h, None) == nwhip.NW_ERR_ARG     # total1 < 0
    assert f(None, *a, 3, 9, 10, 11, p, m, -3, 3, h, None) == nwhip.NW_ERR_ARG     # max_n2 > total2
    assert f(None, *a, 3, 9, 10, 5, None, m, -3, 3, h, None) == nwhip.NW_ERR_ARG   # p == NULL
    assert f(None, *a, 3, 9, 10, 5, p, None, -3, 3, h, None) == nwhip.NW_ERR_ARG   # m == NULL
    assert f(None, *a, 3, 9, 10, 5, p, m, -3, 16, h, None) == nwhip.NW_ERR_ARG     # ends
    assert f(None, *a, 3, 9, 10, 5, p, m, -3, 3, h, None) == nwhip.NW_ERR_ARG      # valid, but no context


@pytest.mark.parametrize("defaults", [True, False])
def test_valid_arguments_reach_the_device(defaults):
    """NW_ERR_NODEVICE is the last refusal; p == NULL is the defaults (mode NW)."""
    c = SemiCall(0 if defaults else -11, ends=3 if defaults else 9)
    if defaults:
        c.p = None
    else:
        c.p = nwhip.params((2, -1, -2), flags=nwhip.FLAG_NO_PROFILE, waves=3)
        c.o = nwhip.NwBatchOpts(1 << 30)
    assert c.score() in VALID
    assert c.align() in VALID
    c.npairs = 0
    c.null = {"s1", "s2", "off1", "off2", "scores", "ops", "ops_off", "n_ops"}
    assert c.score() in VALID
    assert c.align() in VALID


def test_python_wrappers_without_a_device():
    mat = nwhip.SubMatrix.uniform([1, 2, 3], 1, -1)
    for f in (nwhip.score_batch_semi, nwhip.align_batch_semi):
        with pytest.raises(ValueError):  # an unlisted byte without other=
            f([([1, 2, 3], [1, 4])], mat, -1, -3, 3)
        with pytest.raises(nwhip.NwError) as e:
            f([([1, 2, 3], [1, 2])], mat, -1, 1, 3)
        assert e.value.status == nwhip.NW_ERR_ARG
        with pytest.raises(nwhip.NwError) as e:
            f([([1, 2, 3], [1, 2])], mat, -1, -3, 16)
        assert e.value.status == nwhip.NW_ERR_ARG
        if VALID != (nwhip.NW_OK,):
            with pytest.raises(nwhip.NwError) as e:
                f([([1, 2, 3], [1, 2])], mat, -1, -3, 3)
            assert e.value.status == nwhip.NW_ERR_NODEVICE


# ------------------------------------------------------------------ the command line
def _cli(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


def test_cli_ends_argument_errors(tmp_path):
    (tmp_path / "a.bdna").write_bytes(b"ACGTACGT")
    lst = tmp_path / "pairs.txt"
    lst.write_text("a.bdna a.bdna\n")
    r = _cli(str(tmp_path / "a.bdna"), str(tmp_path / "a.bdna"), "--ends", "3")
    assert r.returncode == 1 and "--ends needs --batch" in r.stdout
    r = _cli("--batch", str(lst), "--ends", "3", "--local")
    assert r.returncode == 1 and "--ends cannot be combined with --local" in r.stdout
    for bad in ("16", "-1", "x", "3x"):
        r = _cli("--batch", str(lst), "--ends", bad)
        assert r.returncode == 1 and "--ends expects a number in 0..15" in r.stdout, bad
    r = _cli("--batch", str(lst), "--ends")
    assert r.returncode == 1 and "--ends expects a number in 0..15" in r.stdout
    r = _cli("--batch", str(lst), "--ends", "3", "--scheme", "200,-1,-1")
    assert r.returncode == 1 and "-128..127" in r.stdout
    r = _cli("--batch", str(lst), "--ends", "3", "--gap-open", "3")
    assert r.returncode == 1 and "--gap-open expects a number <= 0" in r.stdout
    r = _cli("--batch", str(lst), "--ends", "3", "--matrix", str(tmp_path / "none.txt"))
    assert r.returncode == 1 and "no such file" in r.stdout
    (tmp_path / "m.txt").write_text("A C\nA 1 -1\nC -1 1\n")
    r = _cli("--batch", str(lst), "--ends", "3", "--matrix", str(tmp_path / "m.txt"))
    assert r.returncode == 1 and "is not a letter of the matrix" in r.stdout  # G, T
    if VALID != (nwhip.NW_OK,):
        r = _cli("--batch", str(lst), "--ends", "3")
        assert r.returncode == 2 and "no gfx950 device" in r.stderr
