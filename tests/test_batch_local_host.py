"""CPU: the host side of the batched local alignment (nw_score_batch_local,
nw_align_batch_local, nw_score_batch_local_async, nw_local_hit; include/nw_hip.h),
nwhip.SubMatrix.uniform and the command line's --local.

The checker of tests/nw_local.py against its own literal fill on asymmetric matrices and,
with gap_open = 0 and a match / mismatch matrix, against the oracle's Smith-Waterman
(fill, best cell, traceback); every refusal of the three entries and its place in the
order -- all answered without a device, NW_ERR_NODEVICE last -- and the struct size.
"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import nw_local as nl
import nwhip
import oracle
from conftest import ROOT
from test_batch_host import ALIGN_REFUSALS, ARG_REFUSALS, PARAM_REFUSALS, VALID, Call, _i8p, _i64p, _u8p
from test_batch_matrix_host import _bad_matrices, random_matrix
from test_sw import SCHEMES as SW_SCHEMES

SHAPES = [(1, 1), (5, 3), (3, 5), (17, 9), (40, 33), (64, 70)]
_hp = ctypes.POINTER(nwhip.NwLocalHit)
EXE = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")


def _pair(rng, n1, n2, alpha=4):
    return rng.integers(1, alpha + 1, n1).astype(np.int8), rng.integers(1, alpha + 1, n2).astype(np.int8)


class LocalCall(Call):
    """test_batch_host.Call through the local entries: mode SW, hits for scores."""

    def __init__(self, gap_open=-3, mat="default"):
        super().__init__()
        self.p = nwhip.params(mode=nwhip.MODE_SW)
        self.go = gap_open
        self.m = nwhip.SubMatrix.uniform([1, 2, 3], 1, 0, other=4).c if isinstance(mat, str) else mat
        self.scores = np.zeros(3, nwhip.LOCAL_HIT_DTYPE)

    def _m(self):
        return ctypes.byref(self.m) if self.m is not None else None

    def _p(self):
        return ctypes.byref(self.p) if self.p is not None else None

    def score(self):
        return nwhip.lib().nw_score_batch_local(
            self._ptr("s1", self.s1, _i8p), self._ptr("off1", self.off1, _i64p), self._ptr("s2", self.s2, _i8p),
            self._ptr("off2", self.off2, _i64p), self.npairs, self._p(), self._m(), self.go,
            self._ptr("scores", self.scores, _hp), None)

    def align(self):
        return nwhip.lib().nw_align_batch_local(
            self._ptr("s1", self.s1, _i8p), self._ptr("off1", self.off1, _i64p), self._ptr("s2", self.s2, _i8p),
            self._ptr("off2", self.off2, _i64p), self.npairs, self._p(), self._m(), self.go,
            ctypes.byref(self.o) if self.o is not None else None, self._ptr("scores", self.scores, _hp),
            self._ptr("ops", self.ops, _u8p), self._ptr("ops_off", self.ops_off, _i64p),
            self._ptr("n_ops", self.n_ops, _i64p), None)

    def score_async(self):
        return nwhip.lib().nw_score_batch_local_async(
            None, self.s1.ctypes.data, self.off1.ctypes.data, self.s2.ctypes.data, self.off2.ctypes.data,
            self.npairs, int(self.off1[-1]), int(self.off2[-1]), 5, self._p(), self._m(), self.go,
            self.scores.ctypes.data, None)


# ------------------------------------------------------------------ the checker itself
@pytest.mark.parametrize("ge", [-1, -2, 0])
def test_checker_row_fill_equals_the_literal_fill(ge):
    rng = np.random.default_rng(41)
    seen_positive = 0
    for (n1, n2), go in itertools.product(SHAPES + [(0, 4), (4, 0), (0, 0)], (0, -1, -5, -11)):
        mat = random_matrix(rng, 6, -9, 7)
        assert (mat.scores != mat.scores.T).any()
        a, b = _pair(rng, n1, n2, 6)
        got, want = nl.fill(a, b, mat.scores, mat.index, ge, go), nl.fill_cells(a, b, mat.scores, mat.index, ge, go)
        for x, y in zip(got, want):
            fin = y > nl.MINF // 2
            np.testing.assert_array_equal(x[fin], y[fin])
            assert (x[~fin] < nl.MINF // 2).all()
        assert (got[0] >= 0).all() and (got[0][0] == 0).all() and (got[0][:, 0] == 0).all()
        seen_positive += got[0].max() > 0
    assert seen_positive > 20


@pytest.mark.parametrize("sch", SW_SCHEMES)
def test_checker_with_gap_open_0_is_the_oracles_smith_waterman(sch):
    """Table, best cell, begin cell and ops on 20 small pairs."""
    rng = np.random.default_rng(42)
    mat = nwhip.SubMatrix.uniform([1, 2, 3, 4], sch[0], sch[1])
    shapes = SHAPES + [(9, 31), (33, 2), (20, 20), (1, 7), (7, 1), (2, 2), (50, 50), (31, 64), (65, 12), (12, 65),
                       (3, 3), (90, 40), (40, 90), (25, 26)]
    assert len(shapes) == 20
    for n1, n2 in shapes:
        a, b = _pair(rng, n1, n2)
        if n1 >= 20 and n2 >= 20:  # a shared segment, so that the best path is long
            b[5:18] = a[3:16]
        t = oracle.sw_fill(a, b, sch)
        tables = nl.fill(a, b, mat.scores, mat.index, sch[2], 0)
        np.testing.assert_array_equal(tables[0], t)
        sc, ei, ej = nl.best(tables[0])
        assert (sc, ei, ej) == tuple(int(v) for v in oracle.sw_best(a, b, sch))
        ops, begin = nl.walk(a, b, mat.scores, mat.index, sch[2], 0, tables)
        want_ops, bi, bj = oracle.sw_traceback(a, b, t, (ei, ej), sch)
        np.testing.assert_array_equal(ops, want_ops)
        assert begin == (bi, bj)
        assert nl.path_score(a, b, ops, begin, mat.scores, mat.index, sch[2], 0) == (sc, (ei, ej))


def test_checker_walk_and_direct_sum_under_affine_cost():
    rng = np.random.default_rng(43)
    for (n1, n2), go, ge in itertools.product(SHAPES, (0, -3, -11), (-1, -2)):
        mat = random_matrix(rng, 20, -8, 6)
        a, b = _pair(rng, n1, n2, 20)
        tables = nl.fill_cells(a, b, mat.scores, mat.index, ge, go)
        sc, ei, ej = nl.best(tables[0])
        ops, begin = nl.walk(a, b, mat.scores, mat.index, ge, go, tables)
        assert nl.path_score(a, b, ops, begin, mat.scores, mat.index, ge, go) == (sc, (ei, ej))
        assert tables[0][begin] == 0 and ops.size <= n1 + n2
        assert nwhip.ops_score_matrix(a, b, ops, mat, ge, go, begin=begin) == sc


def test_all_negative_matrix_aligns_nothing():
    rng = np.random.default_rng(44)
    mat = nwhip.SubMatrix([1, 2, 3, 4], -rng.integers(1, 9, (4, 4)))
    a, b = _pair(rng, 40, 33)
    tables = nl.fill(a, b, mat.scores, mat.index, -1, -3)
    assert nl.best(tables[0]) == (0, 0, 0)
    ops, begin = nl.walk(a, b, mat.scores, mat.index, -1, -3, tables)
    assert ops.size == 0 and begin == (0, 0)
    assert nl.best(nl.fill([], b, mat.scores, mat.index, -1, -3)[0]) == (0, 0, 0)


# ------------------------------------------------------------------ the struct
def test_local_hit_layout():
    assert ctypes.sizeof(nwhip.NwLocalHit) == 32 == nwhip.LOCAL_HIT_DTYPE.itemsize
    assert [f[0] for f in nwhip.NwLocalHit._fields_] == list(nwhip.LOCAL_HIT_DTYPE.names)
    assert nwhip.NwLocalHit.begin_i.offset == 12 and nwhip.NwLocalHit.reserved.offset == 20
    with open(os.path.join(ROOT, "include", "nw_hip.h")) as f:
        assert "typedef struct nw_local_hit {      /* 32 bytes */" in f.read()


# ------------------------------------------------------------------ SubMatrix.uniform
def test_submatrix_uniform():
    m = nwhip.SubMatrix.uniform("ACGT", 2, -3)
    assert m.n == 4 and m.other is None and m.scores.tolist() == (np.eye(4, dtype=int) * 5 - 3).tolist()
    assert m.index[ord("g")] == 2 and not m.listed[ord("N")]
    m = nwhip.SubMatrix.uniform("ACGT", 2, -3, other="N")
    assert m.n == 5 and m.other == ord("N") and m.index[ord("X")] == 4 and m.index[0] == 4
    assert m.scores[4].tolist() == [-3] * 5 and m.scores[:, 4].tolist() == [-3] * 5  # N against N is no match
    assert m.scores[:4, :4].tolist() == (np.eye(4, dtype=int) * 5 - 3).tolist()
    m = nwhip.SubMatrix.uniform([1, 2, 3], 1, 0, other=4)
    assert m.letters == [1, 2, 3, 4] and m.c.n == 4 and m.c.score[0] == 1 and m.c.score[3 * 32 + 3] == 0
    with pytest.raises(ValueError):
        nwhip.SubMatrix.uniform("ACGT", 2, -3, other="A")  # other is one more letter
    with pytest.raises(ValueError):
        nwhip.SubMatrix.uniform("ACGT", 200, -3)


# ------------------------------------------------------------------ refusals, in their order
def test_mode_must_be_sw():
    for kw in (dict(mode=nwhip.MODE_NW), dict(mode=7)):
        c = LocalCall()
        c.p = nwhip.params(**kw)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
        # before every other refusal: a bad matrix, NULL hits and PANELS change nothing
        c.p.kernel = nwhip.KERNEL_PANELS
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
    c = LocalCall()
    c.p = nwhip.params((1, 0, 1), mode=nwhip.MODE_SW)  # gap > 0: valid_params refuses it in mode SW
    assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
    c.p = nwhip.params((1, 0, 0), mode=nwhip.MODE_SW)  # gap = 0 is allowed
    assert c.score() in VALID and c.align() in VALID


@pytest.mark.parametrize("case", sorted(set(PARAM_REFUSALS) - {"mode_sw"}))
def test_param_refusals_need_no_device(case):
    kw, want = PARAM_REFUSALS[case]
    c = LocalCall()
    kw = dict(kw)
    kw.setdefault("mode", nwhip.MODE_SW)
    c.p = nwhip.params(**kw)
    assert c.score() == want
    assert c.align() == want
    assert c.score_async() == want


def test_gap_open_and_matrix_refusals_need_no_device():
    for go in (1, 7, 2 ** 31 - 1):
        c = LocalCall(go)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
    for m in _bad_matrices() + [None]:
        c = LocalCall(mat=m)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
        c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS, mode=nwhip.MODE_SW)  # before NW_ERR_UNSUPPORTED
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
        # and before the offsets are looked at: an empty batch with NULL arrays is refused too
        c = LocalCall(mat=m)
        c.npairs = 0
        c.null = {"s1", "s2", "off1", "off2", "scores", "ops", "ops_off", "n_ops"}
        assert c.score() == c.align() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("case", sorted(ARG_REFUSALS))
def test_batch_refusals_need_no_device(case):
    """NULL hits ("null_scores"), bad offsets, the range: NW_ERR_ARG, before PANELS."""
    c = LocalCall()
    ARG_REFUSALS[case](c)
    c.p.mode = nwhip.MODE_SW  # (the range case replaces the parameters)
    assert c.score() == nwhip.NW_ERR_ARG
    assert c.align() == nwhip.NW_ERR_ARG
    if case != "w_range":
        c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS, mode=nwhip.MODE_SW)
        assert c.score() == nwhip.NW_ERR_ARG
        assert c.align() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("case", sorted(ALIGN_REFUSALS))
def test_align_batch_refusals_need_no_device(case):
    c = LocalCall()
    ALIGN_REFUSALS[case](c)
    assert c.align() == nwhip.NW_ERR_ARG
    assert c.score() in VALID  # (the score entry has no slots and no options)


def test_range_bound_at_its_edge():
    """The matrix entries' bound unchanged: 3 |go| + (M + |gap|) * (n1 + n2 + 2) < 2^28 with M
    = 128 from one entry of -128; the longest pair of the batch is 5 x 5."""
    sc = np.zeros((4, 4), np.int64)
    sc[2, 1] = -128
    m = nwhip.SubMatrix([1, 2, 3, 4], sc, other=1).c
    go = -((2 ** 28 - 1 - 129 * 12) // 3)
    assert 3 * -go + 129 * 12 < 2 ** 28 <= 3 * -go + 129 * 13
    c = LocalCall(go, mat=m)
    assert c.score() in VALID and c.align() in VALID
    c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS, mode=nwhip.MODE_SW)
    assert c.score() == c.align() == nwhip.NW_ERR_UNSUPPORTED  # the range passed; PANELS comes next
    assert LocalCall(go - 1, mat=m).score() == LocalCall(go - 1, mat=m).align() == nwhip.NW_ERR_ARG
    c = LocalCall(go, mat=m)  # 6 x 5
    c.off1[:] = [0, 4, 4, 10]
    c.s1 = np.ones(10, np.int8)
    c.ops_off[:] = [0, 7, 9, 20]
    c.ops = np.zeros(20, np.uint8)
    assert c.score() == c.align() == nwhip.NW_ERR_ARG
    # the async form checks n1 = 0, n2 = max_n2 = 5: 3 |go| + 129 * 7
    go = -((2 ** 28 - 1 - 129 * 7) // 3)
    c = LocalCall(go, mat=m)
    c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS, mode=nwhip.MODE_SW)
    assert c.score_async() == nwhip.NW_ERR_UNSUPPORTED
    c.go = go - 1
    assert c.score_async() == nwhip.NW_ERR_ARG


def test_async_refusals_need_no_device():
    c = LocalCall()
    f = nwhip.lib().nw_score_batch_local_async
    a = (c.s1.ctypes.data, c.off1.ctypes.data, c.s2.ctypes.data, c.off2.ctypes.data)
    p, m = ctypes.byref(c.p), ctypes.byref(c.m)
    h = c.scores.ctypes.data
    assert f(None, *a, -1, 9, 10, 5, p, m, -3, h, None) == nwhip.NW_ERR_ARG     # npairs < 0
    assert f(None, *a, 3, -1, 10, 5, p, m, -3, h, None) == nwhip.NW_ERR_ARG     # total1 < 0
    assert f(None, *a, 3, 9, 10, 11, p, m, -3, h, None) == nwhip.NW_ERR_ARG     # max_n2 > total2
    assert f(None, *a, 3, 9, 10, 5, None, m, -3, h, None) == nwhip.NW_ERR_ARG   # p == NULL
    assert f(None, *a, 3, 9, 10, 5, p, None, -3, h, None) == nwhip.NW_ERR_ARG   # m == NULL
    assert f(None, *a, 3, 9, 10, 5, p, m, -3, h, None) == nwhip.NW_ERR_ARG      # valid, but no context


@pytest.mark.parametrize("defaults", [True, False])
def test_valid_arguments_reach_the_device(defaults):
    """NW_ERR_NODEVICE is the last refusal; p == NULL is the defaults with mode SW."""
    c = LocalCall(0 if defaults else -11)
    if defaults:
        c.p = None
    else:
        c.p = nwhip.params((2, -1, -2), flags=nwhip.FLAG_NO_PROFILE, waves=3, mode=nwhip.MODE_SW)
        c.o = nwhip.NwBatchOpts(1 << 30)
    assert c.score() in VALID
    assert c.align() in VALID
    c.npairs = 0
    c.null = {"s1", "s2", "off1", "off2", "scores", "ops", "ops_off", "n_ops"}
    assert c.score() in VALID
    assert c.align() in VALID


def test_python_wrappers_without_a_device():
    mat = nwhip.SubMatrix.uniform([1, 2, 3], 1, -1)
    for f in (nwhip.score_batch_local, nwhip.align_batch_local):
        with pytest.raises(ValueError):  # an unlisted byte without other=
            f([([1, 2, 3], [1, 4])], mat, -1, -3)
        with pytest.raises(nwhip.NwError) as e:
            f([([1, 2, 3], [1, 2])], mat, -1, 1)
        assert e.value.status == nwhip.NW_ERR_ARG
        with pytest.raises(nwhip.NwError) as e:
            f([([1, 2, 3], [1, 2])], mat, 1, -3)  # gap > 0
        assert e.value.status == nwhip.NW_ERR_ARG
        if VALID != (nwhip.NW_OK,):
            with pytest.raises(nwhip.NwError) as e:
                f([([1, 2, 3], [1, 2])], mat, -1, -3)
            assert e.value.status == nwhip.NW_ERR_NODEVICE


# ------------------------------------------------------------------ the command line
def _cli(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


def test_cli_local_argument_errors(tmp_path):
    (tmp_path / "a.bdna").write_bytes(b"ACGTACGT")
    lst = tmp_path / "pairs.txt"
    lst.write_text("a.bdna a.bdna\n")
    r = _cli(str(tmp_path / "a.bdna"), str(tmp_path / "a.bdna"), "--local")
    assert r.returncode == 1 and "--local needs --batch" in r.stdout
    r = _cli("--batch", str(lst), "--local", "--scheme", "1,-1,1")
    assert r.returncode == 1 and "--local needs a gap of at most 0" in r.stdout
    r = _cli("--batch", str(lst), "--local", "--scheme", "200,-1,-1")
    assert r.returncode == 1 and "-128..127" in r.stdout
    r = _cli("--batch", str(lst), "--local", "--gap-open", "3")
    assert r.returncode == 1 and "--gap-open expects a number <= 0" in r.stdout
    r = _cli("--batch", str(lst), "--local", "--matrix", str(tmp_path / "none.txt"))
    assert r.returncode == 1 and "no such file" in r.stdout
    (tmp_path / "m.txt").write_text("A C\nA 1 -1\nC -1 1\n")
    r = _cli("--batch", str(lst), "--local", "--matrix", str(tmp_path / "m.txt"))
    assert r.returncode == 1 and "is not a letter of the matrix" in r.stdout  # G, T
    lst.write_text("a.bdna missing.bdna\n")
    r = _cli("--batch", str(lst), "--local")
    assert r.returncode == 1 and "no such file" in r.stdout
    if VALID != (nwhip.NW_OK,):
        lst.write_text("a.bdna a.bdna\n")
        r = _cli("--batch", str(lst), "--local")
        assert r.returncode == 2 and "no gfx950 device" in r.stderr
