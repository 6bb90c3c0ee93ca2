"""CPU: the host side of the banded batched alignment (nw_score_batch_banded,
nw_align_batch_banded, nw_score_batch_banded_async, nw_batch_banded_dir_bytes; include/
nw_hip.h) and the command line's --band.

The checker of tests/nw_banded.py against its own literal fill, against a brute force over the
definition (every monotone path whose vertices are all in the band, enumerated), and under a
covering band against tests/nw_gotoh_matrix.py (tables and walk); the direction-byte count;
every refusal of the three entries and its place in the order -- all answered without a
device, NW_ERR_NODEVICE last.
"""
import ctypes
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import nw_banded as nb
import nw_gotoh_matrix as gm
import nwhip
from conftest import ROOT
from test_batch_host import ALIGN_REFUSALS, ARG_REFUSALS, PARAM_REFUSALS, VALID, Call, _i8p, _i32p, _i64p, _u8p
from test_batch_matrix_host import _bad_matrices, identity_matrix, random_matrix

SHAPES = [(1, 1), (5, 3), (3, 5), (17, 9), (9, 30), (40, 33), (64, 70)]
COSTS = [(-1, -11), (-2, -3), (-3, 0)]  # (ge, go)
EXE = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")


def _pair(rng, n1, n2, alpha=4):
    return rng.integers(1, alpha + 1, n1).astype(np.int8), rng.integers(1, alpha + 1, n2).astype(np.int8)


class BandedCall(Call):
    """test_batch_host.Call through the banded entries."""

    def __init__(self, gap_open=-3, mat="default", band=2):
        super().__init__()
        self.go = gap_open
        self.band = band
        self.m = identity_matrix([1, 2, 3, 4], 1, 0, other=1).c if isinstance(mat, str) else mat

    def _m(self):
        return ctypes.byref(self.m) if self.m is not None else None

    def _p(self):
        return ctypes.byref(self.p) if self.p is not None else None

    def score(self):
        return nwhip.lib().nw_score_batch_banded(
            self._ptr("s1", self.s1, _i8p), self._ptr("off1", self.off1, _i64p), self._ptr("s2", self.s2, _i8p),
            self._ptr("off2", self.off2, _i64p), self.npairs, self._p(), self._m(), self.go, self.band,
            self._ptr("scores", self.scores, _i32p), None)

    def align(self):
        return nwhip.lib().nw_align_batch_banded(
            self._ptr("s1", self.s1, _i8p), self._ptr("off1", self.off1, _i64p), self._ptr("s2", self.s2, _i8p),
            self._ptr("off2", self.off2, _i64p), self.npairs, self._p(), self._m(), self.go, self.band,
            ctypes.byref(self.o) if self.o is not None else None, self._ptr("scores", self.scores, _i32p),
            self._ptr("ops", self.ops, _u8p), self._ptr("ops_off", self.ops_off, _i64p),
            self._ptr("n_ops", self.n_ops, _i64p), None)

    def score_async(self):
        return nwhip.lib().nw_score_batch_banded_async(
            None, self.s1.ctypes.data, self.off1.ctypes.data, self.s2.ctypes.data, self.off2.ctypes.data,
            self.npairs, int(self.off1[-1]), int(self.off2[-1]), 5, self._p(), self._m(), self.go, self.band,
            self.scores.ctypes.data, None)


# ------------------------------------------------------------------ the checker itself
def test_in_band_is_the_definition():
    assert nb.limits(5, 5, 0) == (0, 0) and nb.limits(5, 8, 2) == (-2, 5) and nb.limits(8, 5, 2) == (-5, 2)
    assert nb.in_band(3, 3, 0, 0) and not nb.in_band(3, 2, 0, 0) and not nb.in_band(2, 3, 0, 0)
    # the corners are always inside: the band widens by |delta|
    for n1, n2, w in itertools.product(range(7), range(7), range(4)):
        dlo, dhi = nb.limits(n1, n2, w)
        assert nb.in_band(0, 0, dlo, dhi) and nb.in_band(n2, n1, dlo, dhi)


@pytest.mark.parametrize("ge", [-1, -2, 0])
def test_checker_row_fill_equals_the_literal_fill(ge):
    rng = np.random.default_rng(61)
    for (n1, n2), go, w in itertools.product(SHAPES + [(0, 4), (4, 0), (0, 0)], (0, -1, -5, -11), (0, 1, 2, 5, 100)):
        mat = random_matrix(rng, 6, -9, 7)
        a, b = _pair(rng, n1, n2, 6)
        dlo, dhi = nb.limits(n1, n2, w)
        for lim in [dict(band=w), dict(dlo=dlo + 1, dhi=dhi), dict(dlo=dlo, dhi=dhi - 1)]:
            if "dlo" in lim and (lim["dlo"] > min(0, n2 - n1) or lim["dhi"] < max(0, n2 - n1)):
                continue  # (an edge moved past a corner: no path)
            got = nb.fill(a, b, mat.scores, mat.index, ge, go, **lim)
            want = nb.fill_cells(a, b, mat.scores, mat.index, ge, go, **lim)
            for x, y in zip(got, want):
                fin = y > nb.MINF // 2
                np.testing.assert_array_equal(x[fin], y[fin])
                assert (x[~fin] < nb.MINF // 2).all()
            # every in-band cell of H is finite, every other one -inf
            lo, hi = (lim["dlo"], lim["dhi"]) if "dlo" in lim else (dlo, dhi)
            i, j = np.mgrid[0:n2 + 1, 0:n1 + 1]
            inside = (i - j >= lo) & (i - j <= hi)
            assert ((got[0] > nb.MINF // 2) == inside).all()


@functools.lru_cache(maxsize=None)
def _paths(n1, n2):
    """Every monotone path (0, 0) -> (n2, n1): the 0/1 matrix path x diagonal cell, the number
    of gap ops, the number of runs, and the smallest and largest i - j over the vertices."""
    rows = []

    def go_(i, j, cells, gaps, runs, last, lo, hi):
        if (i, j) == (n2, n1):
            rows.append((tuple(cells), gaps, runs, lo, hi))
            return
        if i < n2 and j < n1:
            go_(i + 1, j + 1, cells + [i * n1 + j], gaps, runs, 0, lo, hi)
        if i < n2:
            go_(i + 1, j, cells, gaps + 1, runs + (last != 1), 1, lo, max(hi, i + 1 - j))
        if j < n1:
            go_(i, j + 1, cells, gaps + 1, runs + (last != 2), 2, min(lo, i - j - 1), hi)

    go_(0, 0, [], 0, 0, 0, 0, 0)
    P = np.zeros((len(rows), max(n1 * n2, 1)), np.int64)
    for r, row in enumerate(rows):
        P[r, list(row[0])] = 1
    cols = [np.array([row[k] for row in rows], np.int64) for k in (1, 2, 3, 4)]
    return (P, *cols)


@pytest.mark.parametrize("alpha", [2, 4])
@pytest.mark.parametrize("ge,go", COSTS)
def test_checker_is_the_path_definition(ge, go, alpha):
    """Sides 0..5 (empty sides included), w 0..6: the best score over the enumerated paths that
    stay in the band; 252 tables per cost and alphabet."""
    rng = np.random.default_rng(62 + alpha)
    mat = random_matrix(rng, alpha, -6, 7)
    cases = excluded = 0
    for n1, n2 in itertools.product(range(6), range(6)):
        a, b = _pair(rng, n1, n2, alpha)
        P, gaps, runs, lo, hi = _paths(n1, n2)
        sub = gm.sub_table(a, b, mat.scores, mat.index).reshape(-1) if n1 and n2 else np.zeros(1, np.int64)
        total = P @ sub + ge * gaps + go * runs
        for w in range(7):
            dlo, dhi = nb.limits(n1, n2, w)
            ok = (lo >= dlo) & (hi <= dhi)
            assert ok.any()
            want = int(total[ok].max())
            H, E, F = nb.fill_cells(a, b, mat.scores, mat.index, ge, go, w)
            assert H[-1, -1] == want, (n1, n2, w)
            excluded += not ok.all()
            ops = nb.walk(a, b, mat.scores, mat.index, ge, go, w, tables=(H, E, F))
            assert nb.path_score(a, b, ops, mat.scores, mat.index, ge, go) == want
            assert all(nb.in_band(i, j, dlo, dhi) for i, j in nb.path_vertices(ops))
            cases += 1
    # the band shuts paths out iff w < min(n1, n2): the sum of min(n1, n2) over the sides
    assert cases == 252 and excluded == 55


def test_covering_band_is_the_global_checker():
    rng = np.random.default_rng(63)
    for (n1, n2), (ge, go) in itertools.product(SHAPES + [(0, 4), (4, 0), (0, 0)], COSTS):
        mat = random_matrix(rng, 20, -8, 6)
        a, b = _pair(rng, n1, n2, 20)
        want = gm.fill(a, b, mat.scores, mat.index, ge, go)
        for w in (max(n1, n2), 10 ** 6):
            tables = nb.fill(a, b, mat.scores, mat.index, ge, go, w)
            for x, y in zip(tables, want):
                fin = y > gm.MINF // 2
                np.testing.assert_array_equal(x[fin], y[fin])
            ops = nb.walk(a, b, mat.scores, mat.index, ge, go, w, tables=tables)
            np.testing.assert_array_equal(ops, gm.walk(a, b, mat.scores, mat.index, ge, go, want))
            assert nwhip.ops_score_matrix(a, b, ops, mat, ge, go) == want[0][-1, -1]


def test_score_does_not_decrease_with_the_band_and_w0_is_the_diagonal():
    rng = np.random.default_rng(64)
    for (n1, n2), (ge, go) in itertools.product(SHAPES, COSTS):
        mat = random_matrix(rng, 4, -8, 6)
        a, b = _pair(rng, n1, n2)
        sc = [nb.score(a, b, mat.scores, mat.index, ge, go, w) for w in range(0, max(n1, n2) + 2)]
        assert all(x <= y for x, y in zip(sc, sc[1:]))
        assert sc[-1] == sc[-2] == gm.score(a, b, mat.scores, mat.index, ge, go)
        if n1 == n2:
            assert sc[0] == int(np.trace(gm.sub_table(a, b, mat.scores, mat.index)))
            assert (nb.walk(a, b, mat.scores, mat.index, ge, go, 0) == 0).all()


def test_walks_stay_in_the_band_and_sum_to_the_score():
    rng = np.random.default_rng(65)
    for (n1, n2), (ge, go), w in itertools.product(SHAPES, COSTS, (0, 1, 3, 8)):
        mat = random_matrix(rng, 4, -8, 4)
        a, b = _pair(rng, n1, n2)
        tables = nb.fill(a, b, mat.scores, mat.index, ge, go, w)
        ops = nb.walk(a, b, mat.scores, mat.index, ge, go, w, tables=tables)
        dlo, dhi = nb.limits(n1, n2, w)
        assert all(nb.in_band(i, j, dlo, dhi) for i, j in nb.path_vertices(ops))
        assert nb.path_score(a, b, ops, mat.scores, mat.index, ge, go) == tables[0][-1, -1]
        assert nwhip.ops_score_matrix(a, b, ops, mat, ge, go) == tables[0][-1, -1]


# ------------------------------------------------------------------ direction bytes
def _cap(n1, n2, w):
    return -(-n1 // 256) * (-(-(2 * w + abs(n2 - n1) + 319) // 64) + 3) * 8192


def test_banded_dir_bytes():
    f, full = nwhip.batch_banded_dir_bytes, nwhip.batch_affine_dir_bytes
    assert f(0, 5, 3) == f(5, 0, 3) == f(0, 0, 0) == 0
    assert f(-1, 5, 3) == f(5, -1, 3) == f(5, 5, -1) == f(0, 0, -1) == -1
    sizes = [1, 4, 63, 64, 65, 255, 256, 257, 513, 700, 2048, 8000, 100000]
    for n1, n2 in itertools.product(sizes, sizes):
        prev = 0
        for w in [0, 1, 31, 32, 63, 64, 65, 200, 1000, max(n1, n2) - 1, max(n1, n2), 10 ** 6, 2 ** 31 - 1]:
            got = f(n1, n2, w)
            assert 0 < got <= full(n1, n2) and got % 8192 == 0, (n1, n2, w)
            assert got <= _cap(n1, n2, w), (n1, n2, w)
            if w >= max(n1, n2):
                assert got == full(n1, n2)
        for w in sorted([0, 1, 31, 32, 63, 64, 65, 200, 1000, max(n1, n2), 10 ** 6]):
            assert f(n1, n2, w) >= prev  # monotone in w
            prev = f(n1, n2, w)
    # a long near-diagonal pair: 8000 x 8000 at w = 64 against the whole table's 33 MB
    assert full(8000, 8000) == 32 * 127 * 8192
    assert f(8000, 8000, 64) == 32 * 9 * 8192
    # a covering band by the definition alone: dlo <= -n1 and dhi >= n2
    assert f(300, 40, 40) == full(300, 40) and f(40, 300, 40) == full(40, 300)


def test_exports():
    with open(os.path.join(ROOT, "include", "nw_hip.h")) as fh:
        text = fh.read()
    for sym in ("nw_score_batch_banded_async", "nw_score_batch_banded", "nw_align_batch_banded",
                "nw_batch_banded_dir_bytes"):
        assert sym in nwhip.EXPORTS and hasattr(nwhip.lib(), sym) and sym + "(" in text


# ------------------------------------------------------------------ refusals, in their order
def test_mode_must_be_nw():
    for kw in (dict(mode=nwhip.MODE_SW, scheme=(1, -1, -1)), dict(mode=7)):
        c = BandedCall()
        c.p = nwhip.params(**kw)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("case", sorted(PARAM_REFUSALS))
def test_param_refusals_need_no_device(case):
    kw, want = PARAM_REFUSALS[case]
    for band in (2, -1):  # a bad band does not change the answer of an earlier refusal
        c = BandedCall(band=band)
        c.p = nwhip.params(**kw)
        want_ = nwhip.NW_ERR_ARG if band < 0 else want  # (band comes before NW_ERR_UNSUPPORTED)
        assert c.score() == want_
        assert c.align() == want_
        assert c.score_async() == want_


def test_gap_open_and_matrix_refusals_need_no_device():
    for go in (1, 7, 2 ** 31 - 1):
        c = BandedCall(go)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
    for m in _bad_matrices() + [None]:
        c = BandedCall(mat=m)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
        c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)  # before NW_ERR_UNSUPPORTED
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
        c = BandedCall(mat=m)
        c.npairs = 0
        c.null = {"s1", "s2", "off1", "off2", "scores", "ops", "ops_off", "n_ops"}
        assert c.score() == c.align() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("band", [-1, -2, -2 ** 31])
def test_negative_band_is_refused(band):
    c = BandedCall(band=band)
    assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
    # before NW_KERNEL_PANELS' NW_ERR_UNSUPPORTED, and before the offsets are looked at
    c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
    assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
    c = BandedCall(band=band)
    c.npairs = 0
    c.null = {"s1", "s2", "off1", "off2", "scores", "ops", "ops_off", "n_ops"}
    assert c.score() == c.align() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("band", [0, 1, 5, 10 ** 6, 2 ** 31 - 1])
def test_every_band_from_0_is_accepted(band):
    c = BandedCall(band=band)
    assert c.score() in VALID and c.align() in VALID
    c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
    assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_UNSUPPORTED


@pytest.mark.parametrize("case", sorted(ARG_REFUSALS))
def test_batch_refusals_need_no_device(case):
    """NULL scores, bad offsets, the range: NW_ERR_ARG, before PANELS."""
    c = BandedCall()
    ARG_REFUSALS[case](c)
    assert c.score() == nwhip.NW_ERR_ARG
    assert c.align() == nwhip.NW_ERR_ARG
    if case != "w_range":
        c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
        assert c.score() == nwhip.NW_ERR_ARG
        assert c.align() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("case", sorted(ALIGN_REFUSALS))
def test_align_batch_refusals_need_no_device(case):
    c = BandedCall()
    ALIGN_REFUSALS[case](c)
    assert c.align() == nwhip.NW_ERR_ARG
    assert c.score() in VALID  # (the score entry has no slots and no options)


@pytest.mark.parametrize("band", [0, 3, 10 ** 6])
def test_range_bound_at_its_edge(band):
    """The matrix entries' bound unchanged: 3 |go| + (M + |gap|) * (n1 + n2 + 2) < 2^28 with M
    = 128 from one entry of -128; the longest pair of the batch is 5 x 5.  A negative band is
    refused before it: with the range broken too the answer is still NW_ERR_ARG, and a
    negative band alone is refused where the range holds."""
    sc = np.zeros((4, 4), np.int64)
    sc[2, 1] = -128
    m = nwhip.SubMatrix([1, 2, 3, 4], sc, other=1).c
    go = -((2 ** 28 - 1 - 129 * 12) // 3)
    assert 3 * -go + 129 * 12 < 2 ** 28 <= 3 * -go + 129 * 13
    c = BandedCall(go, mat=m, band=band)
    assert c.score() in VALID and c.align() in VALID
    c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
    assert c.score() == c.align() == nwhip.NW_ERR_UNSUPPORTED  # the range passed; PANELS comes next
    assert BandedCall(go - 1, mat=m, band=band).score() == BandedCall(go - 1, mat=m, band=band).align() \
        == nwhip.NW_ERR_ARG
    assert BandedCall(go, mat=m, band=-1).score() == nwhip.NW_ERR_ARG
    c = BandedCall(go, mat=m, band=band)  # 6 x 5
    c.off1[:] = [0, 4, 4, 10]
    c.s1 = np.ones(10, np.int8)
    c.ops_off[:] = [0, 7, 9, 20]
    c.ops = np.zeros(20, np.uint8)
    assert c.score() == c.align() == nwhip.NW_ERR_ARG
    # the async form checks n1 = 0, n2 = max_n2 = 5: 3 |go| + 129 * 7
    go = -((2 ** 28 - 1 - 129 * 7) // 3)
    c = BandedCall(go, mat=m, band=band)
    c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
    assert c.score_async() == nwhip.NW_ERR_UNSUPPORTED
    c.go = go - 1
    assert c.score_async() == nwhip.NW_ERR_ARG


def test_async_refusals_need_no_device():
    c = BandedCall()
    f = nwhip.lib().nw_score_batch_banded_async
    a = (c.s1.ctypes.data, c.off1.ctypes.data, c.s2.ctypes.data, c.off2.ctypes.data)
    p, m = ctypes.byref(c.p), ctypes.byref(c.m)
    h = c.scores.ctypes.data
    assert f(None, *a, -1, 9, 10, 5, p, m, -3, 2, h, None) == nwhip.NW_ERR_ARG     # npairs < 0
    assert f(None, *a, 3, -1, 10, 5, p, m, -3, 2, h, None) == nwhip.NW_ERR_ARG     # total1 < 0
    assert f(None, *a, 3, 9, 10, 11, p, m, -3, 2, h, None) == nwhip.NW_ERR_ARG     # max_n2 > total2
    assert f(None, *a, 3, 9, 10, 5, None, m, -3, 2, h, None) == nwhip.NW_ERR_ARG   # p == NULL
    assert f(None, *a, 3, 9, 10, 5, p, None, -3, 2, h, None) == nwhip.NW_ERR_ARG   # m == NULL
    assert f(None, *a, 3, 9, 10, 5, p, m, -3, -1, h, None) == nwhip.NW_ERR_ARG     # band
    assert f(None, *a, 3, 9, 10, 5, p, m, -3, 2, h, None) == nwhip.NW_ERR_ARG      # valid, but no context


@pytest.mark.parametrize("defaults", [True, False])
def test_valid_arguments_reach_the_device(defaults):
    """NW_ERR_NODEVICE is the last refusal; p == NULL is the defaults."""
    c = BandedCall(0 if defaults else -11, band=0 if defaults else 7)
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
    for f in (nwhip.score_batch_banded, nwhip.align_batch_banded):
        with pytest.raises(ValueError):  # an unlisted byte without other=
            f([([1, 2, 3], [1, 4])], mat, -1, -3, 2)
        with pytest.raises(nwhip.NwError) as e:
            f([([1, 2, 3], [1, 2])], mat, -1, 1, 2)
        assert e.value.status == nwhip.NW_ERR_ARG
        with pytest.raises(nwhip.NwError) as e:
            f([([1, 2, 3], [1, 2])], mat, -1, -3, -1)
        assert e.value.status == nwhip.NW_ERR_ARG
        if VALID != (nwhip.NW_OK,):
            with pytest.raises(nwhip.NwError) as e:
                f([([1, 2, 3], [1, 2])], mat, -1, -3, 10 ** 12)  # (any width: capped at int32's)
            assert e.value.status == nwhip.NW_ERR_NODEVICE


# ------------------------------------------------------------------ the command line
def _cli(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)


def test_cli_band_argument_errors(tmp_path):
    (tmp_path / "a.bdna").write_bytes(b"ACGTACGT")
    lst = tmp_path / "pairs.txt"
    lst.write_text("a.bdna a.bdna\n")
    r = _cli(str(tmp_path / "a.bdna"), str(tmp_path / "a.bdna"), "--band", "3")
    assert r.returncode == 1 and "--band needs --batch" in r.stdout
    r = _cli("--batch", str(lst), "--band", "3", "--local")
    assert r.returncode == 1 and "--band cannot be combined with --local" in r.stdout
    r = _cli("--batch", str(lst), "--band", "3", "--ends", "3")
    assert r.returncode == 1 and "--band cannot be combined with --ends" in r.stdout
    for bad in ("-1", "x", "3x", "", "99999999999"):
        r = _cli("--batch", str(lst), "--band", bad)
        assert r.returncode == 1 and "--band expects a number >= 0" in r.stdout, bad
    r = _cli("--batch", str(lst), "--band")
    assert r.returncode == 1 and "--band expects a number >= 0" in r.stdout
    r = _cli("--batch", str(lst), "--band", "3", "--gap-open", "3")
    assert r.returncode == 1 and "--gap-open expects a number <= 0" in r.stdout
    (tmp_path / "m.txt").write_text("A C\nA 1 -1\nC -1 1\n")
    r = _cli("--batch", str(lst), "--band", "3", "--matrix", str(tmp_path / "m.txt"))
    assert r.returncode == 1 and "is not a letter of the matrix" in r.stdout  # G, T
    if VALID != (nwhip.NW_OK,):
        r = _cli("--batch", str(lst), "--band", "3")
        assert r.returncode == 2 and "no gfx950 device" in r.stderr
