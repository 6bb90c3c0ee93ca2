"""CPU: the two-piece batch entries (nw_score_batch_dual, nw_align_batch_dual, nw_score_batch_
dual_async, nw_batch_dual_dir_bytes, nw_ops_score_dual) without a device: the checker of
tests/nw_gotoh2.py against the definition (every path of tiny pairs), its row fill against
its cell fill, the three reductions to tests/nw_gotoh_matrix.py, nw_ops_score_dual against
the direct sum, the sizes, every refusal in its order with the range bound at its edge, the
CLI's argument errors, and what tests/test_batch_dual.py relies on: that both pieces matter
on its grid, and that the paths of its coverage list read every unrolled cell instance of
the sweep in every way the five-state walk can read one (tests/nw_dirmap2.py).

`python tests/test_batch_dual_host.py` (with the package on PYTHONPATH) runs the greedy pass
over the coverage candidates again and prints the KEPT table.
"""
import collections
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import nw_dirmap as dm
import nw_dirmap2 as dm2
import nw_gotoh2 as g2
import nw_gotoh_matrix as gm
import nwhip
from conftest import ROOT
from test_batch import _rand, score_pairs
from test_batch_host import ALIGN_REFUSALS, ARG_REFUSALS, PARAM_REFUSALS, VALID, Call, _i8p, _i32p, _i64p, _u8p
from test_batch_matrix_host import _bad_matrices, identity_matrix, random_matrix
from test_batch_paths_host import LETTERS, _matrix, wide_form

# (go1, ge1, go2, ge2)
CROSSING = [(-4, -2, -24, -1), (-2, -3, -5, -1), (0, -3, -6, -1), (-5, -1, -2, -3)]   # two distinct pieces, each best somewhere
EQUAL = [(-3, -2, -3, -2)]
DOMINATED = [(-2, -1, -4, -2), (-6, -3, -2, -1), (-1, 1, -2, 0)]   # piece 2, piece 1, piece 2 under a positive extension
PIECES = CROSSING + EQUAL + DOMINATED


def crossover(pc):
    """The run lengths k >= 1 up to 400 that piece 1 prices, and those piece 2 prices."""
    k = np.arange(1, 401)
    one = pc[0] + k * pc[1] >= pc[2] + k * pc[3]
    return k[one], k[~one]


def test_the_parameter_sets():
    for pc in CROSSING:
        one, two = crossover(pc)
        assert one.size and two.size
    for pc in EQUAL:
        assert pc[:2] == pc[2:]
    for pc in DOMINATED:
        one, two = crossover(pc)
        assert one.size == 0 or two.size == 0 or (pc[0] + one * pc[1] == pc[2] + one * pc[3]).all()
    assert crossover((-4, -2, -24, -1))[1][0] == 21   # a run of 20 ties: both pieces give -44


@functools.lru_cache(maxsize=None)
def matrix(alpha):
    """Seeded, asymmetric, entries in -8..12, over the bytes 1..alpha."""
    m = random_matrix(np.random.default_rng(700 + alpha), alpha)
    assert (m.scores != m.scores.T).any()
    return m


# ------------------------------------------------------------------ the checker against the definition
@pytest.mark.parametrize("pc", PIECES, ids=str)
def test_definition_on_every_path_of_tiny_pairs(pc):
    """brute (every path, the direct sum with the max per run) == the recurrence == the direct
    sum over the walk's ops; sides 0..5, a 4-letter identity-type and an asymmetric matrix."""
    rng = np.random.default_rng(PIECES.index(pc))
    mats = [identity_matrix([1, 2, 3, 4], 2, -4), matrix(4)]
    for t in range(60):
        m = mats[t & 1]
        a = rng.integers(1, 5, int(rng.integers(0, 6))).astype(np.int8)
        b = rng.integers(1, 5, int(rng.integers(0, 6))).astype(np.int8)
        tabs = g2.fill_cells(a, b, m.scores, m.index, pc)
        ops = g2.walk(a, b, m.scores, m.index, pc, tabs)
        want = g2.brute(a, b, m.scores, m.index, pc)
        assert want == tabs[0][-1, -1] == g2.path_score(a, b, ops, m.scores, m.index, pc), (a, b)
        assert max(a.size, b.size) <= ops.size <= a.size + b.size


@pytest.mark.parametrize("pc", PIECES, ids=str)
def test_row_fill_equals_the_cell_recurrence(pc):
    """All five tables, not H alone: the walk's "opening wins" test reads E_t and F_t."""
    rng = np.random.default_rng(3)
    m = matrix(4)
    for n1, n2 in [(0, 4), (4, 0), (1, 1), (37, 29), (70, 41)]:
        a, b = rng.integers(1, 5, n1).astype(np.int8), rng.integers(1, 5, n2).astype(np.int8)
        got, want = g2.fill(a, b, m.scores, m.index, pc), g2.fill_cells(a, b, m.scores, m.index, pc)
        for x, y in zip(got, want):
            np.testing.assert_array_equal(np.maximum(x, -(1 << 30)), np.maximum(y, -(1 << 30)))
        np.testing.assert_array_equal(g2.walk(a, b, m.scores, m.index, pc, got), g2.walk(a, b, m.scores, m.index, pc, want))


# ------------------------------------------------------------------ reductions
REDUCTIONS = [   # (pieces, the (ge, go) of the matrix entries that give the same bytes)
    ((-3, -2, -3, -2), (-2, -3)),      # equal pieces
    ((-11, -1, -11, -1), (-1, -11)),
    ((-2, -1, -4, -2), (-1, -2)),      # piece 2 nowhere above piece 1
    ((-2, -1, -2, -3), (-1, -2)),
    ((-1, 1, -2, 0), (1, -1)),
    ((-6, -3, -2, -1), (-1, -2)),      # piece 1 strictly below piece 2
    ((-3, -1, -2, -1), (-1, -2)),
]


@pytest.mark.parametrize("pc,single", REDUCTIONS, ids=str)
def test_reductions_to_the_matrix_checker(pc, single):
    rng = np.random.default_rng(5)
    for alpha in (4, 20):
        m = matrix(alpha)
        for n1, n2 in [(0, 3), (3, 0), (1, 1), (30, 25), (64, 80), (90, 33)]:
            a, b = rng.integers(1, alpha + 1, n1).astype(np.int8), rng.integers(1, alpha + 1, n2).astype(np.int8)
            tabs = g2.fill(a, b, m.scores, m.index, pc)
            old = gm.fill(a, b, m.scores, m.index, *single)
            assert tabs[0][-1, -1] == old[0][-1, -1]
            np.testing.assert_array_equal(g2.walk(a, b, m.scores, m.index, pc, tabs),
                                          gm.walk(a, b, m.scores, m.index, *single, old))


# ------------------------------------------------------------------ nw_ops_score_dual
def _ops_score(a, b, ops, m, pc):
    return nwhip.ops_score_dual(a, b, ops, m, pc[1], pc[0], pc[3], pc[2])


def test_ops_score_dual_is_the_direct_sum():
    rng = np.random.default_rng(7)
    m = matrix(4)
    for pc in PIECES:
        for _ in range(12):
            a = rng.integers(1, 5, int(rng.integers(0, 40))).astype(np.int8)
            b = rng.integers(1, 5, int(rng.integers(0, 40))).astype(np.int8)
            ops = g2.walk(a, b, m.scores, m.index, pc)
            assert _ops_score(a, b, ops, m, pc) == g2.path_score(a, b, ops, m.scores, m.index, pc)
    # runs at, one below and one above the crossover length; a run alone, first, last
    pc = (-4, -2, -24, -1)
    for k, want in [(19, -42), (20, -44), (21, -45), (300, -324), (1, -6)]:
        a, b = np.ones(k + 2, np.int8), np.ones(2, np.int8)
        s = int(m.scores[0, 0])
        for ops in ([0] + [2] * k + [0], [2] * k + [0, 0], [0, 0] + [2] * k):
            assert _ops_score(a, b, ops, m, pc) == want + 2 * s == g2.path_score(a, b, ops, m.scores, m.index, pc)
            assert _ops_score(b, a, [1 if o == 2 else o for o in ops], m, pc) == want + 2 * s
    # an up-run directly followed by a left-run is two gaps: g(25) + g(30), not g(55)
    a, b = np.ones(30, np.int8), np.ones(25, np.int8)
    ops = [1] * 25 + [2] * 30
    assert _ops_score(a, b, ops, m, pc) == -49 + -54 == g2.path_score(a, b, ops, m.scores, m.index, pc)
    assert _ops_score(a, b, ops[::-1], m, pc) == -49 + -54
    # equal pieces: nw_ops_score_matrix
    a, b = rng.integers(1, 5, 50).astype(np.int8), rng.integers(1, 5, 44).astype(np.int8)
    ops = gm.walk(a, b, m.scores, m.index, -2, -3)
    assert _ops_score(a, b, ops, m, (-3, -2, -3, -2)) == nwhip.ops_score_matrix(a, b, ops, m, -2, -3)


def test_ops_score_dual_refusals():
    m = matrix(4)
    a, b = np.ones(3, np.int8), np.ones(2, np.int8)
    for ops in ([0, 0, 0], [0, 0, 2, 2], [3, 0, 0], [1, 1, 1, 2, 2, 2], [0, 0, 2, 0]):   # as ops_score_matrix refuses them
        with pytest.raises(nwhip.NwError) as e:
            nwhip.ops_score_matrix(a, b, ops, m, -1, -2)
        assert e.value.status == nwhip.NW_ERR_ARG
        with pytest.raises(nwhip.NwError) as e:
            nwhip.ops_score_dual(a, b, ops, m)
        assert e.value.status == nwhip.NW_ERR_ARG
    with pytest.raises(nwhip.NwError):
        nwhip.ops_score_dual(a, b, [0, 0, 2], m, begin=(0, 2))
    f = nwhip.lib().nw_ops_score_dual
    o = np.array([0, 0, 2], np.uint8)
    p, sc = nwhip.params((1, 0, -2)), ctypes.c_int64()
    args = (a.ctypes.data_as(_i8p), 3, b.ctypes.data_as(_i8p), 2, 0, 0, o.ctypes.data_as(_u8p), 3)
    assert f(*args, ctypes.byref(p), ctypes.byref(m.c), -4, -24, -1, ctypes.byref(sc)) == nwhip.NW_OK
    assert sc.value == 2 * int(m.scores[0, 0]) - 6
    assert f(*args, None, ctypes.byref(m.c), -4, -24, -1, ctypes.byref(sc)) == nwhip.NW_ERR_ARG
    assert f(*args, ctypes.byref(p), None, -4, -24, -1, ctypes.byref(sc)) == nwhip.NW_ERR_ARG
    assert f(*args, ctypes.byref(p), ctypes.byref(m.c), -4, -24, -1, None) == nwhip.NW_ERR_ARG
    for bad in _bad_matrices():
        assert f(*args, ctypes.byref(p), ctypes.byref(bad), -4, -24, -1, ctypes.byref(sc)) == nwhip.NW_ERR_ARG


# ------------------------------------------------------------------ sizes
def test_dir_bytes():
    for n1, n2 in [(1, 1), (256, 63), (257, 64), (513, 130), (8000, 8000)]:
        assert nwhip.batch_dual_dir_bytes(n1, n2) == 2 * nwhip.batch_affine_dir_bytes(n1, n2) == dm2.dir_bytes(n1, n2)
    assert nwhip.batch_dual_dir_bytes(0, 5) == nwhip.batch_dual_dir_bytes(5, 0) == nwhip.batch_dual_dir_bytes(0, 0) == 0
    assert nwhip.batch_dual_dir_bytes(-1, 5) == nwhip.batch_dual_dir_bytes(5, -1) == -1


@pytest.mark.parametrize("n1,n2", [(5, 3), (256, 64), (257, 127), (700, 330)])
def test_byte_places_are_distinct_and_inside_the_block(n1, n2):
    r, c = np.mgrid[1:n2 + 1, 1:n1 + 1]
    byte = dm2.byte_place(r, c, n2)
    assert byte.min() >= 0 and byte.max() < dm2.dir_bytes(n1, n2)
    assert np.unique(byte.ravel()).size == n1 * n2


# ------------------------------------------------------------------ refusals
class DualCall(Call):
    """test_batch_host.Call through the two-piece entries."""

    def __init__(self, pc=(-4, -2, -24, -1), mat="default"):
        super().__init__()
        self.go, self.go2, self.ge2 = pc[0], pc[2], pc[3]
        self.p = nwhip.params((1, 0, pc[1]))
        self.m = identity_matrix([1, 2, 3, 4], 1, 0, other=1).c if isinstance(mat, str) else mat

    def _m(self):
        return ctypes.byref(self.m) if self.m is not None else None

    def _p(self):
        return ctypes.byref(self.p) if self.p is not None else None

    def score(self):
        return nwhip.lib().nw_score_batch_dual(
            self._ptr("s1", self.s1, _i8p), self._ptr("off1", self.off1, _i64p), self._ptr("s2", self.s2, _i8p),
            self._ptr("off2", self.off2, _i64p), self.npairs, self._p(), self._m(), self.go, self.go2, self.ge2,
            self._ptr("scores", self.scores, _i32p), None)

    def align(self):
        return nwhip.lib().nw_align_batch_dual(
            self._ptr("s1", self.s1, _i8p), self._ptr("off1", self.off1, _i64p), self._ptr("s2", self.s2, _i8p),
            self._ptr("off2", self.off2, _i64p), self.npairs, self._p(), self._m(), self.go, self.go2, self.ge2,
            ctypes.byref(self.o) if self.o is not None else None, self._ptr("scores", self.scores, _i32p),
            self._ptr("ops", self.ops, _u8p), self._ptr("ops_off", self.ops_off, _i64p),
            self._ptr("n_ops", self.n_ops, _i64p), None)

    def score_async(self):
        return nwhip.lib().nw_score_batch_dual_async(
            None, self.s1.ctypes.data, self.off1.ctypes.data, self.s2.ctypes.data, self.off2.ctypes.data,
            self.npairs, int(self.off1[-1]), int(self.off2[-1]), 5, self._p(), self._m(), self.go, self.go2, self.ge2,
            self.scores.ctypes.data, None)


@pytest.mark.parametrize("case", sorted(PARAM_REFUSALS))
def test_param_refusals_need_no_device(case):
    kw, want = PARAM_REFUSALS[case]
    c = DualCall()
    c.p = nwhip.params(**kw)
    assert c.score() == c.align() == c.score_async() == want


@pytest.mark.parametrize("case", sorted(ARG_REFUSALS))
def test_batch_refusals_need_no_device(case):
    c = DualCall()
    keep = c.p
    ARG_REFUSALS[case](c)
    if case == "w_range":   # (the case puts its own parameters in: piece 2 must not be what is refused)
        c.go2, c.ge2 = c.go, c.p.gap
    elif c.p is not None and c.p.gap != keep.gap:
        c.ge2 = c.p.gap
    assert c.score() == nwhip.NW_ERR_ARG
    assert c.align() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("case", sorted(ALIGN_REFUSALS))
def test_align_batch_refusals_need_no_device(case):
    c = DualCall()
    ALIGN_REFUSALS[case](c)
    assert c.align() == nwhip.NW_ERR_ARG


def test_matrix_and_gap_open_refusals_need_no_device():
    for m in _bad_matrices() + [None]:
        c = DualCall(mat=m)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
        c.p = nwhip.params((1, 0, -2), kernel=nwhip.KERNEL_PANELS)   # before NW_ERR_UNSUPPORTED
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
    for go in (1, 7, 2 ** 31 - 1):
        c = DualCall((go, -2, -24, -1))
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG


def test_piece_2_refusals_and_their_order():
    """gap_open2 > 0; gap2 outside nw_params.gap's range (|gap| < 4096, positive legal); both
    NW_ERR_ARG, before NW_KERNEL_PANELS' NW_ERR_UNSUPPORTED and before the offsets are looked
    at, as the checks before them are."""
    for go2, ge2 in [(1, -1), (2 ** 31 - 1, -1), (-24, 4096), (-24, -4096), (-24, 2 ** 31 - 1), (-24, -2 ** 31)]:
        c = DualCall((-4, -2, go2, ge2))
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
        c.p = nwhip.params((1, 0, -2), kernel=nwhip.KERNEL_PANELS)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
        c = DualCall((-4, -2, go2, ge2))
        c.npairs = 0
        c.null = {"s1", "s2", "off1", "off2", "scores", "ops", "ops_off", "n_ops"}
        assert c.score() == c.align() == nwhip.NW_ERR_ARG
    for go2, ge2 in [(0, -1), (-24, 4095), (-24, -4095), (-24, 1), (-24, 0), (-2 ** 20, -1)]:
        c = DualCall((-4, -2, go2, ge2))
        assert c.score() in VALID and c.align() in VALID
        c.p = nwhip.params((1, 0, -2), kernel=nwhip.KERNEL_PANELS)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_UNSUPPORTED
    # nw_params.gap itself is held to the same range by the parameter check
    c = DualCall()
    c.p = nwhip.params((1, 0, 4096))
    assert c.score() == nwhip.NW_ERR_ARG


def test_range_bound_at_its_edge():
    """3 G + (M + A) * (n1 + n2 + 2) < 2^28, G = max |go_t|, A = max |ge_t|, M = max(A, entries):
    the longest pair of the batch is 5 x 5; one below the edge passes, the edge does not; G, A
    and M are taken from either piece."""
    sc = np.zeros((4, 4), np.int64)
    sc[2, 1] = -128
    m = nwhip.SubMatrix([1, 2, 3, 4], sc, other=1).c
    g = (2 ** 28 - 1 - (128 + 2) * 12) // 3
    assert 3 * g + 130 * 12 < 2 ** 28 <= 3 * (g + 1) + 130 * 12
    panels = nwhip.params((1, 0, -2), kernel=nwhip.KERNEL_PANELS)
    for pc in [(-g, -2, -24, -1), (-4, -2, -g, -1), (-g, -1, -g, -2), (-4, -1, -g, 2)]:
        c = DualCall(pc, mat=m)
        assert c.score() in VALID and c.align() in VALID
        c.p = nwhip.params((1, 0, pc[1]), kernel=nwhip.KERNEL_PANELS)
        assert c.score() == c.align() == nwhip.NW_ERR_UNSUPPORTED   # the range passed
        worse = tuple(-g - 1 if x == -g else x for x in pc)
        c = DualCall(worse, mat=m)
        assert c.score() == c.align() == nwhip.NW_ERR_ARG
        c = DualCall(pc, mat=m)   # 6 x 5
        c.off1[:] = [0, 4, 4, 10]
        c.s1 = np.ones(10, np.int8)
        c.ops_off[:] = [0, 7, 9, 20]
        c.ops = np.zeros(20, np.uint8)
        assert c.score() == c.align() == nwhip.NW_ERR_ARG
    # A from piece 2 alone: |ge2| = 3 makes it (128 + 3) * 12
    c = DualCall((-g, -2, -24, -3), mat=m)
    assert 3 * g + 131 * 12 >= 2 ** 28 and c.score() == nwhip.NW_ERR_ARG
    # M = A when an extension exceeds every entry
    c = DualCall((-g, -2, -24, -200), mat=m)
    assert c.score() == nwhip.NW_ERR_ARG
    g2_ = (2 ** 28 - 1 - 400 * 12) // 3
    assert DualCall((-g2_, -2, -24, -200), mat=m).score() in VALID
    assert DualCall((-g2_ - 1, -2, -24, -200), mat=m).score() == nwhip.NW_ERR_ARG
    # the async form checks n1 = 0, n2 = max_n2 = 5
    ga = (2 ** 28 - 1 - 130 * 7) // 3
    c = DualCall((-4, -2, -ga, -1), mat=m)
    c.p = panels
    assert c.score_async() == nwhip.NW_ERR_UNSUPPORTED
    c.go2 = -ga - 1
    assert c.score_async() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("defaults", [True, False])
def test_valid_arguments_reach_the_device(defaults):
    c = DualCall()
    if defaults:
        c.p = None   # (the reference defaults: gap -1)
    else:
        c.p = nwhip.params((2, -1, -2), waves=3)
        c.o = nwhip.NwBatchOpts(1 << 30)
    assert c.score() in VALID and c.align() in VALID
    c.npairs = 0
    c.null = {"s1", "s2", "off1", "off2", "scores", "ops", "ops_off", "n_ops"}
    assert c.score() in VALID and c.align() in VALID


def test_python_wrappers_without_a_device():
    m = matrix(4)
    with pytest.raises(ValueError):   # a byte the matrix does not list
        nwhip.score_batch_dual([(np.array([9], np.int8), np.array([1], np.int8))], m)
    if VALID == (nwhip.NW_ERR_NODEVICE,):
        with pytest.raises(nwhip.NwError) as e:
            nwhip.score_batch_dual([(np.ones(3, np.int8), np.ones(2, np.int8))], m)
        assert e.value.status == nwhip.NW_ERR_NODEVICE
    with pytest.raises(nwhip.NwError) as e:
        nwhip.align_batch_dual([(np.ones(3, np.int8), np.ones(2, np.int8))], m, gap_open2=1)
    assert e.value.status == nwhip.NW_ERR_ARG


# ------------------------------------------------------------------ CLI argument errors
def test_cli_gap2_argument_errors(tmp_path):
    exe = os.path.join(ROOT, "fast-needleman-wunsch_amd", "build", "nw_align")
    g = os.path.join(ROOT, "tests", "golden", "bdna")
    a, b = os.path.join(g, "small1.bdna"), os.path.join(g, "small2.bdna")
    lst = tmp_path / "pairs.txt"
    lst.write_text(f"{a} {b}\n")
    run = lambda *args: subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
    r = run(a, b, "--gap2", "-24,-1")
    assert r.returncode == 1 and "--gap2 needs --batch" in r.stdout
    for other in (["--local"], ["--ends", "3"], ["--band", "5"]):
        r = run("--batch", str(lst), "--gap2", "-24,-1", *other)
        assert r.returncode == 1 and "--gap2" in r.stdout and other[0] in r.stdout, r.stdout
    for bad in ("-24", "x,y", "-24,-1,3", "1,-1", ""):
        r = run("--batch", str(lst), "--gap2", bad)
        assert r.returncode == 1 and "--gap2" in r.stdout, (bad, r.stdout)
    r = run("--batch", str(lst), "--gap2")
    assert r.returncode == 1


# ------------------------------------------------------------------ both pieces matter on the GPU test's grid
@functools.lru_cache(maxsize=None)
def score_want(alpha, pc):
    m = matrix(alpha)
    return np.array([g2.score(a, b, m.scores, m.index, pc) for a, b in score_pairs(alpha)], np.int32)


@functools.lru_cache(maxsize=None)
def single_want(alpha, ge, go):
    m = matrix(alpha)
    return np.array([gm.score(a, b, m.scores, m.index, ge, go) for a, b in score_pairs(alpha)], np.int32)


def piece_mix(alpha, pc):
    """(pairs with both sides >= 64, those of them whose two-piece score differs from BOTH
    single-piece scores)."""
    big = np.array([a.size >= 64 and b.size >= 64 for a, b in score_pairs(alpha)])
    want = score_want(alpha, pc)
    mixed = (want != single_want(alpha, pc[1], pc[0])) & (want != single_want(alpha, pc[3], pc[2]))
    return int(big.sum()), int((mixed & big).sum())


@pytest.mark.parametrize("pc", CROSSING, ids=str)
@pytest.mark.parametrize("alpha", [4, 20, 32])
def test_both_pieces_matter_on_the_grid(alpha, pc):
    """What tests/test_batch_dual.py's score test asserts before it compares: a kernel that
    ignores one piece cannot pass.  More than a third of the 12 pairs with both sides >= 64."""
    big, mixed = piece_mix(alpha, pc)
    assert big == 12 and 3 * mixed > big, (big, mixed)


# ------------------------------------------------------------------ the GPU test's directed pairs
MM = (-4, -2, -24, -1)      # minimap2's -O4,24 -E2,1; the crossover is at k = 20 (a tie)


def uniform():
    return nwhip.SubMatrix.uniform([1, 2, 3, 4], 2, -4)


def planted(left, ins, right, seed, rows=None):
    """x + ins + y against x + y: `ins` columns that only a left run can cross.  The flanks
    are random over 1..3 and the insertion is all 4s, so that no part of it can pair.  rows =
    (at, k): k more letters 4 in s2 after its `at`-th, an up-run of k."""
    rng = np.random.default_rng(seed)
    x, y = _rand(rng, left, 3), _rand(rng, right, 3)
    a = np.concatenate([x, np.full(ins, 4, np.int8), y])
    b = np.concatenate([x, y])
    if rows is not None:
        b = np.concatenate([b[:rows[0]], np.full(rows[1], 4, np.int8), b[rows[0]:]])
    return a, b


RUNS = [(19, 758, 758, 757), (20, 756, 756, 756), (21, 755, 754, 755)]   # (k, two pieces, piece 1 alone, piece 2 alone)


@pytest.mark.parametrize("k,want,one,two", RUNS)
def test_a_run_at_the_crossover_length_on_the_checker(k, want, one, two):
    mat = uniform()
    a, b = planted(150, k, 250, 31)
    assert g2.score(a, b, mat.scores, mat.index, MM) == want == 800 + max(-4 - 2 * k, -24 - k)
    assert gm.score(a, b, mat.scores, mat.index, -2, -4) == one and gm.score(a, b, mat.scores, mat.index, -1, -24) == two


def two_runs_pair():
    """850 x 553: 300 columns planted across the strip seam at column 256, 3 rows further on."""
    return planted(200, 300, 350, 37, rows=(400, 3))


def test_a_long_and_a_short_run_on_the_checker():
    mat = uniform()
    a, b = two_runs_pair()
    assert (a.size, b.size) == (850, 553)
    for s1, s2 in ((a, b), (b, a)):
        sc = mat.scores.T if s1 is b else mat.scores
        assert g2.score(s1, s2, sc, mat.index, MM) == 766
        assert gm.score(s1, s2, sc, mat.index, -2, -4) == 486 and gm.score(s1, s2, sc, mat.index, -1, -24) == 749


# ------------------------------------------------------------------ the coverage list
# Two cost sets with the crossover in the middle of the programs' run lengths (runs of 1 .. 3,
# in the wide set 1 .. 4, are piece 1's, the last by a tie; longer ones piece 2's), so that the walks read H1 .. H4 and
# both values of all four extend bits.  INT8: every s - 2 ge1 fits int8; WIDE: it does not.
COVER = {"int8": _matrix(71, (3, 6), (-14, -11)) + ((-2, -3, -8, -1),),
         "wide": _matrix(72, (100, 120), (-128, -90)) + ((-10, -20, -50, -10),)}
# the greedy pass's result (search(), below) over 1500 candidates, and three more from a pass over the next 4500
# for the three combinations those left unread
KEPT = (
    0, 1, 4, 6, 7, 8, 10, 11, 12, 13, 14, 16, 18, 19, 20, 21, 23, 25, 26, 30, 31, 35, 37, 39, 40, 43, 44, 45,
    47, 48, 49, 52, 53, 56, 60, 61, 62, 63, 64, 66, 67, 68, 72, 73, 74, 75, 76, 77, 79, 81, 82, 93, 95, 97, 98,
    102, 103, 104, 105, 107, 108, 110, 112, 114, 115, 116, 117, 118, 120, 121, 122, 124, 125, 127, 130, 134,
    135, 138, 140, 141, 142, 143, 145, 151, 153, 154, 159, 160, 162, 164, 165, 166, 168, 169, 170, 171, 173,
    175, 177, 179, 180, 181, 182, 186, 187, 188, 189, 190, 191, 193, 195, 196, 201, 202, 203, 204, 205, 209,
    212, 216, 218, 223, 225, 227, 228, 229, 233, 235, 236, 238, 241, 242, 247, 250, 251, 253, 254, 255, 258,
    259, 260, 263, 264, 265, 266, 267, 268, 271, 275, 276, 278, 279, 280, 283, 286, 288, 291, 292, 293, 294,
    295, 297, 300, 302, 305, 306, 308, 312, 313, 315, 316, 317, 320, 322, 324, 325, 326, 327, 328, 329, 336,
    337, 338, 339, 341, 346, 347, 350, 352, 354, 362, 366, 367, 368, 369, 372, 377, 378, 381, 383, 384, 385,
    386, 388, 393, 395, 396, 399, 400, 401, 402, 403, 405, 407, 409, 410, 411, 413, 416, 417, 418, 420, 422,
    423, 424, 426, 427, 429, 430, 431, 432, 434, 436, 437, 438, 440, 442, 443, 445, 446, 447, 449, 451, 453,
    454, 455, 456, 460, 461, 462, 465, 467, 470, 473, 474, 475, 476, 477, 478, 479, 482, 483, 484, 486, 488,
    490, 492, 493, 495, 496, 499, 500, 503, 505, 506, 508, 509, 512, 514, 515, 517, 518, 521, 523, 524, 525,
    530, 531, 532, 533, 538, 539, 542, 543, 545, 546, 548, 550, 551, 553, 558, 563, 564, 565, 567, 569, 570,
    573, 575, 579, 580, 583, 588, 591, 593, 594, 595, 600, 601, 603, 606, 609, 610, 613, 618, 620, 622, 623,
    624, 626, 630, 631, 632, 634, 636, 637, 638, 639, 644, 645, 646, 652, 653, 655, 659, 662, 664, 668, 673,
    675, 678, 682, 684, 687, 688, 690, 692, 695, 698, 707, 709, 714, 719, 720, 723, 724, 725, 729, 730, 732,
    733, 735, 736, 739, 741, 744, 748, 749, 750, 751, 752, 757, 761, 767, 769, 770, 771, 775, 776, 777, 779,
    785, 791, 795, 798, 801, 807, 811, 818, 827, 829, 837, 845, 847, 851, 855, 863, 864, 874, 875, 876, 883,
    884, 885, 886, 890, 901, 905, 910, 918, 920, 922, 925, 937, 938, 944, 947, 977, 978, 988, 993, 994, 996,
    1001, 1014, 1015, 1017, 1026, 1032, 1034, 1038, 1062, 1071, 1076, 1079, 1080, 1082, 1083, 1088, 1093, 1101,
    1105, 1125, 1130, 1145, 1153, 1160, 1184, 1200, 1202, 1212, 1213, 1217, 1218, 1226, 1236, 1254, 1280, 1379,
    1394, 1404, 1419, 1445, 1460, 1514, 1669, 2013)


def candidate(i):
    rng = np.random.default_rng([9, i])
    prog = dm.program(rng)
    shared = bool(rng.random() < 0.35)
    return dm.pair(prog, int(rng.integers(1 << 30)), shared=shared)


Res = collections.namedtuple("Res", "score ops combos")


def evaluate(a, b):
    """{variant: Res}: the checker's score and ops, and the combinations its walk reads."""
    out = {}
    for v, (sc, index, pc) in COVER.items():
        tabs = g2.fill(a, b, sc, index, pc)
        ops = g2.walk(a, b, sc, index, pc, tabs)
        trace = []
        again = dm2.walk_bits(dm2.dual_bits(tabs, gm.sub_table(a, b, sc, index), pc), a.size, b.size, trace)
        assert again.size == ops.size and (again == ops).all()   # the device walk restated gives the checker's ops
        out[v] = Res(int(tabs[0][-1, -1]), ops, dm2.combos(trace, b.size))
    return out


def search(candidates):
    kept, seen = {}, collections.Counter()
    for i in candidates:
        ev = evaluate(*candidate(i))
        keys = {(v, x) for v, r in ev.items() for x in r.combos}
        if any(k not in seen for k in keys):
            kept[i] = keys
            seen.update(keys)
    for i in sorted(kept, key=lambda i: len(kept[i])):
        if all(seen[k] >= 2 for k in kept[i]):
            seen.subtract(kept.pop(i))
    return sorted(kept), {k for k, n in seen.items() if n > 0}


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(candidate(i) for i in KEPT)


@functools.lru_cache(maxsize=None)
def results():
    return tuple(evaluate(a, b) for a, b in cases())


def test_the_cover_forms():
    assert not wide_form(COVER["int8"][0], COVER["int8"][2][1]) and wide_form(COVER["wide"][0], COVER["wide"][2][1])
    for _, _, pc in COVER.values():
        one, two = crossover(pc)
        assert one[0] == 1 and one[-1] in (3, 4) and two[0] == one[-1] + 1
    pairs = cases()
    assert all(1 <= a.size <= 700 and 1 <= b.size <= 330 for a, b in pairs)
    strips = collections.Counter((a.size + 255) // 256 for a, _ in pairs)
    assert min(strips[1], strips[2], strips[3]) >= 1, strips
    assert sum(b.size >= 127 for _, b in pairs) >= 5   # an iteration that is not an edge one exists


@pytest.mark.parametrize("variant", sorted(COVER))
def test_every_instance_is_read_in_every_way(variant):
    """2 variants of the iteration x 64 steps x 4 columns x (5 H sources + 4 extend bits x 2
    values) = 6656 combinations: all of them, no exclusion."""
    read = set().union(*(r[variant].combos for r in results()))
    want = dm2.all_combos()
    assert len(want) == 2 * 64 * 4 * 13
    assert not want - read, sorted(want - read)[:20]


@pytest.mark.parametrize("variant", sorted(COVER))
def test_cover_path_score_is_the_score(variant):
    sc, index, pc = COVER[variant]
    for (a, b), r in zip(cases(), results()):
        assert g2.path_score(a, b, r[variant].ops, sc, index, pc) == r[variant].score


if __name__ == "__main__":
    import textwrap
    kept, seen = search(list(range(1500)) + [1514, 1669, 2013])
    for v in COVER:
        print("#", v, len({x for w, x in seen if w == v}), "of", len(dm2.all_combos()))
    print("KEPT = (")
    print(textwrap.fill(", ".join(str(i) for i in kept), 112, initial_indent=" " * 4, subsequent_indent=" " * 4) + ")")
