"""CPU: the host side of the batched alignment with a substitution matrix
(nw_score_batch_matrix, nw_align_batch_matrix, nw_score_batch_matrix_async,
nw_ops_score_matrix, nw_submat; include/nw_hip.h) and nwhip.SubMatrix.

The checker of tests/nw_gotoh_matrix.py against the merged one (tests/nw_gotoh.py) on
identity-type matrices and against its own literal fill on asymmetric ones,
nw_ops_score_matrix against the checker's direct summation, every new refusal and its
place in the order -- all answered without a device, NW_ERR_NODEVICE last -- the struct
size and the text format.
"""
import ctypes
import itertools

import numpy as np
import pytest

import nw_gotoh
import nw_gotoh_matrix as gm
import nwhip
from test_batch_host import ALIGN_REFUSALS, ARG_REFUSALS, PARAM_REFUSALS, VALID, Call, _i8p, _i32p, _i64p, _u8p

SCHEMES = [(1, 0, -1), (1, -1, -1), (2, -1, -2), (2, -1, 0)]
SHAPES = [(1, 1), (5, 3), (3, 5), (17, 9), (40, 33), (64, 70)]


def identity_matrix(letters, match, mismatch, other=None):
    """match on the diagonal, mismatch elsewhere: byte equality over `letters`."""
    n = len(letters)
    sc = np.full((n, n), mismatch, np.int64)
    sc[np.arange(n), np.arange(n)] = match
    return nwhip.SubMatrix(letters, sc, other)


def random_matrix(rng, n, lo=-8, hi=12, letters=None, other=None):
    """A seeded asymmetric n-letter matrix over the bytes 1..n."""
    letters = list(range(1, n + 1)) if letters is None else letters
    return nwhip.SubMatrix(letters, rng.integers(lo, hi + 1, (n, n)), other)


def _pair(rng, n1, n2, alpha=4):
    return rng.integers(1, alpha + 1, n1).astype(np.int8), rng.integers(1, alpha + 1, n2).astype(np.int8)


class MatrixCall(Call):
    """test_batch_host.Call through the matrix entries."""

    def __init__(self, gap_open=-3, mat="default"):
        super().__init__()
        self.go = gap_open
        self.m = identity_matrix([1, 2, 3, 4], 1, 0, other=1).c if isinstance(mat, str) else mat

    def _m(self):
        return ctypes.byref(self.m) if self.m is not None else None

    def _p(self):
        return ctypes.byref(self.p) if self.p is not None else None

    def score(self):
        return nwhip.lib().nw_score_batch_matrix(
            self._ptr("s1", self.s1, _i8p), self._ptr("off1", self.off1, _i64p), self._ptr("s2", self.s2, _i8p),
            self._ptr("off2", self.off2, _i64p), self.npairs, self._p(), self._m(), self.go,
            self._ptr("scores", self.scores, _i32p), None)

    def align(self):
        return nwhip.lib().nw_align_batch_matrix(
            self._ptr("s1", self.s1, _i8p), self._ptr("off1", self.off1, _i64p), self._ptr("s2", self.s2, _i8p),
            self._ptr("off2", self.off2, _i64p), self.npairs, self._p(), self._m(), self.go,
            ctypes.byref(self.o) if self.o is not None else None, self._ptr("scores", self.scores, _i32p),
            self._ptr("ops", self.ops, _u8p), self._ptr("ops_off", self.ops_off, _i64p),
            self._ptr("n_ops", self.n_ops, _i64p), None)

    def score_async(self):
        return nwhip.lib().nw_score_batch_matrix_async(
            None, self.s1.ctypes.data, self.off1.ctypes.data, self.s2.ctypes.data, self.off2.ctypes.data,
            self.npairs, int(self.off1[-1]), int(self.off2[-1]), 5, self._p(), self._m(), self.go,
            self.scores.ctypes.data, None)


# ------------------------------------------------------------------ the checker itself
@pytest.mark.parametrize("scheme", SCHEMES)
def test_checker_on_identity_matrices_is_the_merged_checker(scheme):
    """Score, the three tables and the ops, on a dozen small pairs."""
    rng = np.random.default_rng(31)
    mat = identity_matrix([1, 2, 3, 4], scheme[0], scheme[1])
    shapes = SHAPES + [(0, 4), (4, 0), (0, 0), (9, 31), (33, 2), (20, 20)]
    assert len(shapes) == 12
    for (n1, n2), go in itertools.product(shapes, (0, -1, -3, -11)):
        a, b = _pair(rng, n1, n2)
        want = nw_gotoh.fill(a, b, scheme, go)
        got = gm.fill(a, b, mat.scores, mat.index, scheme[2], go)
        for x, y in zip(got, want):
            fin = y > nw_gotoh.NEG // 2
            np.testing.assert_array_equal(x[fin], y[fin])
            assert (x[~fin] < gm.MINF // 2).all()
        assert gm.score(a, b, mat.scores, mat.index, scheme[2], go) == nw_gotoh.score(a, b, scheme, go)
        ops = gm.walk(a, b, mat.scores, mat.index, scheme[2], go, got)
        np.testing.assert_array_equal(ops, nw_gotoh.walk(a, b, scheme, go, want))
        assert gm.path_score(a, b, ops, mat.scores, mat.index, scheme[2], go) == \
            nw_gotoh.path_score_affine(a, b, ops, scheme, go) == want[0][-1, -1]


@pytest.mark.parametrize("ge", [-1, -2, 0, 1])
def test_checker_row_fill_equals_the_literal_fill(ge):
    rng = np.random.default_rng(32)
    for (n1, n2), go in itertools.product(SHAPES + [(0, 4), (4, 0), (0, 0)], (0, -1, -5, -11)):
        mat = random_matrix(rng, 6, -9, 9)
        assert (mat.scores != mat.scores.T).any()
        a, b = _pair(rng, n1, n2, 6)
        for x, y in zip(gm.fill(a, b, mat.scores, mat.index, ge, go),
                        gm.fill_cells(a, b, mat.scores, mat.index, ge, go)):
            fin = y > gm.MINF // 2
            np.testing.assert_array_equal(x[fin], y[fin])
            assert (x[~fin] < gm.MINF // 2).all()


def test_checker_first_index_is_the_s1_letter():
    mat = nwhip.SubMatrix([1, 2], [[0, 7], [-7, 0]])
    # one cell: s1 = letter 0 (byte 1), s2 = letter 1 (byte 2) -> mat[0][1]
    assert gm.score([1], [2], mat.scores, mat.index, -100, -100) == 7
    assert gm.score([2], [1], mat.scores, mat.index, -100, -100) == -7


# ------------------------------------------------------------------ nw_ops_score_matrix
def test_ops_score_matrix_is_the_direct_sum():
    rng = np.random.default_rng(33)
    for (n1, n2), go, ge in itertools.product(SHAPES + [(0, 4), (4, 0)], (0, -1, -11), (-1, -3)):
        mat = random_matrix(rng, 20)
        a, b = _pair(rng, n1, n2, 20)
        tables = gm.fill(a, b, mat.scores, mat.index, ge, go)
        ops = gm.walk(a, b, mat.scores, mat.index, ge, go, tables)
        want = gm.path_score(a, b, ops, mat.scores, mat.index, ge, go)
        assert want == tables[0][-1, -1]  # the walk's path is an optimal one
        assert nwhip.ops_score_matrix(a, b, ops, mat, ge, go) == want
    # asymmetric, by hand: s1 = [1, 2], s2 = [2, 1, 1]; diag, up, diag
    mat = nwhip.SubMatrix([1, 2], [[3, 7], [-7, 5]])
    assert nwhip.ops_score_matrix([1, 2], [2, 1, 1], [0, 1, 0], mat, -1, -10) == 7 - 11 - 7
    assert nwhip.ops_score_matrix([1, 2], [2, 1, 1], [1, 1, 2, 0], mat, -1, -10) == 2 * -10 - 3 - 7
    assert nwhip.ops_score_matrix([1, 2], [2, 1], [], mat, -1, -10, begin=(2, 2)) == 0
    # an identity matrix: nw_ops_score_affine
    ident = identity_matrix([1, 2, 3, 4], 2, -1)
    a, b = _pair(rng, 40, 33)
    ops = nw_gotoh.walk(a, b, (2, -1, -2), -3)
    assert nwhip.ops_score_matrix(a, b, ops, ident, -2, -3) == nwhip.ops_score_affine(a, b, ops, (2, -1, -2), -3)


def test_ops_score_matrix_refusals():
    mat = identity_matrix([1, 2, 3], 1, 0, other=1)
    a, b = np.array([1, 2], np.int8), np.array([1, 2, 3], np.int8)
    for ops in ([3], [0, 0, 0], [2, 2, 2], [1, 1, 1, 1]):
        with pytest.raises(nwhip.NwError) as e:
            nwhip.ops_score_matrix(a, b, ops, mat, -1, -3)
        assert e.value.status == nwhip.NW_ERR_ARG
    with pytest.raises(nwhip.NwError):
        nwhip.ops_score_matrix(a, b, [0], mat, -1, -3, begin=(4, 0))
    f = nwhip.lib().nw_ops_score_matrix
    o = np.zeros(1, np.uint8)
    sc = ctypes.c_int64()
    p = nwhip.params()
    args = (a.ctypes.data_as(_i8p), 2, b.ctypes.data_as(_i8p), 3, 0, 0, o.ctypes.data_as(_u8p), 1)
    m = ctypes.byref(mat.c)
    assert f(*args, None, m, -3, ctypes.byref(sc)) == nwhip.NW_ERR_ARG
    assert f(*args, ctypes.byref(p), None, -3, ctypes.byref(sc)) == nwhip.NW_ERR_ARG
    assert f(*args, ctypes.byref(p), m, -3, None) == nwhip.NW_ERR_ARG
    assert f(*args, ctypes.byref(p), m, -3, ctypes.byref(sc)) == nwhip.NW_OK and sc.value == 1
    for bad in _bad_matrices():
        assert f(*args, ctypes.byref(p), ctypes.byref(bad), -3, ctypes.byref(sc)) == nwhip.NW_ERR_ARG


# ------------------------------------------------------------------ the struct
def test_submat_layout():
    assert nwhip.SUBMAT_MAX == 32
    assert ctypes.sizeof(nwhip.NwSubmat) == 16 + 256 + 1024
    assert nwhip.NwSubmat.index.offset == 16 and nwhip.NwSubmat.score.offset == 272
    mat = nwhip.SubMatrix([5, 6, 7], [[1, 2, 3], [4, 5, 6], [7, 8, -9]], other=6)
    assert mat.c.n == 3 and list(mat.c.reserved) == [0, 0, 0]
    assert mat.c.index[5] == 0 and mat.c.index[7] == 2 and mat.c.index[0] == mat.c.index[255] == 1
    assert mat.c.score[0 * 32 + 2] == 3 and mat.c.score[2 * 32 + 0] == 7 and mat.c.score[2 * 32 + 2] == -9
    assert mat.c.score[3] == 0 and mat.c.score[3 * 32] == 0


# ------------------------------------------------------------------ refusals
def _copy(m):
    c = nwhip.NwSubmat()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(m), ctypes.sizeof(c))
    return c


def _bad_matrices():
    good = identity_matrix([1, 2, 3, 4], 1, 0, other=1).c
    out = []
    for n in (0, 33, -1):
        m = _copy(good)
        m.n = n
        out.append(m)
    for b in (0, 200, 255):  # an index entry = n
        m = _copy(good)
        m.index[b] = 4
        out.append(m)
    for k in range(3):
        m = _copy(good)
        m.reserved[k] = 1
        out.append(m)
    return out


def test_matrix_refusals_need_no_device():
    for m in _bad_matrices() + [None]:
        c = MatrixCall(mat=m)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
        # before NW_KERNEL_PANELS' NW_ERR_UNSUPPORTED
        c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
        # and before the offsets are looked at: an empty batch with NULL arrays is refused too
        c = MatrixCall(mat=m)
        c.npairs = 0
        c.null = {"s1", "s2", "off1", "off2", "scores", "ops", "ops_off", "n_ops"}
        assert c.score() == c.align() == nwhip.NW_ERR_ARG
    # n = 32 and n = 1 are valid
    for n in (1, 32):
        m = identity_matrix(list(range(1, n + 1)), 1, 0, other=1).c
        c = MatrixCall(mat=m)
        assert c.score() in VALID and c.align() in VALID
    # entries at or beyond n are ignored, whatever they hold
    m = _copy(identity_matrix([1, 2, 3, 4], 1, 0, other=1).c)
    m.score[5] = -128
    m.score[31 * 32 + 31] = 127
    c = MatrixCall(-((2 ** 28 - 1 - 2 * 12) // 3), mat=m)  # at the edge for M = 1
    assert c.score() in VALID and c.align() in VALID


def test_range_bound_at_its_edge():
    """3 |go| + (M + |gap|) * (n1 + n2 + 2) < 2^28 with M = 128 from one entry of -128: the
    longest pair of the batch is 5 x 5, and one more character tips it."""
    sc = np.zeros((4, 4), np.int64)
    sc[2, 1] = -128
    m = nwhip.SubMatrix([1, 2, 3, 4], sc, other=1).c
    go = -((2 ** 28 - 1 - 129 * 12) // 3)
    assert 3 * -go + 129 * 12 < 2 ** 28 <= 3 * -go + 129 * 13
    c = MatrixCall(go, mat=m)
    assert c.score() in VALID and c.align() in VALID
    c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
    assert c.score() == c.align() == nwhip.NW_ERR_UNSUPPORTED  # the range passed
    c = MatrixCall(go, mat=m)  # 6 x 5
    c.off1[:] = [0, 4, 4, 10]
    c.s1 = np.ones(10, np.int8)
    c.ops_off[:] = [0, 7, 9, 20]
    c.ops = np.zeros(20, np.uint8)
    assert c.score() == c.align() == nwhip.NW_ERR_ARG
    assert MatrixCall(go - 1, mat=m).score() == nwhip.NW_ERR_ARG
    # the entry counts only below n: the same matrix with n = 2 has M = |gap| = 1
    m2 = _copy(m)
    m2.n = 2
    for b in range(256):
        m2.index[b] = min(m2.index[b], 1)
    c = MatrixCall(go - 1, mat=m2)
    assert c.score() in VALID
    # |gap| above the largest entry: M = |gap|
    c = MatrixCall(go, mat=m)
    c.p = nwhip.params((1, 0, -200))
    assert 3 * -go + 400 * 12 >= 2 ** 28 and c.score() == nwhip.NW_ERR_ARG
    # the async form checks n1 = 0, n2 = max_n2 = 5: 3 |go| + 129 * 7
    go = -((2 ** 28 - 1 - 129 * 7) // 3)
    c = MatrixCall(go, mat=m)
    c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
    assert c.score_async() == nwhip.NW_ERR_UNSUPPORTED
    c.go = go - 1
    assert c.score_async() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("case", sorted(PARAM_REFUSALS))
def test_param_refusals_need_no_device(case):
    """match / mismatch are not used, but the parameters must still be valid."""
    kw, want = PARAM_REFUSALS[case]
    c = MatrixCall()
    c.p = nwhip.params(**kw)
    assert c.score() == want
    assert c.align() == want
    assert c.score_async() == want


@pytest.mark.parametrize("case", sorted(ARG_REFUSALS))
def test_batch_refusals_need_no_device(case):
    c = MatrixCall()
    ARG_REFUSALS[case](c)
    assert c.score() == nwhip.NW_ERR_ARG
    assert c.align() == nwhip.NW_ERR_ARG
    if case != "w_range":
        c.p = nwhip.params(kernel=nwhip.KERNEL_PANELS)
        assert c.score() == nwhip.NW_ERR_ARG
        assert c.align() == nwhip.NW_ERR_ARG


@pytest.mark.parametrize("case", sorted(ALIGN_REFUSALS))
def test_align_batch_refusals_need_no_device(case):
    c = MatrixCall()
    ALIGN_REFUSALS[case](c)
    assert c.align() == nwhip.NW_ERR_ARG


def test_gap_open_and_async_refusals_need_no_device():
    for go in (1, 7, 2 ** 31 - 1):
        c = MatrixCall(go)
        assert c.score() == c.align() == c.score_async() == nwhip.NW_ERR_ARG
    c = MatrixCall()
    f = nwhip.lib().nw_score_batch_matrix_async
    a = (c.s1.ctypes.data, c.off1.ctypes.data, c.s2.ctypes.data, c.off2.ctypes.data)
    p, m = ctypes.byref(c.p), ctypes.byref(c.m)
    sc = c.scores.ctypes.data
    assert f(None, *a, -1, 9, 10, 5, p, m, -3, sc, None) == nwhip.NW_ERR_ARG     # npairs < 0
    assert f(None, *a, 3, -1, 10, 5, p, m, -3, sc, None) == nwhip.NW_ERR_ARG     # total1 < 0
    assert f(None, *a, 3, 9, 10, 11, p, m, -3, sc, None) == nwhip.NW_ERR_ARG     # max_n2 > total2
    assert f(None, *a, 3, 9, 10, 5, None, m, -3, sc, None) == nwhip.NW_ERR_ARG   # p == NULL
    assert f(None, *a, 3, 9, 10, 5, p, None, -3, sc, None) == nwhip.NW_ERR_ARG   # m == NULL
    assert f(None, *a, 3, 9, 10, 5, p, m, -3, sc, None) == nwhip.NW_ERR_ARG      # valid, but no context


@pytest.mark.parametrize("defaults", [True, False])
def test_valid_arguments_reach_the_device(defaults):
    c = MatrixCall(0 if defaults else -11)
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
    c = MatrixCall()
    c.off1[:] = 0
    c.off2[:] = [0, 3, 5, 10]
    c.null = {"s1"}
    assert c.score() in VALID
    assert c.align() in VALID


def test_python_wrappers_without_a_device():
    mat = identity_matrix([1, 2, 3], 1, -1)
    # an unlisted byte without other=: refused before the library is asked
    for f in (nwhip.score_batch_matrix, nwhip.align_batch_matrix):
        with pytest.raises(ValueError):
            f([([1, 2, 3], [1, 4])], mat, -1, -3)
    with pytest.raises(ValueError):
        nwhip.ops_score_matrix([1, 2], [1, 9], [0, 0], mat, -1, -3)
    if VALID == (nwhip.NW_OK,):
        return  # (with a device the wrappers are tests/test_batch_matrix.py's)
    for f in (nwhip.score_batch_matrix, nwhip.align_batch_matrix):
        with pytest.raises(nwhip.NwError) as e:
            f([([1, 2, 3], [1, 2])], mat, -1, -3)
        assert e.value.status == nwhip.NW_ERR_NODEVICE
        with pytest.raises(nwhip.NwError) as e:
            f([([1, 2, 3], [1, 2])], mat, -1, 1)
        assert e.value.status == nwhip.NW_ERR_ARG


# ------------------------------------------------------------------ SubMatrix and its text format
TEXT = """# a comment
#  another, then a blank line

   A  R  N  *
A  4 -1 -2 -4
R -1  5  0 -4
# a comment between rows
N -2  1  6 -4
* -4 -4 -4  1
"""


def test_submatrix_construction():
    m = nwhip.SubMatrix("AC", [[1, -1], [-2, 1]])
    assert m.n == 2 and m.letters == [65, 67] and m.other is None
    assert m.index[ord("C")] == 1 and m.index[ord("c")] == 1 and m.listed[ord("a")] and not m.listed[ord("G")]
    assert nwhip.SubMatrix(b"AC", [[1, -1], [-2, 1]]).letters == [65, 67]
    # explicitly letter 0 for everything unlisted
    m = nwhip.SubMatrix("AC", [[1, -1], [-2, 1]], other="A")
    assert m.index[ord("G")] == 0 and m.index[200] == 0 and m.index[ord("C")] == 1
    # a listed lower-case letter is its own
    m = nwhip.SubMatrix("Aa", [[1, -1], [-2, 1]])
    assert m.index[ord("a")] == 1
    for bad in [("AA", [[1, 1], [1, 1]], None), ("AC", [[1, 1, 1], [1, 1, 1]], None), ("AC", [[1, 128], [1, 1]], None),
                ("AC", [[1, -129], [1, 1]], None), ("AC", [[1, 1], [1, 1]], "G"), ("", np.zeros((0, 0), int), None),
                ("AC", [[1.5, 1], [1, 1]], None), (list(range(33)), np.zeros((33, 33), int), None)]:
        with pytest.raises(ValueError):
            nwhip.SubMatrix(*bad)


def test_from_text_round_trip(tmp_path):
    m = nwhip.SubMatrix.from_text(TEXT)
    assert m.letters == [ord(c) for c in "ARN*"]
    assert m.scores.tolist() == [[4, -1, -2, -4], [-1, 5, 0, -4], [-2, 1, 6, -4], [-4, -4, -4, 1]]
    assert m.scores[2, 1] == 1 and m.scores[1, 2] == 0  # row letter first
    # the '*' column is the wildcard unless other= names one
    assert m.other == ord("*") and m.index[ord("Z")] == 3 and m.index[0] == 3
    assert m.index[ord("r")] == 1 and m.index[ord("n")] == 2  # lower case like upper case
    m = nwhip.SubMatrix.from_text(TEXT, other="A")
    assert m.index[ord("Z")] == 0 and m.index[ord("*")] == 3
    path = tmp_path / "m.txt"
    path.write_text(TEXT)
    m2 = nwhip.SubMatrix.from_text(str(path))
    assert m2.scores.tolist() == m.scores.tolist() and m2.letters == m.letters
    # without a wildcard an unlisted byte raises where sequences are looked at
    strict = nwhip.SubMatrix.from_text("A C\nA 1 -1\nC -1 1\n")
    assert strict.other is None
    strict.check(b"ACca", [65, 67])
    with pytest.raises(ValueError):
        strict.check(b"ACG")
    # byte values as letters
    m = nwhip.SubMatrix.from_text("0x01 0x02 0xfe\n0x01 1 2 3\n0x02 4 5 6\n0xfe 7 8 9\n", other="0xfe")
    assert m.letters == [1, 2, 254] and m.index[9] == 2 and m.scores[2, 0] == 7
    for bad in ["A C\nA 1 -1\nC -1 128\n",          # outside int8
                "A C\nA 1 -1\nC -1 -129\n",
                "A C\nA 1 -1\n",                     # a row missing
                "A C\nA 1 -1\nA -1 1\n",             # a row twice
                "A C\nA 1 -1\nG -1 1\n",             # a row of no header letter
                "A C\nA 1 -1 0\nC -1 1 0\n",         # too many numbers
                "A C\nA 1 x\nC -1 1\n",              # not a number
                "A A\nA 1 -1\nA -1 1\n",             # a letter twice
                "AB C\nAB 1 -1\nC -1 1\n",           # not a letter
                "# nothing\n\n"]:
        with pytest.raises(ValueError):
            nwhip.SubMatrix.from_text(bad)
