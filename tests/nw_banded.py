"""Plain Python banded Gotoh with substitution by matrix -- the checker of the banded batch
entries (tests/test_batch_banded.py, tests/test_batch_banded_host.py).  A helper, not a
conftest; nothing here touches the library.  Written apart from the other checkers: only
sub_table comes from tests/nw_gotoh_matrix.py.

The definition of include/nw_hip.h: with n1 columns (s1), n2 rows (s2) and band w,
    delta = n2 - n1, dlo = min(0, delta) - w, dhi = max(0, delta) + w
    cell (i, j), 0 <= i <= n2, 0 <= j <= n1, is in the band iff dlo <= i - j <= dhi
    H, E, F outside the band are -inf; inside:
    E[i][j] = max(E[i][j-1] + ge, H[i][j-1] + go + ge)
    F[i][j] = max(F[i-1][j] + ge, H[i-1][j] + go + ge)
    H[i][j] = max(H[i-1][j-1] + sub[i-1][j-1], F[i][j], E[i][j])
    H[0][0] = 0, H[0][j] = go + j*ge, H[i][0] = go + i*ge, E[i][0] = F[0][j] = -inf

Every fill takes `band`, or an explicit (dlo, dhi) in its place, so that a test can move
one edge of the band by one diagonal.

fill_cells(): those lines, cell by cell.
fill():       a row at a time.  The in-band columns of a row are one interval, and within a
              row only E looks left: E[j] = max over the in-band k < j of H[k] + go + (j -
              k)*ge, where H[k] may be replaced by max(diag[k], F[k]) (a k whose H came from
              E[k] is dominated by the k' that opened E[k]: go <= 0) -- one running maximum.
walk():       the three-state machine of include/nw_hip.h from (n2, n1) to (0, 0); it
              asserts that every vertex is in the band.
"""
import numpy as np

from nw_gotoh_matrix import sub_table

MINF = -(1 << 44)  # minus infinity for int64 tables; a finite value is above MINF // 2


def limits(n1, n2, band):
    """(dlo, dhi) of a pair under the call's band."""
    assert band >= 0
    delta = n2 - n1
    return min(0, delta) - band, max(0, delta) + band


def in_band(i, j, dlo, dhi):
    return dlo <= i - j <= dhi


def _limits(n1, n2, band, dlo, dhi):
    if band is not None:
        assert dlo is None and dhi is None
        return limits(n1, n2, band)
    return dlo, dhi


def fill_cells(s1, s2, mat, index, ge, go, band=None, dlo=None, dhi=None):
    n1, n2 = len(s1), len(s2)
    dlo, dhi = _limits(n1, n2, band, dlo, dhi)
    sub = sub_table(s1, s2, mat, index)
    H = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    E = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    F = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    for i in range(n2 + 1):
        for j in range(n1 + 1):
            if not in_band(i, j, dlo, dhi):
                continue
            if i == 0 or j == 0:
                H[i, j] = 0 if i == j else go + (i + j) * ge
                continue
            E[i, j] = max(MINF, E[i, j - 1] + ge, H[i, j - 1] + go + ge)
            F[i, j] = max(MINF, F[i - 1, j] + ge, H[i - 1, j] + go + ge)
            H[i, j] = max(MINF, H[i - 1, j - 1] + sub[i - 1, j - 1], F[i, j], E[i, j])
    return H, E, F


def fill(s1, s2, mat, index, ge, go, band=None, dlo=None, dhi=None):
    """(H, E, F), int64 arrays of (n2 + 1, n1 + 1); -inf cells hold values below MINF // 2."""
    assert go <= 0
    n1, n2 = len(s1), len(s2)
    dlo, dhi = _limits(n1, n2, band, dlo, dhi)
    H = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    E = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    F = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    j = np.arange(n1 + 1, dtype=np.int64)
    rows = np.arange(n2 + 1, dtype=np.int64)
    H[0] = np.where(j == 0, 0, go + j * ge)
    H[:, 0] = np.where(rows == 0, 0, go + rows * ge)
    H[0, (-j < dlo) | (-j > dhi)] = MINF
    H[(rows < dlo) | (rows > dhi), 0] = MINF
    if n1 == 0 or n2 == 0:
        return H, E, F
    sub = sub_table(s1, s2, mat, index)
    for i in range(1, n2 + 1):
        out = (i - j < dlo) | (i - j > dhi)
        F[i, 1:] = np.maximum(F[i - 1, 1:], H[i - 1, 1:] + go) + ge
        best = np.empty(n1 + 1, np.int64)  # what a left run may open from: column 0, else max(diag, F)
        best[0] = H[i, 0]
        best[1:] = np.maximum(H[i - 1, :-1] + sub[i - 1], F[i, 1:])
        best[out] = MINF
        opened = np.maximum.accumulate(best - j * ge)  # max over k <= j of best[k] - k*ge
        E[i, 1:] = opened[:-1] + go + j[1:] * ge
        H[i, 1:] = np.maximum(best[1:], E[i, 1:])
        for T in (H, E, F):
            T[i, out] = MINF
            T[i, T[i] < MINF // 2] = MINF  # (sums of -inf: -inf again, so that nothing accumulates)
    return H, E, F


def score(s1, s2, mat, index, ge, go, band=None, dlo=None, dhi=None) -> int:
    return int(fill(s1, s2, mat, index, ge, go, band, dlo, dhi)[0][-1, -1])


def walk(s1, s2, mat, index, ge, go, band=None, dlo=None, dhi=None, tables=None) -> np.ndarray:
    """Ops in path order (0, 0) -> (n2, n1): 0 diag, 1 up, 2 left."""
    n1, n2 = len(s1), len(s2)
    dlo, dhi = _limits(n1, n2, band, dlo, dhi)
    H, E, F = tables if tables is not None else fill(s1, s2, mat, index, ge, go, dlo=dlo, dhi=dhi)
    sub = sub_table(s1, s2, mat, index) if n1 and n2 else None
    i, j = n2, n1
    out = []
    state = 0  # 0 H, 1 F, 2 E
    while i or j:
        assert in_band(i, j, dlo, dhi) and H[i, j] > MINF // 2, (i, j)
        if state == 0:
            if i == 0 or j == 0:
                op = 2 if i == 0 else 1
                out.append(op)
                i -= op == 1
                j -= op == 2
            elif H[i, j] == H[i - 1, j - 1] + sub[i - 1, j - 1]:
                out.append(0)
                i -= 1
                j -= 1
            elif H[i, j] == F[i, j]:
                state = 1
            else:
                assert H[i, j] == E[i, j], (i, j)
                state = 2
        elif state == 1:
            assert F[i, j] > MINF // 2
            out.append(1)
            state = 0 if F[i, j] == H[i - 1, j] + go + ge else 1  # opening wins a tie over extending
            i -= 1
        else:
            assert E[i, j] > MINF // 2
            out.append(2)
            state = 0 if E[i, j] == H[i, j - 1] + go + ge else 2
            j -= 1
    assert state == 0
    return np.array(out[::-1], np.uint8)


def path_vertices(ops):
    """The vertices (i, j) of a path from (0, 0), the first included."""
    i = j = 0
    v = [(0, 0)]
    for op in ops:
        i += op != 2
        j += op != 1
        v.append((i, j))
    return v


def path_score(s1, s2, ops, mat, index, ge, go) -> int:
    """Score of a global path by direct summation: the matrix entry per diag, ge per up or
    left, go for every run of ups and every run of lefts."""
    mat = np.asarray(mat, np.int64)
    a = np.asarray(s1, np.int8).view(np.uint8)
    b = np.asarray(s2, np.int8).view(np.uint8)
    i = j = total = 0
    last = 0
    for op in ops:
        if op == 0:
            total += int(mat[index[a[j]], index[b[i]]])
            i += 1
            j += 1
        else:
            total += ge + (go if op != last else 0)
            i += op == 1
            j += op == 2
        last = op
    assert (i, j) == (len(b), len(a))
    return total
