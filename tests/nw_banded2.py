"""Plain Python global alignment with a substitution matrix under a TWO-PIECE affine gap cost
inside a BAND of diagonals -- the checker of the nw_*_batch_dual_banded entries (tests/
test_batch_dual_banded.py, tests/test_batch_dual_banded_host.py).  A helper, not a conftest;
nothing here touches the library.  Written apart from the other checkers: only sub_table comes
from tests/nw_gotoh_matrix.py.

The definition of include/nw_hip.h.  A run of k ups or of k lefts costs g(k) = max(go1 + k*ge1,
go2 + k*ge2); `pc` is (go1, ge1, go2, ge2).  With n1 columns (s1), n2 rows (s2) and band w,
    delta = n2 - n1, dlo = min(0, delta) - w, dhi = max(0, delta) + w
    cell (i, j), 0 <= i <= n2, 0 <= j <= n1, is in the band iff dlo <= i - j <= dhi
    H, E_1, E_2, F_1, F_2 outside the band are -inf; inside:
    E_t[i][j] = max(E_t[i][j-1] + ge_t, H[i][j-1] + go_t + ge_t)      t = 1, 2
    F_t[i][j] = max(F_t[i-1][j] + ge_t, H[i-1][j] + go_t + ge_t)
    H[i][j]   = max(H[i-1][j-1] + sub[i-1][j-1], F_1, E_1, F_2, E_2)
    H[0][0] = 0, H[0][j] = g(j), H[i][0] = g(i), E_t[i][0] = F_t[0][j] = -inf

Every fill takes `band`, or an explicit (dlo, dhi) in its place, so that a test can move one
edge of the band by one diagonal.

fill_cells(): those lines, cell by cell.
fill():       a row at a time.  The in-band columns of a row are one interval, and within a row
              only the E_t look left.  First H: max(E_1, E_2)[j] is the maximum over the in-band
              k < j and both pieces of H[k] + go_t + (j - k)*ge_t, where H[k] may be replaced by
              max(diag[k], F_1[k], F_2[k]) (a k whose H came from a left run opened at k' is
              dominated by k' itself under one of the pieces: g(a) + g(b) <= g(a + b), and k' is
              in the band when k and j are).  The exact E_t, which the walk's "opening wins"
              test reads, then come from the exact H by the same accumulate, once per piece.
walk():       the five-state machine of include/nw_hip.h from (n2, n1) to (0, 0); it asserts
              that every vertex is in the band.
path_score(): the direct sum over the ops, the better piece per maximal run.
brute():      every monotone path of a tiny pair; those inside the band, priced by g.
"""
import numpy as np

from nw_gotoh_matrix import sub_table

MINF = -(1 << 44)  # minus infinity for int64 tables; a finite value is above MINF // 2


def gap(pc, k):
    """g(k), k >= 1 (numbers or arrays)."""
    go1, ge1, go2, ge2 = pc
    return np.maximum(go1 + k * ge1, go2 + k * ge2)


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


def fill_cells(s1, s2, mat, index, pc, band=None, dlo=None, dhi=None):
    """(H, E1, F1, E2, F2), int64 arrays of (n2 + 1, n1 + 1); -inf is MINF exactly."""
    go1, ge1, go2, ge2 = pc
    n1, n2 = len(s1), len(s2)
    dlo, dhi = _limits(n1, n2, band, dlo, dhi)
    sub = sub_table(s1, s2, mat, index) if n1 and n2 else None
    H, E1, F1, E2, F2 = (np.full((n2 + 1, n1 + 1), MINF, np.int64) for _ in range(5))
    for i in range(n2 + 1):
        for j in range(n1 + 1):
            if not in_band(i, j, dlo, dhi):
                continue
            if i == 0 or j == 0:
                H[i, j] = 0 if i == j else int(gap(pc, i + j))
                continue
            E1[i, j] = max(MINF, E1[i, j - 1] + ge1, H[i, j - 1] + go1 + ge1)
            E2[i, j] = max(MINF, E2[i, j - 1] + ge2, H[i, j - 1] + go2 + ge2)
            F1[i, j] = max(MINF, F1[i - 1, j] + ge1, H[i - 1, j] + go1 + ge1)
            F2[i, j] = max(MINF, F2[i - 1, j] + ge2, H[i - 1, j] + go2 + ge2)
            H[i, j] = max(MINF, H[i - 1, j - 1] + sub[i - 1, j - 1], F1[i, j], E1[i, j], F2[i, j], E2[i, j])
    for T in (H, E1, F1, E2, F2):
        T[T < MINF // 2] = MINF  # (sums of -inf: -inf again)
    return H, E1, F1, E2, F2


def fill(s1, s2, mat, index, pc, band=None, dlo=None, dhi=None):
    """fill_cells() a row at a time: all five tables exact, -inf cells hold MINF."""
    go1, ge1, go2, ge2 = pc
    assert go1 <= 0 and go2 <= 0
    n1, n2 = len(s1), len(s2)
    dlo, dhi = _limits(n1, n2, band, dlo, dhi)
    H, E1, F1, E2, F2 = (np.full((n2 + 1, n1 + 1), MINF, np.int64) for _ in range(5))
    j = np.arange(n1 + 1, dtype=np.int64)
    rows = np.arange(n2 + 1, dtype=np.int64)
    H[0] = np.where(j == 0, 0, gap(pc, j))
    H[:, 0] = np.where(rows == 0, 0, gap(pc, rows))
    H[0, (-j < dlo) | (-j > dhi)] = MINF
    H[(rows < dlo) | (rows > dhi), 0] = MINF
    if n1 == 0 or n2 == 0:
        return H, E1, F1, E2, F2
    sub = sub_table(s1, s2, mat, index)

    def lefts(src, go, ge):  # [j >= 1]: max over k < j of src[k] + go + (j - k) * ge
        return np.maximum.accumulate(src - j * ge)[:-1] + go + j[1:] * ge

    for i in range(1, n2 + 1):
        out = (i - j < dlo) | (i - j > dhi)
        F1[i, 1:] = np.maximum(F1[i - 1, 1:], H[i - 1, 1:] + go1) + ge1
        F2[i, 1:] = np.maximum(F2[i - 1, 1:], H[i - 1, 1:] + go2) + ge2
        best = np.empty(n1 + 1, np.int64)  # what a left run need open from: column 0, else max(diag, F_1, F_2)
        best[0] = H[i, 0]
        best[1:] = np.maximum(H[i - 1, :-1] + sub[i - 1], np.maximum(F1[i, 1:], F2[i, 1:]))
        best[out] = MINF
        H[i, 1:] = np.maximum(best[1:], np.maximum(lefts(best, go1, ge1), lefts(best, go2, ge2)))
        H[i, out] = MINF
        H[i, H[i] < MINF // 2] = MINF
        E1[i, 1:] = lefts(H[i], go1, ge1)
        E2[i, 1:] = lefts(H[i], go2, ge2)
        for T in (E1, F1, E2, F2):
            T[i, out] = MINF
            T[i, T[i] < MINF // 2] = MINF  # (sums of -inf: -inf again, so that nothing accumulates)
    return H, E1, F1, E2, F2


def score(s1, s2, mat, index, pc, band=None, dlo=None, dhi=None) -> int:
    return int(fill(s1, s2, mat, index, pc, band, dlo, dhi)[0][-1, -1])


def walk(s1, s2, mat, index, pc, band=None, dlo=None, dhi=None, tables=None) -> np.ndarray:
    """Ops in path order (0, 0) -> (n2, n1): 0 diag, 1 up, 2 left.  States: 0 H, 1 F1, 2 E1, 3
    F2, 4 E2."""
    go1, ge1, go2, ge2 = pc
    n1, n2 = len(s1), len(s2)
    dlo, dhi = _limits(n1, n2, band, dlo, dhi)
    H, E1, F1, E2, F2 = tables if tables is not None else fill(s1, s2, mat, index, pc, dlo=dlo, dhi=dhi)
    sub = sub_table(s1, s2, mat, index) if n1 and n2 else None
    run = {1: (F1, go1 + ge1), 2: (E1, go1 + ge1), 3: (F2, go2 + ge2), 4: (E2, go2 + ge2)}
    i, j = n2, n1
    out = []
    state = 0
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
            else:
                state = next(s for s in (1, 2, 3, 4) if H[i, j] == run[s][0][i, j])
        elif state in (1, 3):
            assert run[state][0][i, j] > MINF // 2
            out.append(1)
            state = 0 if run[state][0][i, j] == H[i - 1, j] + run[state][1] else state  # opening wins a tie
            i -= 1
        else:
            assert run[state][0][i, j] > MINF // 2
            out.append(2)
            state = 0 if run[state][0][i, j] == H[i, j - 1] + run[state][1] else state
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


def path_score(s1, s2, ops, mat, index, pc) -> int:
    """Score of a global path by direct summation: the matrix entry per diag, g(k) for every
    maximal run of k ups and every maximal run of k lefts (an up-run directly followed by a
    left-run is two runs)."""
    mat = np.asarray(mat, np.int64)
    a = np.asarray(s1, np.int8).view(np.uint8)
    b = np.asarray(s2, np.int8).view(np.uint8)
    i = j = total = run = 0
    last = 0
    for op in ops:
        if op != last and run:
            total += int(gap(pc, run))
            run = 0
        if op == 0:
            total += int(mat[index[a[j]], index[b[i]]])
            i += 1
            j += 1
        else:
            run += 1
            i += op == 1
            j += op == 2
        last = op
    if run:
        total += int(gap(pc, run))
    assert (i, j) == (len(b), len(a))
    return total


def brute(s1, s2, mat, index, pc, band=None, dlo=None, dhi=None):
    """The best path_score over every path (0, 0) -> (n2, n1) all of whose vertices lie in the
    band (None if there is none): tiny pairs only.  Every path is enumerated; the band only
    filters."""
    n1, n2 = len(s1), len(s2)
    dlo, dhi = _limits(n1, n2, band, dlo, dhi)
    best = [None]

    def go(i, j, ops):
        if i == n2 and j == n1:
            if all(in_band(x, y, dlo, dhi) for x, y in path_vertices(ops)):
                v = path_score(s1, s2, ops, mat, index, pc)
                best[0] = v if best[0] is None else max(best[0], v)
            return
        if i < n2 and j < n1:
            go(i + 1, j + 1, ops + [0])
        if i < n2:
            go(i + 1, j, ops + [1])
        if j < n1:
            go(i, j + 1, ops + [2])

    go(0, 0, [])
    return best[0]
