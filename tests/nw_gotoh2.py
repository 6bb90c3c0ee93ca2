"""Plain Python global alignment with a substitution matrix under a TWO-PIECE affine gap
cost -- the checker of the nw_*_batch_dual entries (tests/test_batch_dual.py, tests/
test_batch_dual_host.py).  A helper, not a conftest; nothing here touches the library.

A run of k ups or of k lefts costs g(k) = max(go1 + k*ge1, go2 + k*ge2); `pc` below is (go1,
ge1, go2, ge2).  With sub[r][c] = mat[index[s1[c]]][index[s2[r]]] as in tests/nw_gotoh_matrix.py:

    E_t[i][j] = max(E_t[i][j-1] + ge_t, H[i][j-1] + go_t + ge_t)      t = 1, 2
    F_t[i][j] = max(F_t[i-1][j] + ge_t, H[i-1][j] + go_t + ge_t)
    H[i][j]   = max(H[i-1][j-1] + sub[i-1][j-1], F_1, E_1, F_2, E_2)
    H[0][0] = 0, H[0][j] = g(j), H[i][0] = g(i), E_t[i][0] = F_t[0][j] = -inf

fill_cells(): those lines, cell by cell (small shapes).
fill():       a row at a time.  Within a row only the E_t look left.  First H: E_t[j] = max
              over k < j of H[k] + go_t + (j - k)*ge_t, and a k whose H[k] came from a left
              run (of either piece) opened at k' is dominated by k' itself under one of the
              pieces (g(a) + g(b) <= g(a + b)), so max(E_1, E_2) -- not each E_t -- is exact
              when H[k] is replaced by max(diag[k], F_1[k], F_2[k]).  That gives the exact
              H; the exact E_t, which the walk's "opening wins" test reads, then come from
              the exact H by the same accumulate, once per piece.
walk():       the five-state machine of include/nw_hip.h from (n2, n1) to (0, 0).
path_score(): the direct sum over the ops, the better piece per maximal run.
brute():      the best path_score over every path of a tiny pair.
"""
import numpy as np

from nw_gotoh_matrix import MINF, sub_table


def gap(pc, k):
    """g(k), k >= 1 (numbers or arrays)."""
    go1, ge1, go2, ge2 = pc
    return np.maximum(go1 + k * ge1, go2 + k * ge2)


def _tables(n1, n2, pc):
    H = np.zeros((n2 + 1, n1 + 1), np.int64)
    H[0, 1:] = gap(pc, np.arange(1, n1 + 1, dtype=np.int64))
    H[1:, 0] = gap(pc, np.arange(1, n2 + 1, dtype=np.int64))
    return [H] + [np.full((n2 + 1, n1 + 1), MINF, np.int64) for _ in range(4)]


def fill_cells(s1, s2, mat, index, pc):
    """(H, E1, F1, E2, F2), int64 arrays of (n2 + 1, n1 + 1)."""
    go1, ge1, go2, ge2 = pc
    n1, n2 = len(s1), len(s2)
    H, E1, F1, E2, F2 = _tables(n1, n2, pc)
    sub = sub_table(s1, s2, mat, index) if n1 and n2 else None
    for i in range(1, n2 + 1):
        for j in range(1, n1 + 1):
            E1[i, j] = max(E1[i, j - 1] + ge1, H[i, j - 1] + go1 + ge1)
            E2[i, j] = max(E2[i, j - 1] + ge2, H[i, j - 1] + go2 + ge2)
            F1[i, j] = max(F1[i - 1, j] + ge1, H[i - 1, j] + go1 + ge1)
            F2[i, j] = max(F2[i - 1, j] + ge2, H[i - 1, j] + go2 + ge2)
            H[i, j] = max(H[i - 1, j - 1] + sub[i - 1, j - 1], F1[i, j], E1[i, j], F2[i, j], E2[i, j])
    return H, E1, F1, E2, F2


def fill(s1, s2, mat, index, pc):
    """fill_cells() a row at a time: H, F_t and E_t exact; -inf cells hold values below MINF / 2."""
    go1, ge1, go2, ge2 = pc
    assert go1 <= 0 and go2 <= 0
    n1, n2 = len(s1), len(s2)
    H, E1, F1, E2, F2 = _tables(n1, n2, pc)
    if n1 == 0 or n2 == 0:
        return H, E1, F1, E2, F2
    sub = sub_table(s1, s2, mat, index)
    j = np.arange(n1 + 1, dtype=np.int64)

    def lefts(src, go, ge):   # [j >= 1]: max over k < j of src[k] + go + (j - k) * ge
        return np.maximum.accumulate(src - j * ge)[:-1] + go + j[1:] * ge

    for i in range(1, n2 + 1):
        F1[i, 1:] = np.maximum(F1[i - 1, 1:], H[i - 1, 1:] + go1) + ge1
        F2[i, 1:] = np.maximum(F2[i - 1, 1:], H[i - 1, 1:] + go2) + ge2
        best = np.empty(n1 + 1, np.int64)   # what a left run need open from: column 0, else max(diag, F_1, F_2)
        best[0] = H[i, 0]
        best[1:] = np.maximum(H[i - 1, :-1] + sub[i - 1], np.maximum(F1[i, 1:], F2[i, 1:]))
        H[i, 1:] = np.maximum(best[1:], np.maximum(lefts(best, go1, ge1), lefts(best, go2, ge2)))
        E1[i, 1:] = lefts(H[i], go1, ge1)
        E2[i, 1:] = lefts(H[i], go2, ge2)
    return H, E1, F1, E2, F2


def score(s1, s2, mat, index, pc) -> int:
    return int(fill(s1, s2, mat, index, pc)[0][-1, -1])


def walk(s1, s2, mat, index, pc, tables=None) -> np.ndarray:
    """Ops in path order (0, 0) -> (n2, n1): 0 diag, 1 up, 2 left.  States: 0 H, 1 F1, 2 E1,
    3 F2, 4 E2."""
    go1, ge1, go2, ge2 = pc
    H, E1, F1, E2, F2 = tables if tables is not None else fill(s1, s2, mat, index, pc)
    sub = sub_table(s1, s2, mat, index) if len(s1) and len(s2) else None
    run = {1: (F1, go1 + ge1), 2: (E1, go1 + ge1), 3: (F2, go2 + ge2), 4: (E2, go2 + ge2)}
    i, j = len(s2), len(s1)
    out = []
    state = 0
    while i or j:
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
            out.append(1)
            state = 0 if run[state][0][i, j] == H[i - 1, j] + run[state][1] else state   # opening wins a tie
            i -= 1
        else:
            out.append(2)
            state = 0 if run[state][0][i, j] == H[i, j - 1] + run[state][1] else state
            j -= 1
    assert state == 0
    return np.array(out[::-1], np.uint8)


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


def brute(s1, s2, mat, index, pc) -> int:
    """The best path_score over every path (0, 0) -> (n2, n1): tiny pairs only."""
    n1, n2 = len(s1), len(s2)
    best = [None]

    def go(i, j, ops):
        if i == n2 and j == n1:
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
