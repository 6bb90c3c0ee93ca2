"""Plain Python Gotoh with substitution by matrix -- the checker of the batched
alignment with a substitution matrix (tests/test_batch_matrix.py, tests/
test_batch_matrix_host.py).  A helper, not a conftest; nothing here touches the library,
and nothing here is taken from tests/nw_gotoh.py, whose substitution is an equality
test inside its fill and its walk: the host tests hold the two checkers equal on
identity-type matrices.

    sub[r][c] = mat[index[s1[c]]][index[s2[r]]]      (mat: n x n, first index the s1 letter;
                                                      index: 256 entries, byte -> letter)
    E[i][j] = max(E[i][j-1] + ge, H[i][j-1] + go + ge)
    F[i][j] = max(F[i-1][j] + ge, H[i-1][j] + go + ge)
    H[i][j] = max(H[i-1][j-1] + sub[i-1][j-1], F[i][j], E[i][j])
    H[0][0] = 0, H[0][j] = go + j*ge, H[i][0] = go + i*ge, E[i][0] = F[0][j] = -inf

fill_cells(): those lines, cell by cell (small shapes).
fill():       a row at a time.  Within a row only E looks left.  E[j] = max over k < j of
              H[k] + go + (j - k)*ge; a k whose H[k] came from E[k] is dominated by the k'
              that opened E[k] (it pays go <= 0 once more), so H[k] may be replaced by
              max(diag[k], F[k]) and the maximum over k is one np.maximum.accumulate.
walk():       the three-state machine of include/nw_hip.h from (n2, n1) to (0, 0).
"""
import numpy as np

MINF = -(1 << 44)  # minus infinity for int64 tables


def sub_table(s1, s2, mat, index):
    """(n2, n1) int64: the substitution score of every cell."""
    mat = np.asarray(mat, np.int64)
    index = np.asarray(index)
    x = index[np.asarray(s1, np.int8).view(np.uint8)].astype(np.intp)
    y = index[np.asarray(s2, np.int8).view(np.uint8)].astype(np.intp)
    return mat[x[None, :], y[:, None]]


def fill_cells(s1, s2, mat, index, ge, go):
    sub = sub_table(s1, s2, mat, index)
    n2, n1 = sub.shape if sub.size else (len(s2), len(s1))
    H = np.zeros((n2 + 1, n1 + 1), np.int64)
    E = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    F = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    for j in range(1, n1 + 1):
        H[0, j] = go + j * ge
    for i in range(1, n2 + 1):
        H[i, 0] = go + i * ge
    for i in range(1, n2 + 1):
        for j in range(1, n1 + 1):
            E[i, j] = max(E[i, j - 1] + ge, H[i, j - 1] + go + ge)
            F[i, j] = max(F[i - 1, j] + ge, H[i - 1, j] + go + ge)
            H[i, j] = max(H[i - 1, j - 1] + sub[i - 1, j - 1], F[i, j], E[i, j])
    return H, E, F


def fill(s1, s2, mat, index, ge, go):
    """(H, E, F), int64 arrays of (n2 + 1, n1 + 1); -inf cells hold values below MINF / 2."""
    assert go <= 0
    n1, n2 = len(s1), len(s2)
    H = np.zeros((n2 + 1, n1 + 1), np.int64)
    E = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    F = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    j = np.arange(n1 + 1, dtype=np.int64)
    H[0, 1:] = go + j[1:] * ge
    H[1:, 0] = go + np.arange(1, n2 + 1, dtype=np.int64) * ge
    if n1 == 0 or n2 == 0:
        return H, E, F
    sub = sub_table(s1, s2, mat, index)
    for i in range(1, n2 + 1):
        F[i, 1:] = np.maximum(F[i - 1, 1:], H[i - 1, 1:] + go) + ge
        best = np.empty(n1 + 1, np.int64)  # what a left run may open from: column 0, else max(diag, F)
        best[0] = H[i, 0]
        best[1:] = np.maximum(H[i - 1, :-1] + sub[i - 1], F[i, 1:])
        opened = np.maximum.accumulate(best - j * ge)  # max over k <= j of best[k] - k*ge
        E[i, 1:] = opened[:-1] + go + j[1:] * ge
        H[i, 1:] = np.maximum(best[1:], E[i, 1:])
    return H, E, F


def score(s1, s2, mat, index, ge, go) -> int:
    return int(fill(s1, s2, mat, index, ge, go)[0][-1, -1])


def walk(s1, s2, mat, index, ge, go, tables=None) -> np.ndarray:
    """Ops in path order (0, 0) -> (n2, n1): 0 diag, 1 up, 2 left."""
    H, E, F = tables if tables is not None else fill(s1, s2, mat, index, ge, go)
    sub = sub_table(s1, s2, mat, index) if len(s1) and len(s2) else None
    i, j = len(s2), len(s1)
    out = []
    state = 0  # 0 H, 1 F, 2 E
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
            elif H[i, j] == F[i, j]:
                state = 1
            else:
                assert H[i, j] == E[i, j], (i, j)
                state = 2
        elif state == 1:
            out.append(1)
            state = 0 if F[i, j] == H[i - 1, j] + go + ge else 1  # opening wins a tie over extending
            i -= 1
        else:
            out.append(2)
            state = 0 if E[i, j] == H[i, j - 1] + go + ge else 2
            j -= 1
    assert state == 0
    return np.array(out[::-1], np.uint8)


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
