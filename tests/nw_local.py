"""Plain Python Smith-Waterman under affine gap cost with substitution by matrix -- the
checker of the batched local alignment (tests/test_batch_local.py, tests/
test_batch_local_host.py).  A helper, not a conftest; nothing here touches the library,
and nothing is taken from tests/nw_gotoh_matrix.py beyond its sub_table (the matrix
lookup of every cell): the host tests hold this checker equal to the oracle's
Smith-Waterman on match / mismatch matrices with gap_open = 0.

    E[i][j] = max(E[i][j-1] + ge, H[i][j-1] + go + ge)
    F[i][j] = max(F[i-1][j] + ge, H[i-1][j] + go + ge)
    H[i][j] = max(0, H[i-1][j-1] + sub[i-1][j-1], F[i][j], E[i][j])
    H[0][j] = H[i][0] = 0,   E[i][0] = F[0][j] = -inf

fill_cells(): those lines, cell by cell (small shapes).
fill():       a row at a time.  Within a row only E looks left.  E[j] = max over k < j of
              H[k] + go + (j - k)*ge; a k whose H[k] came from E[k] is dominated by the k'
              that opened E[k] (it pays go <= 0 once more), so H[k] may be replaced by
              max(0, diag[k], F[k]) and the maximum over k is one np.maximum.accumulate.
best():       (score, end_i, end_j): the first maximum in row-major order; 0 at (0, 0).
walk():       the machine of include/nw_hip.h from the end cell: in state H it stops at a
              cell with H == 0 (checked first), else takes the first of diag, F, E that
              equals H; in F and E opening wins a tie over extending.
path_score(): direct summation along ops from a begin cell.
"""
import numpy as np

from nw_gotoh_matrix import sub_table

MINF = -(1 << 44)  # minus infinity for int64 tables


def fill_cells(s1, s2, mat, index, ge, go):
    n1, n2 = len(s1), len(s2)
    H = np.zeros((n2 + 1, n1 + 1), np.int64)
    E = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    F = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    if n1 == 0 or n2 == 0:
        return H, E, F
    sub = sub_table(s1, s2, mat, index)
    for i in range(1, n2 + 1):
        for j in range(1, n1 + 1):
            E[i, j] = max(E[i, j - 1] + ge, H[i, j - 1] + go + ge)
            F[i, j] = max(F[i - 1, j] + ge, H[i - 1, j] + go + ge)
            H[i, j] = max(0, H[i - 1, j - 1] + sub[i - 1, j - 1], F[i, j], E[i, j])
    return H, E, F


def fill(s1, s2, mat, index, ge, go):
    """(H, E, F), int64 arrays of (n2 + 1, n1 + 1); -inf cells hold values below MINF / 2."""
    assert go <= 0
    n1, n2 = len(s1), len(s2)
    H = np.zeros((n2 + 1, n1 + 1), np.int64)
    E = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    F = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    if n1 == 0 or n2 == 0:
        return H, E, F
    j = np.arange(n1 + 1, dtype=np.int64)
    sub = sub_table(s1, s2, mat, index)
    for i in range(1, n2 + 1):
        F[i, 1:] = np.maximum(F[i - 1, 1:], H[i - 1, 1:] + go) + ge
        base = np.zeros(n1 + 1, np.int64)  # what a left run may open from: column 0, else max(0, diag, F)
        base[1:] = np.maximum(np.maximum(H[i - 1, :-1] + sub[i - 1], F[i, 1:]), 0)
        opened = np.maximum.accumulate(base - j * ge)  # max over k <= j of base[k] - k*ge
        E[i, 1:] = opened[:-1] + go + j[1:] * ge
        H[i, 1:] = np.maximum(base[1:], E[i, 1:])
    return H, E, F


def best(H):
    """(score, end_i, end_j): the first row-major maximum of H; (0, 0, 0) when it is 0."""
    k = int(np.argmax(H))  # (the first occurrence in C order)
    i, j = divmod(k, H.shape[1])
    if H[i, j] <= 0:
        return 0, 0, 0
    return int(H[i, j]), i, j


def walk(s1, s2, mat, index, ge, go, tables=None, end=None):
    """(ops in path order begin -> end: 0 diag, 1 up, 2 left; (begin_i, begin_j))."""
    H, E, F = tables if tables is not None else fill(s1, s2, mat, index, ge, go)
    sub = sub_table(s1, s2, mat, index) if len(s1) and len(s2) else None
    i, j = end if end is not None else best(H)[1:]
    out = []
    state = 0  # 0 H, 1 F, 2 E
    while True:
        if state == 0:
            if H[i, j] == 0:
                break
            if H[i, j] == H[i - 1, j - 1] + sub[i - 1, j - 1]:
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
    return np.array(out[::-1], np.uint8), (i, j)


def path_score(s1, s2, ops, begin, mat, index, ge, go):
    """(score, end cell) of a path from `begin` by direct summation: the matrix entry per
    diag, ge per up or left, go for every run of ups and every run of lefts."""
    mat = np.asarray(mat, np.int64)
    a = np.asarray(s1, np.int8).view(np.uint8)
    b = np.asarray(s2, np.int8).view(np.uint8)
    i, j = begin
    total = 0
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
    return total, (int(i), int(j))
