"""Plain Python semi-global Gotoh with substitution by matrix -- the checker of the batched
semi-global alignment (tests/test_batch_semi.py, tests/test_batch_semi_host.py).  A helper,
not a conftest; nothing here touches the library, and nothing is taken from the other
checkers beyond tests/nw_gotoh_matrix.py's sub_table (the matrix lookup of every cell): the
host tests hold this one equal to nw_gotoh_matrix with ends = 0 and to a brute force over
the path definition for all 16 `ends`.

    ends bits: 1 H[0][j] = 0;  2 the end cell may be any (n2, j);  4 H[i][0] = 0;
               8 the end cell may be any (i, n1)
    E[i][j] = max(E[i][j-1] + ge, H[i][j-1] + go + ge)
    F[i][j] = max(F[i-1][j] + ge, H[i-1][j] + go + ge)
    H[i][j] = max(H[i-1][j-1] + sub[i-1][j-1], F[i][j], E[i][j])
    H[0][0] = 0, E[i][0] = F[0][j] = -inf; a boundary that is not free: go + k*ge

fill_cells(): those lines, cell by cell (small shapes).
fill():       a row at a time.  Within a row only E looks left.  E[j] = max over k < j of
              H[k] + go + (j - k)*ge; a k whose H[k] came from E[k] is dominated by the k'
              that opened E[k] (it pays go <= 0 once more), so H[k] may be replaced by
              max(diag[k], F[k]) and the maximum over k is one np.maximum.accumulate.
end_cell():   (score, i, j): the first row-major maximum among the admissible end cells.
walk():       the machine of include/nw_hip.h from the end cell; (ops, begin cell).
path_score(): direct summation along ops from a begin cell.
"""
import numpy as np

from nw_gotoh_matrix import sub_table

MINF = -(1 << 44)  # minus infinity for int64 tables
S1_BEGIN, S1_END, S2_BEGIN, S2_END = 1, 2, 4, 8


def _boundaries(n1, n2, ge, go, ends):
    H = np.zeros((n2 + 1, n1 + 1), np.int64)
    E = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    F = np.full((n2 + 1, n1 + 1), MINF, np.int64)
    if not ends & S1_BEGIN:
        for j in range(1, n1 + 1):
            H[0, j] = go + j * ge
    if not ends & S2_BEGIN:
        for i in range(1, n2 + 1):
            H[i, 0] = go + i * ge
    return H, E, F


def fill_cells(s1, s2, mat, index, ge, go, ends):
    n1, n2 = len(s1), len(s2)
    H, E, F = _boundaries(n1, n2, ge, go, ends)
    if n1 == 0 or n2 == 0:
        return H, E, F
    sub = sub_table(s1, s2, mat, index)
    for i in range(1, n2 + 1):
        for j in range(1, n1 + 1):
            E[i, j] = max(E[i, j - 1] + ge, H[i, j - 1] + go + ge)
            F[i, j] = max(F[i - 1, j] + ge, H[i - 1, j] + go + ge)
            H[i, j] = max(H[i - 1, j - 1] + sub[i - 1, j - 1], F[i, j], E[i, j])
    return H, E, F


def fill(s1, s2, mat, index, ge, go, ends):
    """(H, E, F), int64 arrays of (n2 + 1, n1 + 1); -inf cells hold values below MINF / 2."""
    assert go <= 0
    n1, n2 = len(s1), len(s2)
    H, E, F = _boundaries(n1, n2, ge, go, ends)
    if n1 == 0 or n2 == 0:
        return H, E, F
    j = np.arange(n1 + 1, dtype=np.int64)
    sub = sub_table(s1, s2, mat, index)
    for i in range(1, n2 + 1):
        F[i, 1:] = np.maximum(F[i - 1, 1:], H[i - 1, 1:] + go) + ge
        base = np.empty(n1 + 1, np.int64)  # what a left run may open from: column 0, else max(diag, F)
        base[0] = H[i, 0]
        base[1:] = np.maximum(H[i - 1, :-1] + sub[i - 1], F[i, 1:])
        opened = np.maximum.accumulate(base - j * ge)  # max over k <= j of base[k] - k*ge
        E[i, 1:] = opened[:-1] + go + j[1:] * ge
        H[i, 1:] = np.maximum(base[1:], E[i, 1:])
    return H, E, F


def end_cells(n1, n2, ends):
    """The admissible end cells in row-major order."""
    cells = {(n2, n1)}
    if ends & S1_END:
        cells |= {(n2, j) for j in range(n1 + 1)}
    if ends & S2_END:
        cells |= {(i, n1) for i in range(n2 + 1)}
    return sorted(cells)


def end_cell(H, ends):
    """(score, end_i, end_j): the first row-major maximum of H among the admissible end cells."""
    n2, n1 = H.shape[0] - 1, H.shape[1] - 1
    best = None
    for i, j in end_cells(n1, n2, ends):
        if best is None or H[i, j] > best[0]:
            best = (int(H[i, j]), i, j)
    return best


def walk(s1, s2, mat, index, ge, go, ends, tables=None, end=None):
    """(ops in path order begin -> end: 0 diag, 1 up, 2 left; (begin_i, begin_j))."""
    H, E, F = tables if tables is not None else fill(s1, s2, mat, index, ge, go, ends)
    sub = sub_table(s1, s2, mat, index) if len(s1) and len(s2) else None
    i, j = end if end is not None else end_cell(H, ends)[1:]
    out = []
    state = 0  # 0 H, 1 F, 2 E
    while i or j:
        if state == 0:
            if i == 0:
                if ends & S1_BEGIN:
                    break
                out.append(2)
                j -= 1
            elif j == 0:
                if ends & S2_BEGIN:
                    break
                out.append(1)
                i -= 1
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
