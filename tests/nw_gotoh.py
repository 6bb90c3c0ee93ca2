"""Plain Python Gotoh -- the checker of the batched alignment under affine gap cost
(tests/test_batch_affine.py, tests/test_batch_affine_host.py).  A helper, not a
conftest; nothing here touches the library.

A run of L consecutive ups, or of L consecutive lefts, costs go + L * ge (go =
gap_open <= 0, ge = scheme[2]):

    E[i][j] = max(E[i][j-1] + ge, H[i][j-1] + go + ge)      (a left run ends at (i, j))
    F[i][j] = max(F[i-1][j] + ge, H[i-1][j] + go + ge)      (an up run ends at (i, j))
    H[i][j] = max(H[i-1][j-1] + s(s1[j-1], s2[i-1]), F[i][j], E[i][j])
    H[0][0] = 0, H[0][j] = go + j*ge, H[i][0] = go + i*ge, E[i][0] = F[0][j] = -inf

fill_cells(): that recurrence cell by cell, literally (small shapes only).
fill():       the same three tables a row at a time.  F and the diagonal depend on the
              row above only.  E unrolls to max over k < j of H[i][k] + go + (j - k)*ge,
              and a k whose H[i][k] is itself E[i][k] never wins alone (opening twice
              costs go <= 0 more than extending), so H[i][k] may be replaced by T[k] =
              max(diag, F) -- known before E -- and E becomes a running maximum.
              tests/test_batch_affine_host.py holds the two fills equal.
walk():       the three-state machine of include/nw_hip.h from (n2, n1) to (0, 0).
"""
import numpy as np

NEG = -(1 << 40)  # minus infinity: far below any score, far from int64 overflow


def _seqs(s1, s2):
    return np.asarray(s1, dtype=np.int8), np.asarray(s2, dtype=np.int8)


def fill_cells(s1, s2, scheme, go):
    s1, s2 = _seqs(s1, s2)
    m, mm, ge = scheme
    n1, n2 = s1.size, s2.size
    H = [[0] * (n1 + 1) for _ in range(n2 + 1)]
    E = [[NEG] * (n1 + 1) for _ in range(n2 + 1)]
    F = [[NEG] * (n1 + 1) for _ in range(n2 + 1)]
    for j in range(1, n1 + 1):
        H[0][j] = go + j * ge
    for i in range(1, n2 + 1):
        H[i][0] = go + i * ge
        for j in range(1, n1 + 1):
            E[i][j] = max(E[i][j - 1] + ge, H[i][j - 1] + go + ge)
            F[i][j] = max(F[i - 1][j] + ge, H[i - 1][j] + go + ge)
            d = H[i - 1][j - 1] + (m if s1[j - 1] == s2[i - 1] else mm)
            H[i][j] = max(d, F[i][j], E[i][j])
    return np.array(H, np.int64), np.array(E, np.int64), np.array(F, np.int64)


def fill(s1, s2, scheme, go):
    """(H, E, F), int64 arrays of (n2 + 1, n1 + 1); -inf cells hold values below NEG / 2."""
    assert go <= 0
    s1, s2 = _seqs(s1, s2)
    m, mm, ge = scheme
    n1, n2 = s1.size, s2.size
    H = np.zeros((n2 + 1, n1 + 1), np.int64)
    E = np.full((n2 + 1, n1 + 1), NEG, np.int64)
    F = np.full((n2 + 1, n1 + 1), NEG, np.int64)
    cols = np.arange(n1 + 1, dtype=np.int64)
    H[0, 1:] = go + cols[1:] * ge
    for i in range(1, n2 + 1):
        H[i, 0] = go + i * ge
        if n1 == 0:
            continue
        F[i, 1:] = np.maximum(F[i - 1, 1:] + ge, H[i - 1, 1:] + go + ge)
        d = H[i - 1, :-1] + np.where(s1 == s2[i - 1], m, mm)
        t = np.empty(n1 + 1, np.int64)
        t[0] = H[i, 0]
        t[1:] = np.maximum(d, F[i, 1:])
        # E[j] = go + j*ge + max over k < j of (T[k] - k*ge)
        run = np.maximum.accumulate(t - cols * ge)
        E[i, 1:] = go + cols[1:] * ge + run[:-1]
        H[i, 1:] = np.maximum(t[1:], E[i, 1:])
    return H, E, F


def score(s1, s2, scheme, go) -> int:
    return int(fill(s1, s2, scheme, go)[0][-1, -1])


def walk(s1, s2, scheme, go, tables=None) -> np.ndarray:
    """Ops in path order (0, 0) -> (n2, n1): 0 diag, 1 up, 2 left."""
    s1, s2 = _seqs(s1, s2)
    H, E, F = tables if tables is not None else fill(s1, s2, scheme, go)
    m, mm, ge = scheme
    i, j = s2.size, s1.size
    ops = []
    state = "H"
    while i > 0 or j > 0:
        if state == "H":
            if i == 0:
                ops.append(2)
                j -= 1
            elif j == 0:
                ops.append(1)
                i -= 1
            elif H[i, j] == H[i - 1, j - 1] + (m if s1[j - 1] == s2[i - 1] else mm):
                ops.append(0)
                i, j = i - 1, j - 1
            elif H[i, j] == F[i, j]:
                state = "F"
            else:
                assert H[i, j] == E[i, j], (i, j)
                state = "E"
        elif state == "F":
            assert i >= 1 and j >= 1
            ops.append(1)
            state = "H" if F[i, j] == H[i - 1, j] + go + ge else "F"
            i -= 1
        else:
            assert i >= 1 and j >= 1
            ops.append(2)
            state = "H" if E[i, j] == H[i, j - 1] + go + ge else "E"
            j -= 1
    assert state == "H"
    return np.array(ops[::-1], dtype=np.uint8)


def path_score_affine(s1, s2, ops, scheme, go) -> int:
    """Score of a global path by direct summation: match / mismatch per diag, ge per up
    or left, go for every run of ups and every run of lefts."""
    m, mm, ge = scheme
    i = j = 0
    total = 0
    prev = 0
    for op in ops:
        if op == 0:
            total += m if s1[j] == s2[i] else mm
            i, j = i + 1, j + 1
        else:
            total += ge + (go if op != prev else 0)
            if op == 1:
                i += 1
            else:
                j += 1
        prev = op
    assert (i, j) == (len(s2), len(s1))
    return total


def runs(ops, op):
    """Lengths and starts of the maximal runs of `op`: [(start, length), ..]."""
    out = []
    k = 0
    ops = list(ops)
    while k < len(ops):
        if ops[k] == op:
            e = k
            while e < len(ops) and ops[e] == op:
                e += 1
            out.append((k, e - k))
            k = e
        else:
            k += 1
    return out
