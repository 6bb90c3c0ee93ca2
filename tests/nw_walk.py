"""Plain Python walk of a Needleman-Wunsch table -- the checker of the device
traceback (tests/test_align.py, tests/test_align_host.py).  A helper, not a conftest.

walk(): from (n2, n1) to (0, 0), at every inner cell the first move that
reproduces t in the order diag > up > left (the order in which serial.cpp:24-30
takes its max); along row 0 the move is left, along column 0 up, without looking
at the table.  Returns the ops in path order (0, 0) -> (n2, n1): 0 diag, 1 up,
2 left (the convention of include/nw_hip.h).
"""
import numpy as np

import oracle


def walk(s1, s2, table=None, scheme=(1, 0, -1)) -> np.ndarray:
    s1 = np.asarray(s1, dtype=np.int8)
    s2 = np.asarray(s2, dtype=np.int8)
    if table is None:
        table = oracle.fill(s1, s2, scheme)
    m, mm, g = scheme
    i, j = s2.size, s1.size
    assert table.shape == (i + 1, j + 1)
    ops = []
    while i > 0 or j > 0:
        if i == 0:
            ops.append(2)
            j -= 1
            continue
        if j == 0:
            ops.append(1)
            i -= 1
            continue
        t = int(table[i, j])
        if t == int(table[i - 1, j - 1]) + (m if s1[j - 1] == s2[i - 1] else mm):
            ops.append(0)
            i, j = i - 1, j - 1
        elif t == int(table[i - 1, j]) + g:
            ops.append(1)
            i -= 1
        else:
            assert t == int(table[i, j - 1]) + g, (i, j)
            ops.append(2)
            j -= 1
    return np.array(ops[::-1], dtype=np.uint8)


def path_score(s1, s2, ops, scheme=(1, 0, -1)) -> int:
    """Score of a global path by direct summation (independent of the library)."""
    m, mm, g = scheme
    i = j = 0
    total = 0
    for op in ops:
        if op == 0:
            total += m if s1[j] == s2[i] else mm
            i, j = i + 1, j + 1
        elif op == 1:
            total += g
            i += 1
        else:
            total += g
            j += 1
    assert (i, j) == (len(s2), len(s1))
    return total
