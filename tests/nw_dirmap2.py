"""Where the two-piece batch sweep (csrc/nw_batch_dual.hip) puts a cell's direction byte, and
what the five-state walk reads of it -- tests/nw_dirmap.py's questions for the nw_*_batch_dual
entries (tests/test_batch_dual.py, tests/test_batch_dual_host.py).  A helper, not a conftest;
plain Python that never touches the library.  The instance of a cell (edge, u, k) is
nw_dirmap.coords(): the sweep has the batch's geometry.

byte_place():  dual_dir_byte (csrc/nw_batch_dev.h) restated: one byte per cell.
dual_bits():   the byte the directions kernel writes per inner cell, from the checker's tables:
               bits 0-2 the H source (0 diag, 1 F1, 2 E1, 3 F2, 4 E2: the first that equals H),
               bits 3-6 "extended, not opened" for E1, F1, E2, F2.
walk_bits():   nw_batch_dual_walk restated over those bytes, with a trace of its reads.
A read is (r, c, cls): cls "H0".."H4" in state H (the source found there), "F1x" / "F1o" in
state F1 (the extend bit set: stays; clear: opened here, back to H), and so on for E1, F2, E2.
"""
import numpy as np

from nw_dirmap import coords, iters

SOURCES = ("H0", "H1", "H2", "H3", "H4")
RUNS = {1: ("F1", 16), 2: ("E1", 8), 3: ("F2", 64), 4: ("E2", 32)}   # state: (name, its extend bit)
CLASSES = SOURCES + tuple(n + x for n, _ in RUNS.values() for x in "xo")


def byte_place(r, c, n2):
    """Index of cell (r, c)'s byte in a pair's block: byte k of dword [p][s][l], s = r + l,
    a strip holding 64 * iters(n2) steps."""
    _, _, k, p, l, _ = coords(r, c, n2)
    return ((p * iters(n2) * 64 + r + l) * 64 + l) * 4 + k


def dir_bytes(n1, n2):
    return ((n1 + 255) // 256) * iters(n2) * 64 * 64 * 4


def dual_bits(tabs, sub, pc):
    go1, ge1, go2, ge2 = pc
    H, E1, F1, E2, F2 = tabs
    out = np.zeros(H.shape, np.uint8)
    x = H[1:, 1:]
    code = np.where(x == H[:-1, :-1] + sub, 0,
                    np.where(x == F1[1:, 1:], 1, np.where(x == E1[1:, 1:], 2, np.where(x == F2[1:, 1:], 3, 4))))
    ext = lambda T, go, up: (T[:-1, 1:] if up else T[1:, :-1]) > (H[:-1, 1:] if up else H[1:, :-1]) + go
    out[1:, 1:] = (code | (ext(E1, go1, False) << 3) | (ext(F1, go1, True) << 4) | (ext(E2, go2, False) << 5)
                   | (ext(F2, go2, True) << 6))
    return out


def walk_bits(bits, n1, n2, trace=None):
    """(ops in path order): the device walk over `bits`; trace receives (r, c, cls) per read."""
    r, c, state = n2, n1, 0
    ops = []
    while r > 0 or c > 0:
        if r == 0 or c == 0:
            op = 2 if r == 0 else 1
        else:
            b = int(bits[r, c])
            if state == 0:
                state = b & 7
                assert state <= 4
                if trace is not None:
                    trace.append((r, c, SOURCES[state]))
                if state:
                    continue
                op = 0
            else:
                name, bit = RUNS[state]
                op = 1 if state & 1 else 2
                if trace is not None:
                    trace.append((r, c, name + ("x" if b & bit else "o")))
                state = state if b & bit else 0
        ops.append(op)
        r -= op != 2
        c -= op != 1
    return np.array(ops[::-1], np.uint8)


def combos(trace, n2):
    """{(edge, u, k, cls)} of a trace."""
    if not trace:
        return set()
    r, c, cls = zip(*trace)
    edge, u, k, _, _, _ = coords(np.array(r), np.array(c), n2)
    return set(zip(edge.tolist(), u.tolist(), k.tolist(), cls))


def all_combos():
    return {(e, u, k, cls) for e in (False, True) for u in range(64) for k in range(4) for cls in CLASSES}
