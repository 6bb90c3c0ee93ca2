"""Where the banded two-piece sweep (csrc/nw_batch_dual_banded.hip) puts a cell's direction
byte, which variant of the iteration computed it, and what the five-state walk reads of it --
tests/nw_dirmap2.py's questions for the nw_*_batch_dual_banded entries (tests/
test_batch_dual_banded.py, tests/test_batch_dual_banded_host.py).  A helper, not a conftest;
plain Python that never touches the library.  The geometry (csrc/nw_batch.h's batch_banded_*) is
restated here, not imported.

limits():      dlo, dhi as the kernel holds them (kept within PAD diagonals of the table's own).
slots(), first(): a strip's slots in the pair's block and its first iteration.
byte_place():  dual_banded_dir_byte (csrc/nw_batch_dev.h) restated: byte k of dword [p][it -
               first(p)][u][l].
dir_bytes():   nw_batch_dual_banded_dir_bytes restated.
variant():     (masked, edge) of the iteration that computed a cell: `edge` as the sweep picks the
               EDGE variant, `masked` unless the iteration's 64 steps lie wholly in the band.
iterations():  the (masked, edge) of every iteration a pair's strips run.
walk_bits():   nw_batch_dual_banded_walk restated over the checker's bytes (nw_dirmap2.dual_bits
               makes them), with a trace of its reads; it is nw_dirmap2.walk_bits, the address
               apart, and asserts that every read lies in the strip's range.
"""
import numpy as np

import nw_dirmap2 as dm2
from nw_dirmap import coords

PAD = 1024
CLASSES = dm2.CLASSES
VARIANTS = tuple((m, e) for m in (False, True) for e in (False, True))   # (masked, edge)


def limits(n1, n2, band):
    dlo = min(0, n2 - n1) - band
    dhi = max(0, n2 - n1) + band
    return max(dlo, -n1 - PAD), min(dhi, n2 + PAD)


def iters(n2):
    return n2 // 64 + 2


def slots(n1, n2, band):
    dlo, dhi = limits(n1, n2, band)
    return min((dhi - dlo + 319 + 63) // 64 + 2, iters(n2))


def first(p, dlo):
    s = 256 * p + dlo
    return s >> 6 if s > 0 else 0


def last(p, n1, n2, band):
    """The last iteration strip p runs."""
    dlo, dhi = limits(n1, n2, band)
    return min(n2 // 64 + 1, ((256 * p + 319 + dhi) >> 6) + 1, first(p, dlo) + slots(n1, n2, band) - 1)


def dir_bytes(n1, n2, band):
    if n1 < 0 or n2 < 0 or band < 0:
        return -1
    if n1 == 0 or n2 == 0:
        return 0
    return ((n1 + 255) // 256) * slots(n1, n2, band) * 64 * 64 * 4


def byte_place(r, c, n1, n2, band):
    """Index of cell (r, c)'s byte in a pair's block (numbers or arrays), the slot unclamped."""
    dlo, _ = limits(n1, n2, band)
    _, u, k, p, l, it = coords(r, c, n2)
    f = np.where(256 * p + dlo > 0, (256 * p + dlo) >> 6, 0)
    return (((p * slots(n1, n2, band) + it - f) * 64 + u) * 64 + l) * 4 + k


def inside(it, p, dlo, dhi):
    """The iteration's 64 steps lie wholly in the band: the sweep runs the unmasked variant."""
    return (64 * it - 256 * p - 319 >= dlo) & (64 * it + 62 - 256 * p <= dhi)


def variant(r, c, n1, n2, band):
    """(masked, edge, u, k) of cell (r, c) (numbers or arrays)."""
    dlo, dhi = limits(n1, n2, band)
    edge, u, k, p, _, it = coords(r, c, n2)
    return ~inside(it, p, dlo, dhi), edge, u, k


def iterations(n1, n2, band):
    """[(p, it, masked, edge)] of every iteration the sweep runs for this pair."""
    dlo, dhi = limits(n1, n2, band)
    out = []
    for p in range((n1 + 255) // 256):
        for it in range(first(p, dlo), last(p, n1, n2, band) + 1):
            out.append((p, it, not bool(inside(it, p, dlo, dhi)), it == 0 or 64 * it + 63 > n2))
    return out


def walk_bits(bits, n1, n2, band, trace=None):
    """(ops in path order): the device walk over `bits` ((n2 + 1, n1 + 1) bytes of the checker's
    tables); trace receives (r, c, cls) per read."""
    dlo, _ = limits(n1, n2, band)
    nslots = slots(n1, n2, band)
    size = dir_bytes(n1, n2, band)
    r, c, state = n2, n1, 0
    ops = []
    while r > 0 or c > 0:
        if r == 0 or c == 0:
            op = 2 if r == 0 else 1
        else:
            _, _, _, p, _, it = coords(r, c, n2)
            assert 0 <= it - first(int(p), dlo) < nslots and it <= last(int(p), n1, n2, band), (r, c)
            assert 0 <= int(byte_place(r, c, n1, n2, band)) < size
            b = int(bits[r, c])
            if state == 0:
                state = b & 7
                assert state <= 4
                if trace is not None:
                    trace.append((r, c, dm2.SOURCES[state]))
                if state:
                    continue
                op = 0
            else:
                name, bit = dm2.RUNS[state]
                op = 1 if state & 1 else 2
                if trace is not None:
                    trace.append((r, c, name + ("x" if b & bit else "o")))
                state = state if b & bit else 0
        ops.append(op)
        r -= op != 2
        c -= op != 1
    return np.array(ops[::-1], np.uint8)


def combos(trace, n1, n2, band):
    """{(masked, edge, u, k, cls)} of a trace."""
    if not trace:
        return set()
    r, c, cls = zip(*trace)
    m, e, u, k = variant(np.array(r), np.array(c), n1, n2, band)
    return set(zip(m.tolist(), e.tolist(), u.tolist(), k.tolist(), cls))


def all_combos():
    return {(m, e, u, k, cls) for m, e in VARIANTS for u in range(64) for k in range(4) for cls in CLASSES}
