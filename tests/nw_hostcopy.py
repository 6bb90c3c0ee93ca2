"""Plain-Python restatement of nw_fill's copy-back arithmetic (csrc/nw_hostcopy.h):
the staging chunk a table asks for, the chunk plan, the copy-thread rule and the
spans of the threaded memcpy -- the fixed one and the one before the fix, whose
uncopied bytes (`holes`) the GPU tests aim at.  No numpy, no device."""
from collections import namedtuple

K_STAGES = 3
STAGE_MAX, STAGE_MIN = 256 << 20, 16 << 20
PAR_MIN = 8 << 20
THREADS_MAX = 64
MIB = 1 << 20

Plan = namedtuple("Plan", "stage_cap rpc nch direct")


def stage_want(table_bytes: int) -> int:
    two = 2 * MIB
    return min(STAGE_MAX, max(STAGE_MIN, (table_bytes // K_STAGES + two - 1) // two * two))


def plan_bytes(table_bytes: int, row_bytes: int, rows: int, stage_cap: int = 0) -> Plan:
    cap = max(stage_cap, stage_want(table_bytes))
    rpc = max(1, cap // row_bytes)
    return Plan(cap, rpc, -(-rows // rpc), rpc * row_bytes > cap)


def plan(n1: int, n2: int, stage_cap: int = 0) -> Plan:
    """The plan of an n1 x n2 table ((n2 + 1) rows of (n1 + 1) int32) when the ring
    holds chunks of stage_cap bytes (0: after nw_host_release)."""
    w = 4 * (n1 + 1)
    return plan_bytes(w * (n2 + 1), w, n2 + 1, stage_cap)


def chunks(p: Plan, rows: int):
    """[(first row, rows)] of every chunk."""
    return [(ch * p.rpc, min(p.rpc, rows - ch * p.rpc)) for ch in range(p.nch)]


def warm_cap() -> int:
    """stage_cap after nw_host_warmup."""
    return stage_want(STAGE_MAX * K_STAGES)


def threads_of(env, cores: int = 8) -> int:
    """The copy threads for NW_COPY_THREADS = env (None: unset), C strtol semantics."""
    if env is None:
        return min(8, max(1, cores))
    s = env.lstrip(" \t\n\v\f\r")
    sign, i = 1, 0
    if s[:1] in ("+", "-"):
        sign, i = (-1 if s[0] == "-" else 1), 1
    j = i
    while j < len(s) and s[j].isdigit() and s[j].isascii():
        j += 1
    v = sign * int(s[i:j]) if j > i else 0
    return min(THREADS_MAX, max(1, v))


def spans(nbytes: int, threads: int, fixed: bool = True):
    """[(offset, bytes)] that par_memcpy's threads copy.  fixed=False: the span
    before the fix, the floor of nbytes / threads rounded up to 4096."""
    if threads <= 1 or nbytes < PAR_MIN:
        return [(0, nbytes)]
    q = -(-nbytes // threads) if fixed else nbytes // threads
    per = (q + 4095) // 4096 * 4096
    out = []
    for t in range(threads):
        o = t * per
        if o >= nbytes:
            break
        out.append((o, min(per, nbytes - o)))
    return out


def uncopied(nbytes: int, threads: int, fixed: bool = True) -> int:
    """Bytes at the end of the block that no span covers."""
    o, n = spans(nbytes, threads, fixed)[-1]
    return nbytes - (o + n)


def holes(n1: int, n2: int, threads: int = 8, stage_cap: int = 0, fixed: bool = False):
    """[(chunk, row, column)] of the int32 cells of nw_fill's host table that the
    threaded copy leaves unwritten (none when fixed; none on the direct branch)."""
    p = plan(n1, n2, stage_cap)
    if p.direct:
        return []
    w = 4 * (n1 + 1)
    out = []
    for ch, (r0, nr) in enumerate(chunks(p, n2 + 1)):
        lost = uncopied(nr * w, threads, fixed)
        first = (r0 * w + nr * w - lost) // 4
        out += [(ch, c // (n1 + 1), c % (n1 + 1)) for c in range(first, first + lost // 4)]
    return out
