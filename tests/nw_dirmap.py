"""Where the batch sweeps put a cell's direction bits, and which of them a walk reads --
the checker of tests/test_batch_paths.py and tests/test_batch_paths_host.py.  A helper,
not a conftest; plain Python that never touches the library.

The four batch sweeps (csrc/nw_batch.hip, nw_batch_affine.hip, and the skeleton of
nw_batch_dev.h under nw_batch_matrix.hip and nw_batch_local.hip) are fully unrolled: a
64-step iteration is 16 groups x 4 steps x 4 columns = 256 cell INSTANCES (u, k), each with
its own constant shift and its own direction dword, each compiled twice (EDGE and not).  A
walk reads only the bits of the cells on its path, so a test covers an instance only where
one of its paths passes a cell that this instance computed.

coords():     the instance of cell (r, c) and where its bits lie, restated from the comments
              of the two layouts.
reads():      what a walk reads, from the checker's ops alone (it never reads a table).
program(), pair(), junk():  structured pairs on tests/nw_windows.py build() / junk().
linear_bits(), affine_bits(), walk_bits():  the direction bits the checker's tables imply
              and the device walks restated over them, with one cell's bits replaced: the
              reference side of the mutation argument.
"""
import numpy as np

import nw_windows as nw

LINEAR, AFFINE, LOCAL = "linear", "affine", "local"
CLASSES = {LINEAR: ("D", "U", "L"),
           AFFINE: ("H0", "H1", "H2", "F0", "F1", "E0", "E1"),
           LOCAL: ("H0", "H1", "H2", "F0", "F1", "E0", "E1", "STOP", "END")}
MAX_PERM = 7       # kMaxPerm: distinct column characters the v_perm score tables cover
STRIP, LANES, C = 256, 64, 4


def coords(r, c, n2):
    """(edge, u, k, p, l, it) of cell (r, c), r, c >= 1, of a pair of n2 rows (numbers or
    arrays): strip p, lane l, column k of the lane, step s = r + l = 64 it + u; `edge` as
    sweep_pair / affine_pair / batch_pair pick the EDGE variant of an iteration (the final
    iteration it == n2 / 64 + 1 is always an edge one)."""
    cj = np.asarray(c) - 1
    p, l, k = cj >> 8, (cj & 255) >> 2, cj & 3
    s = np.asarray(r) + l
    it, u = s >> 6, s & 63
    edge = (it == 0) | (64 * it + 63 > n2)
    return edge, u, k, p, l, it


def iters(n2):
    """batch_iters: iterations of one strip (row 64 * nblocks - 1 completes in iteration nblocks)."""
    return n2 // 64 + 2


def linear_place(r, c, n2):
    """(byte index, bit shift) of the 2 bits of cell (r, c) in a pair's block of
    nw_batch_sweep<true>: byte s % 4 of dword [p][s / 4][l], bits 2k."""
    _, _, k, p, l, _ = coords(r, c, n2)
    s = r + l
    return ((p * iters(n2) * 16 + (s >> 2)) * 64 + l) * 4 + (s & 3), 2 * k


def nibble_place(r, c, n2):
    """(byte index, bit shift) of the 4 bits of cell (r, c) in the affine family's layout
    (NW_DIR_NIBBLE): nibble k % 2 of byte (s % 2) * 2 + k / 2 of dword [p][s / 64][s % 64 / 4]
    [s % 4 / 2][l]."""
    _, u, k, p, l, it = coords(r, c, n2)
    s = r + l
    dword = (((p * iters(n2) + it) * 16 + (u >> 2)) * 2 + ((s & 3) >> 1)) * 64 + l
    return dword * 4 + (s & 1) * 2 + (k >> 1), 4 * (k & 1)


def dir_bytes(n1, n2, kind):
    """Bytes of a pair's direction block (without the padding between pairs)."""
    return ((n1 + STRIP - 1) // STRIP) * iters(n2) * 16 * LANES * 4 * (1 if kind == LINEAR else 2)


def _runs(ops, op):
    """[(lo, hi)]: the maximal runs ops[lo..hi] == op."""
    at = np.flatnonzero(ops == op)
    if at.size == 0:
        return []
    cut = np.flatnonzero(np.diff(at) > 1)
    return list(zip(at[np.concatenate([[0], cut + 1])].tolist(), at[np.concatenate([cut, [at.size - 1]])].tolist()))


def reads(ops, begin, n1, n2, kind, hit=True):
    """[(edge, u, k, cls, p, l, it)]: what the walk of `kind` reads on the path `ops` (path
    order, from the cell `begin`), from the ops alone.

    linear: at every inner cell the 2 bits, cls D / U / L = the op emitted there; row 0 and
    column 0 are walked without reading.
    affine (also the matrix kernels; gap_open < 0): a diag is H0 at the cell it leaves.  A
    maximal run of ups on a column >= 1 is ONE F run -- re-entering F from H right after
    leaving it would mean H == F at a cell whose F the run extended, and extending beats
    opening by -gap_open > 0 there -- so the walk reads H1 at the run's end-side cell, F1 (bit
    3 set, stay) at every cell of the run but the begin-side one and F0 (bit 3 clear, back
    to H) there.  Lefts likewise with H2, E1, E0 (bit 2).  Ups on column 0 and lefts on row 0
    read nothing.
    local: the same, plus STOP at the begin cell when it is an inner cell (code 3 ends the
    walk; on row 0 / column 0 the boundary does) and END at the path's end cell, the cell
    whose instance's `step` constant produced end_i (hit=False: a pair without a hit).
    tests/test_batch_paths_host.py holds this equal to a traced walk over the bits."""
    ops = np.asarray(ops, np.uint8)
    i, j = nw.cells(ops, begin)
    r, c = i[1:], j[1:]                       # the cell at which op t is emitted
    inner = (r >= 1) & (c >= 1)
    where, cls = [], []
    if kind == LINEAR:
        at = np.flatnonzero(inner)
        where.append(at)
        cls += [CLASSES[LINEAR][o] for o in ops[at].tolist()]
    else:
        at = np.flatnonzero(inner & (ops == 0))
        where.append(at)
        cls += ["H0"] * at.size
        for op, h, stay, leave in ((1, "H1", "F1", "F0"), (2, "H2", "E1", "E0")):
            for lo, hi in _runs(np.where(inner, ops, 255), op):
                where.append(np.concatenate([[hi], np.arange(hi, lo, -1), [lo]]))
                cls += [h] + [stay] * (hi - lo) + [leave]
    at = np.concatenate(where) if where else np.zeros(0, np.int64)
    rr, cc = r[at], c[at]
    if kind == LOCAL:
        if begin[0] >= 1 and begin[1] >= 1 and hit:
            rr, cc = np.append(rr, begin[0]), np.append(cc, begin[1])
            cls.append("STOP")
        if hit:
            rr, cc = np.append(rr, i[-1]), np.append(cc, j[-1])
            cls.append("END")
    edge, u, k, p, l, it = coords(rr, cc, n2)
    return list(zip(edge.tolist(), u.tolist(), k.tolist(), cls, p.tolist(), l.tolist(), it.tolist()))


def combos(rd):
    """{(edge, u, k, cls)} of a list of reads."""
    return {x[:4] for x in rd}


def all_combos(kind):
    return {(e, u, k, cls) for e in (False, True) for u in range(64) for k in range(4) for cls in CLASSES[kind]}


# ---------------------------------------------------------------- structured pairs
SMALL = 4                                   # M letters of the small-alphabet form
S_LEFT = 5                                  # s1's left-run letter there: 5 distinct bytes in all


def program(rng, cap=(700, 330)):
    """A random segment program: an optional lead of lefts and ups (the path then runs
    through other lanes and steps), then 6..13 x [M 1..39, one of U 1..9, L 1..11, X (1..7,
    1..5), S 2..9, T 2..9], cut where the pair would exceed `cap` columns x rows.  S k / T k
    (pair() below): k ups / k lefts across cells where a diagonal ties with the run."""
    prog, n1, n2 = [], 0, 0
    lead = rng.integers(0, 4)
    if lead & 1:
        a = int(rng.integers(1, 420))
        prog.append(("L", a))
        n1 += a
    if lead & 2:
        b = int(rng.integers(1, 130))
        prog.append(("U", b))
        n2 += b
    for _ in range(int(rng.integers(6, 14))):
        seg = [("M", int(rng.integers(1, 40)))]
        kind = rng.integers(0, 5)
        if kind == 0:
            seg.append(("U", int(rng.integers(1, 10))))
        elif kind == 1:
            seg.append(("L", int(rng.integers(1, 12))))
        elif kind == 2:
            seg.append(("X", int(rng.integers(1, 8)), int(rng.integers(1, 6))))
        else:
            seg.append(("S" if kind == 3 else "T", int(rng.integers(2, 10))))
        d1 = sum(s[1] for s in seg if s[0] not in "US")
        d2 = sum(s[1] if s[0] in "MUS" else s[2] if s[0] == "X" else 0 for s in seg)
        if n1 + d1 > cap[0] or n2 + d2 > cap[1]:
            break
        prog += seg
        n1, n2 = n1 + d1, n2 + d2
    return prog


def pair(prog, seed, small=False, shared=False):
    """(s1, s2) of a program.  small: the M letters are 1..4 and the left-run letter is 5,
    so that a batch's s1 holds 5 distinct bytes, within the 7 the v_perm tables cover, and the
    SUB_PERM kernels run (build()'s 20 letters force the compares).  shared: the gap runs' letters
    are drawn from the M letters instead of side-private ones, so that a run may slide and a
    diagonal may tie with the run it crosses.  Segments beyond build()'s: ('S', k), k - 1
    copies of the last M letter and then one letter of s2 alone, all in s2 -- k ups on the
    column of that M letter, and on all of them but the end-side one the diagonal (a match
    from the cell left of the run) equals F, so that H there is "diag" while F was extended
    through it; ('T', k), the same in s1 with lefts and E."""
    if not small and not shared and all(s[0] in "MULX" for s in prog):
        return nw.build(prog, 20, seed)
    alpha = SMALL if small else 20
    rng = np.random.default_rng(seed)
    a, b = [], []
    draw = lambda n: rng.integers(1, alpha + 1, n).tolist()
    for seg in prog:
        if seg[0] == "M":
            x = draw(seg[1])
            a += x
            b += x
            continue
        if seg[0] in "ST":
            left, up = S_LEFT if small else nw.LEFT_LETTER, nw.UP_LETTER
            if seg[0] == "S":
                b += [a[-1] if a else up] * (seg[1] - 1) + [up]
            else:
                a += [b[-1] if b else left] * (seg[1] - 1) + [left]
            continue
        na = seg[1] if seg[0] in "LX" else 0
        nb = seg[1] if seg[0] == "U" else seg[2] if seg[0] == "X" else 0
        a += draw(na) if shared else [S_LEFT if small else nw.LEFT_LETTER] * na
        b += draw(nb) if shared else [nw.UP_LETTER] * nb
    return np.array(a, np.int8), np.array(b, np.int8)


junk = nw.junk


# ---------------------------------------------------------------- bits and walks over them
def linear_bits(T, sub, g):
    """(n2 + 1, n1 + 1) uint8: the code nw_batch_sweep<true> writes per inner cell (0 diag, 1
    up, 2 left: the first that reproduces t), from the table T; sub: (n2, n1) scores."""
    T = np.asarray(T, np.int64)
    out = np.zeros(T.shape, np.uint8)
    x = T[1:, 1:]
    out[1:, 1:] = np.where(x == T[:-1, :-1] + sub, 0, np.where(x == T[:-1, 1:] + g, 1, 2))
    return out


def affine_bits(H, E, F, sub, ge, go, local=False):
    """(n2 + 1, n1 + 1) uint8: the nibble the affine family's directions kernels write per
    inner cell: bits 0-1 the H choice (local: 3 where H == 0, tested first), bit 2 "E
    extended" (strictly better than opening), bit 3 "F extended"."""
    out = np.zeros(H.shape, np.uint8)
    x = H[1:, 1:]
    code = np.where(x == H[:-1, :-1] + sub, 0, np.where(x == F[1:, 1:], 1, 2))
    if local:
        code = np.where(x == 0, 3, code)
    ext_e = E[1:, :-1] + ge > H[1:, :-1] + go + ge
    ext_f = F[:-1, 1:] + ge > H[:-1, 1:] + go + ge
    out[1:, 1:] = code | (ext_e << 2) | (ext_f << 3)
    return out


def walk_bits(bits, n1, n2, kind, end=None, flip=None, trace=None, state=0, max_ops=None):
    """The device walk of `kind` over `bits` (nw_batch_walk, nw_batch_affine_walk, nw_batch_
    local_walk restated): (ops in path order, the cell where it ended).  flip = (r, c,
    value): that cell's bits replaced.  trace: a list that receives (r, c, cls) per read.
    end, state, max_ops: a part of a walk, from that cell in that state, of at most so many
    ops."""
    r, c = end if end is not None else (n2, n1)
    ops = []
    limit = n1 + n2 + 2 if max_ops is None else max_ops

    def get(r, c):
        return flip[2] if flip is not None and (r, c) == flip[:2] else int(bits[r, c])

    def note(cls):
        if trace is not None:
            trace.append((r, c, cls))

    while ((r > 0 and c > 0) if kind == LOCAL else (r > 0 or c > 0)) and len(ops) < limit:
        if r == 0 or c == 0:
            op = 2 if r == 0 else 1
        elif kind == LINEAR:
            op = get(r, c) & 3
            note("DUL"[op] if op < 3 else "?")
        else:
            b = get(r, c)
            if state == 0:
                state = b & 3
                if state == 3:
                    if kind == LOCAL:
                        note("STOP")
                        break
                    state = 2   # (no global kernel writes 3; nw_batch_affine_walk's last branch takes it as E)
                note("H%d" % (b & 3))
                if state:
                    continue
                op = 0
            elif state == 1:
                op, state = 1, 1 if b & 8 else 0
                note("F1" if b & 8 else "F0")
            else:
                op, state = 2, 2 if b & 4 else 0
                note("E1" if b & 4 else "E0")
        ops.append(op)
        r -= op != 2
        c -= op != 1
    return np.array(ops[::-1], np.uint8), (r, c)
