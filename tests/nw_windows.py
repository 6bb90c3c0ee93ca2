"""Structured pairs and a restatement of the windowed traceback's round structure --
the checker of tests/test_path_geometry.py and tests/test_path_geometry_host.py.
A helper, not a conftest.

build(): a pair from a list of segments, so that the path holds runs of a chosen
length at a chosen place.  rounds_model(): what run_traceback (csrc/nw_sw.hip)
launches for a given path -- rounds, windows, tail ops -- restated in plain Python
and driven by the checker's ops alone; it never reads a table.
"""
import collections

import numpy as np

R = 64                       # rows per window (kTbR)
LOCAL, GLOBAL, BLOCK = 0, 1, 2   # kTbLocal, kTbGlobal, kTbBlock

# letters outside 1..alpha (alpha <= 20), each on one side only
UP_LETTER, LEFT_LETTER = 30, 40                  # s2 only / s1 only
JUNK1_HEAD, JUNK1_TAIL, JUNK2_HEAD, JUNK2_TAIL = 50, 51, 60, 61


def build(prog, alpha=20, seed=1):
    """(s1, s2) from segments: ('M', k) k random letters of 1..alpha on both sides;
    ('U', k) k letters that s2 alone holds (k ups); ('L', k) k letters that s1 alone
    holds (k lefts); ('X', a, b) a letters of s1 alone and b of s2 alone (a corner:
    under mismatch < 2 gap, walked end -> begin, b ups then a lefts)."""
    assert alpha <= 20
    rng = np.random.default_rng(seed)
    a, b = [], []
    for seg in prog:
        if seg[0] == 'M':
            x = rng.integers(1, alpha + 1, seg[1]).tolist()
            a += x
            b += x
        elif seg[0] == 'U':
            b += [UP_LETTER] * seg[1]
        elif seg[0] == 'L':
            a += [LEFT_LETTER] * seg[1]
        elif seg[0] == 'X':
            a += [LEFT_LETTER] * seg[1]
            b += [UP_LETTER] * seg[2]
        else:
            raise ValueError(seg)
    return np.array(a, dtype=np.int8), np.array(b, dtype=np.int8)


def junk(s1, s2, ja, jb, ta, tb):
    """The pair with ja / jb side-private letters before s1 / s2 and ta / tb after
    them: a local alignment of the pair then begins and ends at inner cells."""
    f = lambda n, c: np.full(n, c, dtype=np.int8)
    return (np.concatenate([f(ja, JUNK1_HEAD), s1, f(ta, JUNK1_TAIL)]),
            np.concatenate([f(jb, JUNK2_HEAD), s2, f(tb, JUNK2_TAIL)]))


def runs(ops):
    """Longest run of each op: {0: diag, 1: up, 2: left}."""
    best = {0: 0, 1: 0, 2: 0}
    ops = np.asarray(ops)
    if ops.size:
        edge = np.flatnonzero(np.diff(ops)) + 1
        first = np.concatenate([[0], edge])
        for o, n in zip(ops[first].tolist(), np.diff(np.concatenate([first, [ops.size]])).tolist()):
            best[o] = max(best[o], n)
    return best


def cells(ops, begin=(0, 0)):
    """(i, j) of the cells of a path, begin -> end: arrays of len(ops) + 1."""
    ops = np.asarray(ops)
    i = begin[0] + np.concatenate([[0], np.cumsum(ops != 2)])
    j = begin[1] + np.concatenate([[0], np.cumsum(ops != 1)])
    return i, j


def _tdiv(a, b):
    """C's integer division: truncation toward zero (Python's // floors)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def tb_shift(k, i_s, j_s, B, aim, row0=0):
    """tb_shift (csrc/nw_sw.hip): the cumulative column shift of window k of a round
    from (i_s, j_s) aimed at the global (0, 0)."""
    if not aim:
        return 0
    gi = i_s + row0
    num, lim = j_s - gi, B // 2
    if R * abs(num) > lim * gi:
        return (-k if num < 0 else k) * lim
    return _tdiv(k * R * num, gi)


INT32_MAX = 2 ** 31 - 1


def tb_steep_cap(i_s, j_s, B, row0=0):
    """tb_steep_cap: windows worth launching when the line outruns the B / 2 step."""
    gi = i_s + row0
    mag, lim = abs(j_s - gi), B // 2
    drift = _tdiv(R * mag - lim * gi, gi)
    return INT32_MAX if drift <= 0 else min(B // drift + 2, INT32_MAX)


Rounds = collections.namedtuple(
    "Rounds", "rounds windows tail_ops max_moves x_min x_max stop_r starts used")
Rounds.__doc__ = """rounds, windows (launched), tail_ops: run_traceback's info[4..6];
max_moves: the most moves any one window's walk made; x_min, x_max: the window
columns the path's cells had; stop_r: the window row of the cell where the walk
stopped inside a window (None: it ended in the host loop); starts: each round's
(ci, cj, nwin); used: the windows each round's path entered."""


def rounds_model(rops, start, n1, band, max_windows, aim, kind, row0=0, rows=None):
    """run_traceback for the path whose ops, walked end -> begin, are `rops`, from
    the cell start = (ci, cj) of a table of n1 columns and `rows` rows (default ci;
    a block's rows, with row0 its checkpoint's global row)."""
    B, W = band, 2 * band + 1
    ci, cj = start
    maxwin = min(max_windows, (ci if rows is None else rows) // R + 1)   # tb_workspace
    aim = 1 if aim and kind != LOCAL else 0
    rops = [int(o) for o in rops]
    n, p = len(rops), 0
    rounds = windows = max_moves = 0
    x_min, x_max, stop_r, starts, used = W, -1, None, [], []
    stopped = False
    while not stopped and ci > 0 and cj > 0:
        nwin = min((ci + R) // R, maxwin)
        if aim:
            nwin = min(nwin, tb_steep_cap(ci, cj, B, row0))
        rounds += 1
        windows += nwin
        starts.append((ci, cj, nwin))
        k, x, i, j, cnt = 0, B, ci, cj, 0
        while True:
            i0 = ci - (k + 1) * R + 1
            r = i - i0
            assert 0 <= r < R and 0 <= x < W
            assert j == cj - ci + i0 - B - tb_shift(k, ci, cj, B, aim, row0) + r + x
            assert i >= 0 and 0 <= j <= n1
            x_min, x_max = min(x_min, x), max(x_max, x)
            # the cell's move code (nw_tb_windows)
            inner = i >= 1 and j >= 1
            if kind == LOCAL:
                c = rops[p] if p < n else None                    # t = 0, row / column 0
            elif kind == BLOCK:
                c = rops[p] if inner else None if i == 0 else 1   # row 0 stops; column 0 goes up
            else:
                c = rops[p] if inner else None if i == 0 and j == 0 else 2 if i == 0 else 1
            if c is None:
                stopped, stop_r = True, r
                break
            assert p < n and rops[p] == c, "a forced move the path does not make"
            nx = x + 1 if c == 1 else x - 1 if c == 2 else x
            if nx < 0 or nx >= W:
                break                                 # out of the band: restart at this cell
            p += 1
            cnt += 1
            if c != 2:
                i -= 1
            if c != 1:
                j -= 1
            if c != 2 and r == 0:                     # out of the window's top
                max_moves, cnt = max(max_moves, cnt), 0
                if k + 1 < nwin:
                    x2 = nx + tb_shift(k + 1, ci, cj, B, aim, row0) - tb_shift(k, ci, cj, B, aim, row0)
                    if 0 <= x2 < W:
                        k, x = k + 1, x2
                        continue
                break                                 # restart at the cell after the move
            x = nx
        max_moves = max(max_moves, cnt)
        used.append(k + 1)
        ci, cj = i, j
    tail = 0
    if not stopped:
        if kind == GLOBAL:
            tail = ci if ci > 0 else cj
            forced = 1 if ci > 0 else 2
        elif kind == BLOCK and ci > 0:
            tail, forced = ci, 1
        assert all(o == forced for o in rops[p:p + tail]) if tail else True
    assert p + tail == n, (p, tail, n)
    return Rounds(rounds, windows, tail, max_moves, x_min if rounds else None, x_max if rounds else None,
                  stop_r, starts, used)
