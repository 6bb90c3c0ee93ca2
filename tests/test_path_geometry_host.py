"""CPU: the inputs of tests/test_path_geometry.py and the model they are judged by.

The windowed traceback (nw_tb_windows / nw_tb_chain / nw_tb_emit and the host loop
run_traceback, csrc/nw_sw.hip) is fed paths of a chosen SHAPE here: runs of hundreds
of lefts or ups, a window that holds the most moves a window can, paths along row 0,
column 0 and column n1, a round of more than 32 windows.  Each case is a segment
program (tests/nw_windows.py build()); its path comes from oracle.fill /
oracle.sw_fill and the plain walks (tests/nw_walk.py, oracle.sw_traceback), and the
rounds, windows and tail ops it must cost from nw_windows.rounds_model, which reads
the checker's ops and no table.

This module pins the model (the three device counts DESIGN.md records; tb_shift
against the library's own) and asserts, from checker and model alone, that every
case reaches what it is there for.  The GPU module imports the cases and calls
conditions() before it looks at the device's answer.
"""
import functools

import numpy as np
import pytest

import nwhip
import oracle
import nw_windows as nww
from nw_walk import walk
from nw_windows import BLOCK, GLOBAL, LOCAL, R, build, cells, junk, rounds_model, runs

# (band, max_windows, no_aim) of nw_tb_opts
GEOMS = {"aimed": (256, 512, False), "no_aim": (256, 512, True), "narrow": (128, 4096, False),
         "tiny": (17, 3, False)}

UNIT = (1, -1, -1)
CASES = {
    "left_run": ([('M', 300), ('L', 1100), ('M', 300)], UNIT),
    "up_run": ([('M', 300), ('U', 700), ('M', 300)], UNIT),
    "full_window": ([('M', 200), ('X', 700, 256), ('M', 63)], (1, -3, -1)),
    "full_window64": ([('M', 200), ('X', 700, 256), ('M', 64)], (1, -3, -1)),
    "stairs": ([('U', 5), ('M', 3), ('L', 5), ('M', 3)] * 60, (2, -1, -1)),
    "begin_L": ([('L', 400), ('M', 500)], UNIT),
    "begin_U": ([('U', 400), ('M', 500)], UNIT),
    "end_L": ([('M', 500), ('L', 400)], UNIT),
    "end_U": ([('M', 500), ('U', 400)], UNIT),
    "chain66": ([('M', 700), ('L', 3), ('M', 700), ('U', 3)] * 3, UNIT),
    "row0_63": ([('L', 400), ('M', 63)], UNIT),
    "row0_64": ([('L', 400), ('M', 64)], UNIT),
    "row0_65": ([('L', 400), ('M', 65)], UNIT),
    "row0_128": ([('L', 400), ('M', 128)], UNIT),
    # block cases only: the run of lefts lies on a row that is a checkpoint row for
    # K = 64, 128 and 192 / a table tall enough for a block from row 640
    "left_run_ckpt": ([('M', 384), ('L', 1100), ('M', 300)], UNIT),
    "left_run_tall": ([('M', 700), ('L', 1100), ('M', 300)], UNIT),
}
GLOBAL_CASES = [c for c in CASES if c not in ("left_run_ckpt", "left_run_tall")]

# (rounds, windows) of a CPU prototype of the model written apart from it (pure numpy,
# its own fill and walk), per geometry; None: not recorded
PROTOTYPE = {
    "left_run": ((5, 32), (5, 30), (10, 39), (68, 143)),
    "up_run": ((1, 21), (3, 41), (4, 55), (45, 102)),
    "full_window": ((3, 19), (2, 13), None, None),
    "stairs": ((1, 11), (1, 11), (1, 11), (4, 11)),
    "begin_L": ((2, 10, 16), (1, 8, 144), (3, 15, 208), (4, 8, 375)),
    "begin_U": ((1, 15, 0), (1, 15, 144), (2, 25), (4, 8, 388)),
    "end_L": ((2, 16), (2, 16), (4, 32), (26, 65)),
    "end_U": ((1, 15), (2, 26), (3, 36), (26, 73)),
    "chain66": ((1, 66), (1, 66), (1, 66), (22, 66)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(s1, s2, the walk's ops begin -> end, score) of a global case (read-only)."""
    prog, scheme = CASES[name]
    s1, s2 = build(prog)
    t = oracle.fill(s1, s2, scheme)
    ops = walk(s1, s2, t, scheme)
    for a in (s1, s2, ops):
        a.setflags(write=False)
    return s1, s2, ops, int(t[s2.size, s1.size])


@functools.lru_cache(maxsize=None)
def model(name, geom):
    s1, s2, ops, _ = case(name)
    band, maxwin, no_aim = GEOMS[geom]
    return rounds_model(ops[::-1], (s2.size, s1.size), s1.size, band, maxwin, not no_aim, GLOBAL)


def same_row_restarts(m):
    """Rounds that start on the row of the round before: restarts inside a run of lefts."""
    return sum(1 for a, b in zip(m.starts, m.starts[1:]) if a[0] == b[0])


@functools.lru_cache(maxsize=None)
def conditions(name):
    """What the global case `name` is there for, from the walk and the model alone."""
    s1, s2, ops, _ = case(name)
    n1, n2 = s1.size, s2.size
    run = runs(ops)
    m = {g: model(name, g) for g in GEOMS}
    i, j = cells(ops)
    if name == "left_run":
        assert run[2] == 1100 and run[1] == 0
        assert np.count_nonzero(i == 300) == 1101                      # one table row holds the run
        assert all(same_row_restarts(m[g]) >= 2 for g in GEOMS)        # rounds restart in mid-run
        assert m["aimed"].max_moves >= 400 and m["aimed"].x_min == 0
    elif name == "up_run":
        assert run[1] == 700 and run[2] == 0
        assert m["aimed"].rounds == 1 and m["aimed"].used == [21]      # the aim holds it
        assert m["no_aim"].rounds >= 3 and m["no_aim"].x_max == 512    # x runs to 2B
    elif name == "full_window":
        assert (run[1], run[2]) == (256, 700)
        # 63 moves up the window's rows + 512 lefts: all a window can hold
        assert m["no_aim"].max_moves == 575 >= 570 and (m["no_aim"].x_min, m["no_aim"].x_max) == (0, 512)
        assert m["aimed"].max_moves >= 520
    elif name == "full_window64":
        # one more trailing match moves the corner row off the window grid: 512 lefts, no more
        assert (run[1], run[2]) == (256, 700) and m["no_aim"].max_moves == 512
    elif name == "stairs":
        assert run == {0: 3, 1: 5, 2: 5} and np.count_nonzero(np.diff(ops)) >= 4 * 60 - 1
        assert all(m[g].max_moves >= 90 for g in GEOMS)
        assert [m[g].rounds for g in ("aimed", "no_aim", "narrow")] == [1, 1, 1] and m["tiny"].rounds > 1
    elif name == "begin_L":
        assert run[2] == 400 and not (ops[:400] != 2).any()            # row 0, from column 400 to 0
        # forced lefts inside the windows, then the tail
        assert all(0 < m[g].tail_ops < 400 and m[g].stop_r is None for g in GEOMS)
        assert len({m[g].tail_ops for g in GEOMS}) == 4
    elif name == "begin_U":
        assert run[1] == 400 and not (ops[:400] != 1).any()            # column 0
        assert m["aimed"].tail_ops == 0 and m["aimed"].stop_r is not None   # (0, 0) met inside a window
        assert m["narrow"].tail_ops == 0 and m["narrow"].rounds == 2
        assert 0 < m["no_aim"].tail_ops < 400 and 0 < m["tiny"].tail_ops < 400
    elif name == "end_L":
        assert run[2] == 400 and not (ops[-400:] != 2).any()           # the start cell's own row
        for g in GEOMS:
            assert m[g].used[0] == 1 and m[g].starts[1][0] == n2 and m[g].x_min == 0
    elif name == "end_U":
        assert run[1] == 400 and not (ops[-400:] != 1).any()
        assert np.count_nonzero(j == n1) == 401                        # up column n1
        assert m["aimed"].rounds == 1 and m["no_aim"].rounds == 2 and m["no_aim"].x_max == 512
    elif name == "chain66":
        for g in ("aimed", "no_aim", "narrow"):
            assert m[g].rounds == 1 and m[g].used == [66]              # past windows 32 and 64 of one chain
        assert m["tiny"].rounds == 22
    elif name.startswith("row0_"):
        k = int(name[5:])
        assert n2 == k and run[2] == 400
        for g in GEOMS:
            assert m[g].rounds == 1 and m[g].starts[0][0] == k
        if k == 63:    # one window; its row r = 0 is the table's row 0
            assert all(m[g].windows == 1 and 0 < m[g].tail_ops < 400 for g in GEOMS)
        else:
            # the last window launched holds table row 0 on its row r = 63 (k a multiple of 64) or 62
            assert m["no_aim"].windows == k // R + 1 == m["no_aim"].used[0]
            assert m["no_aim"].tail_ops == 144
        if k == 128:   # the steep line caps the aimed rounds below what the rows allow
            assert m["narrow"].windows == 2 < k // R + 1 and m["narrow"].tail_ops == 400
            assert m["aimed"].tail_ops == 0 and m["aimed"].stop_r == 63      # (0, 0) on window row 63
    else:
        raise KeyError(name)
    return True


# ------------------------------------------------------------------ local cases
LOCAL_GEOMS = {"default": (256, 512), "short": (128, 2), "tiny": (17, 3)}   # NW_TB_BAND, NW_TB_MAXWIN
UPS = (2, -3, -1)
CORNER = (2, -7, -1)


def _ups(first=300):
    return [('M', first), ('U', 300), ('M', 300)]


def _corner(first=300):
    return [('M', first), ('X', 300, 100), ('M', 300)]


# name: (program, scheme, (ja, jb, ta, tb))
LOCAL_CASES = {
    "ups_end0": (_ups(), UPS, (37, 60, 40, 17)),
    "ups_end1": (_ups(), UPS, (37, 61, 40, 17)),
    "ups_end63": (_ups(), UPS, (37, 59, 40, 17)),
    "ups_row1": (_ups(), UPS, (37, 0, 40, 17)),
    "ups_stop_r0": (_ups(339), UPS, (37, 29, 40, 17)),
    "ups_stop_r63": (_ups(340), UPS, (37, 29, 40, 17)),
    "corner_end0": (_corner(), CORNER, (37, 4, 40, 17)),
    "corner_end1": (_corner(), CORNER, (37, 5, 40, 17)),
    "corner_end63": (_corner(), CORNER, (37, 3, 40, 17)),
    "corner_col1": (_corner(), CORNER, (0, 29, 40, 17)),
    "corner_stop_r0": (_corner(303), CORNER, (100, 29, 5, 9)),
    "corner_stop_r63": (_corner(304), CORNER, (100, 29, 5, 9)),
}


@functools.lru_cache(maxsize=None)
def local_case(name):
    """(s1, s2, ops begin -> end, begin, end, score) from the oracle (read-only)."""
    prog, scheme, jk = LOCAL_CASES[name]
    s1, s2 = junk(*build(prog), *jk)
    t = oracle.sw_fill(s1, s2, scheme)
    score, ei, ej = oracle.sw_best(s1, s2, scheme)
    ops, bi, bj = oracle.sw_traceback(s1, s2, t, (ei, ej), scheme)
    for a in (s1, s2, ops):
        a.setflags(write=False)
    return s1, s2, ops, (bi, bj), (ei, ej), score


@functools.lru_cache(maxsize=None)
def local_model(name, geom):
    s1, s2, ops, _, end, _ = local_case(name)
    band, maxwin = LOCAL_GEOMS[geom]
    return rounds_model(ops[::-1], end, s1.size, band, maxwin, False, LOCAL)


@functools.lru_cache(maxsize=None)
def local_conditions(name):
    prog, scheme, (ja, jb, ta, tb) = LOCAL_CASES[name]
    s1, s2, ops, (bi, bj), (ei, ej), score = local_case(name)
    run = runs(ops)
    first = prog[0][1]
    if name.startswith("ups"):
        assert (run[1], run[2]) == (300, 0) and score == 2 * (first + 300) - 300 and ops.size == first + 600
    else:
        # the whole corner is on the path: 100 ups, then 300 lefts (walked end -> begin)
        assert (run[1], run[2]) == (100, 300) and score == 2 * (first + 300) - 400 and ops.size == first + 700
        k = int(np.flatnonzero(ops == 2)[0])
        assert not (ops[k:k + 300] != 2).any() and not (ops[k + 300:k + 400] != 1).any()
    # the whole pair is aligned, between the junk
    assert (bi, bj) == (jb, ja) and (ei, ej) == (s2.size - tb, s1.size - ta)
    m = {g: local_model(name, g) for g in LOCAL_GEOMS}
    assert m["default"].rounds <= 2 < m["short"].rounds < m["tiny"].rounds
    tag = name.split("_", 1)[1]
    if tag.startswith("end"):
        assert ei % R == int(tag[3:]) and bi > 1 and bj > 1 and ei < s2.size and ej < s1.size
    elif tag == "row1":
        assert bi == 0 and bj > 0          # the first aligned cell is on row 1: the boundary stops the walk
        assert all(m[g].stop_r is not None for g in LOCAL_GEOMS)
    elif tag == "col1":
        assert bj == 0 and bi > 0
        assert all(m[g].stop_r is not None for g in LOCAL_GEOMS)
    else:
        assert m["default"].stop_r == int(tag[6:]) and bi > 1 and bj > 1
    return True


# ------------------------------------------------------------------ block cases
def block_slices(ops, n2, K):
    """The blocks nw_align_ckpt walks, last to first: (b, row0, rows, cj, lo, hi) -- block b's
    walk starts at (row0 + rows, cj) and makes the moves ops[lo:hi].  A walk from below
    arrives on a row at the last of the path's cells on it and the block ends there."""
    i, j = cells(ops)
    out, cj = [], int(j[-1])
    for b in range(max(1, -(-n2 // K)) - 1, -1, -1):
        if cj == 0:
            break                      # the rest is column 0: a memset on the host
        row0 = b * K
        rows = min(row0 + K, n2) - row0
        hi = int(np.flatnonzero(i == row0 + rows)[-1])
        lo = int(np.flatnonzero(i == row0)[-1]) if b else 0
        assert int(j[hi]) == cj
        out.append((b, row0, rows, cj, lo, hi))
        cj = int(j[lo])
    return out


def block_model(ops, blk, band, maxwin, aim):
    b, row0, rows, cj, lo, hi = blk
    return rounds_model(ops[lo:hi][::-1], (rows, cj), cj, band, maxwin, aim, BLOCK if row0 else GLOBAL, row0, rows)


BLOCK_CASES = ["up_run", "left_run", "left_run_ckpt", "begin_U", "end_U"]
BLOCK_ROWS = [64, 128, 192]
ALONE = {"up_run": (640, 660), "left_run_tall": (640, 360)}      # traceback_block alone: (row0, rows)


@functools.lru_cache(maxsize=None)
def ckpt_model(name, K):
    """(rounds, windows) nw_align_ckpt reports at the default geometry: the blocks' sums."""
    s1, s2, ops, _ = case(name)
    ms = [block_model(ops, blk, 256, 512, True) for blk in block_slices(ops, s2.size, K)]
    return sum(m.rounds for m in ms), sum(m.windows for m in ms)


@functools.lru_cache(maxsize=None)
def block_conditions(name, K):
    s1, s2, ops, _ = case(name)
    n2 = s2.size
    blks = block_slices(ops, n2, K)
    nblk = -(-n2 // K)
    assert nblk >= 3
    i, j = cells(ops)
    # blocks whose start cell lies in a run of lefts on its own row (the block's bottom row)
    in_run = [b for b, row0, rows, cj, lo, hi in blks if hi - lo >= 100 and not (ops[hi - 100:hi] != 2).any()]
    if name == "up_run":
        assert len(blks) == nblk
        pure = [b for b, row0, rows, cj, lo, hi in blks if hi - lo == rows and not (ops[lo:hi] != 1).any()]
        assert len(pure) >= 700 // K - 1               # blocks that are nothing but ups
    elif name == "left_run":
        assert len(blks) == nblk and in_run == []      # row 300: the run is in mid-block
        b, row0, rows, cj, lo, hi = [x for x in blks if x[1] < 300 <= x[1] + x[2]][0]
        assert hi - lo >= 1100 + rows - 1
        assert block_model(ops, (b, row0, rows, cj, lo, hi), 256, 512, True).rounds >= 4
    elif name == "left_run_ckpt":
        # row 384 is a checkpoint row: the block above it ends at the run's right end, and
        # the block below starts there -- 1100 lefts along its bottom row before anything else
        assert len(blks) == nblk and in_run == [384 // K - 1]
        b, row0, rows, cj, lo, hi = [x for x in blks if x[0] == in_run[0]][0]
        assert row0 + rows == 384 and cj == 384 + 1100 and not (ops[hi - 1100:hi] != 2).any()
        m = block_model(ops, (b, row0, rows, cj, lo, hi), 256, 512, True)
        assert m.rounds >= 4 and m.used[0] == 1
    elif name == "begin_U":
        # the walk meets column 0 in the block that holds row 400 and runs up it; above: no walk
        assert len(blks) == nblk - 400 // K and blks[-1][1] <= 400 < blks[-1][1] + blks[-1][2]
        assert int(j[blks[-1][4]]) == 0
    elif name == "end_U":
        assert len(blks) == nblk
        assert sum(1 for b, row0, rows, cj, lo, hi in blks if cj == s1.size and row0 >= 500) >= 400 // K
    else:
        raise KeyError(name)
    return True


# ================================================================== tests
# ------------------------------------------------------------------ 1. the model
def test_model_reproduces_documented_device_counts():
    """DESIGN 6b / tests/test_align.py: identical 2000^2 is (1 round, 32 windows, tail 0) at
    the defaults; s2 = s1[::2], 2000 x 1000, band 128: 1 round of 16 windows aimed, 8 rounds of
    72 windows on the diagonal -- counts measured on the device, which the model has to give."""
    s = np.random.default_rng(2000).integers(1, 5, 2000).astype(np.int8)
    ops = walk(s, s, oracle.fill(s, s, (1, 0, -1)), (1, 0, -1))
    assert not ops.any()
    m = rounds_model(ops[::-1], (2000, 2000), 2000, 256, 512, True, GLOBAL)
    assert (m.rounds, m.windows, m.tail_ops) == (1, 32, 0)
    n1, n2 = 2000, 1000
    for alpha in (20, 4):
        s1 = np.random.default_rng(n1 + 7 * n2 + alpha).integers(1, alpha + 1, n1).astype(np.int8)
        s2 = s1[::2].copy()
        ops = walk(s1, s2, oracle.fill(s1, s2, UNIT), UNIT)
        m = rounds_model(ops[::-1], (n2, n1), n1, 128, 4096, True, GLOBAL)
        assert (m.rounds, m.windows, m.tail_ops) == (1, 16, 0)
        m = rounds_model(ops[::-1], (n2, n1), n1, 128, 4096, False, GLOBAL)
        assert (m.rounds, m.windows, m.tail_ops) == (8, 72, 0)


def test_model_tb_shift_is_the_librarys():
    """nww.tb_shift against nw_debug_tb_shift: lines to the left (num < 0, where C's division
    truncates and Python's floors) and to the right, the B / 2 clamp on both sides, row0 > 0."""
    f = nwhip.lib().nw_debug_tb_shift       # host code: answers without a device
    rng = np.random.default_rng(11)
    grid = [(k, i_s, j_s, B, row0) for k in (0, 1, 2, 3, 31, 32, 65, 511) for i_s in (1, 63, 64, 65, 600, 4209)
            for j_s in (0, 1, 300, 599, 600, 601, 1700, 4209, 100000) for B in (1, 2, 3, 17, 128, 255, 256)
            for row0 in (0, 64, 640, 1 << 19)]
    grid += [(int(rng.integers(0, 600)), int(rng.integers(1, 1 << 20)), int(rng.integers(0, 1 << 20)),
              int(rng.integers(1, 257)), int(rng.integers(0, 1 << 20))) for _ in range(3000)]
    seen = set()
    for k, i_s, j_s, B, row0 in grid:
        assert f(k, i_s, j_s, B, 0, row0) == nww.tb_shift(k, i_s, j_s, B, 0, row0) == 0
        got = f(k, i_s, j_s, B, 1, row0)
        assert got == nww.tb_shift(k, i_s, j_s, B, 1, row0), (k, i_s, j_s, B, row0)
        gi = i_s + row0
        num, clamped = j_s - gi, R * abs(j_s - gi) > (B // 2) * gi
        inexact = not clamped and (k * R * num) % gi != 0
        seen.add((num < 0, clamped, row0 > 0, inexact))
        if inexact and num < 0:
            assert got == (k * R * num) // gi + 1          # toward zero: one above the floor
    assert len(seen) == 2 * 2 * 2 * 2 - 4                   # (a clamped shift has no remainder)
    # consecutive shifts never differ by more than B / 2
    for i_s, j_s, B, row0 in [(600, 1700, 256, 0), (1300, 600, 128, 0), (300, 1508, 17, 640), (64, 464, 256, 0)]:
        c = [nww.tb_shift(k, i_s, j_s, B, 1, row0) for k in range(40)]
        assert max(abs(b - a) for a, b in zip(c, c[1:])) <= B // 2


def test_model_steep_cap():
    """tb_steep_cap restated: no cap while the line's step stays below B / 2 + 1 columns per
    window (drift 0), then B / drift + 2 windows; a block's line is the whole table's."""
    assert nww.tb_steep_cap(1000, 1000, 256) == nww.INT32_MAX
    assert nww.tb_steep_cap(1000, 3000, 256) == nww.INT32_MAX          # step 128 = B / 2: drift 0
    assert nww.tb_steep_cap(1000, 3015, 256) == nww.INT32_MAX          # step 128.96: drift 0
    assert nww.tb_steep_cap(1000, 3016, 256) == 256 // 1 + 2           # step 129.02: drift 1
    assert nww.tb_steep_cap(64, 464, 256) == 256 // (400 - 128) + 2 == 2
    assert nww.tb_steep_cap(600, 1700, 17) == 17 // ((64 * 1100 - 8 * 600) // 600) + 2
    assert nww.tb_steep_cap(300, 1508, 256, 640) == nww.tb_steep_cap(940, 1508, 256)


@pytest.mark.parametrize("name", sorted(PROTOTYPE))
def test_model_agrees_with_the_prototype(name):
    for g, want in zip(GEOMS, PROTOTYPE[name]):
        if want is not None:
            m = model(name, g)
            assert (m.rounds, m.windows, m.tail_ops)[:len(want)] == want, g


# ------------------------------------------------------------------ 2. the cases
@pytest.mark.parametrize("name", GLOBAL_CASES)
def test_global_case_conditions(name):
    s1, s2, ops, score = case(name)
    prog, scheme = CASES[name]
    assert nwhip.ops_score(s1, s2, ops, scheme) == score
    assert conditions(name)
    for g in GEOMS:
        m = model(name, g)
        assert m.rounds >= 1 and m.windows >= sum(m.used) and m.max_moves <= 2 * R - 1 + 2 * GEOMS[g][0]


def test_window_capacity():
    """The most a window's walk can hold -- 64 non-left moves (63 between its rows and the one
    that leaves it) and 2B lefts -- fits the exit record's 10 bits and nw_tb_emit's staging."""
    top = R + 2 * 256
    assert top == 576 <= 1023 and top <= 2 * R + 513 + 8
    assert model("full_window", "no_aim").max_moves == top - 1


@pytest.mark.parametrize("name", sorted(LOCAL_CASES))
def test_local_case_conditions(name):
    assert local_conditions(name)


def test_local_cases_cover_the_residues():
    ends = {local_case(n)[4][0] % R for n in LOCAL_CASES}
    assert {0, 1, 63} <= ends
    assert {local_model(n, "default").stop_r for n in LOCAL_CASES} >= {0, 63}
    assert any(local_case(n)[3][0] == 0 for n in LOCAL_CASES) and any(local_case(n)[3][1] == 0 for n in LOCAL_CASES)


def test_left_run_that_costs_more_than_it_earns_is_dropped():
    """L600 after M300 at match 2: the run costs what the segment before it earned, the walk
    stops at the tie and the run is not on the local path -- why the local cases keep theirs
    at 300."""
    s1, s2 = junk(*build([('M', 300), ('L', 600), ('M', 700)]), 37, 29, 40, 17)
    t = oracle.sw_fill(s1, s2, UPS)
    score, ei, ej = oracle.sw_best(s1, s2, UPS)
    ops, bi, bj = oracle.sw_traceback(s1, s2, t, (ei, ej), UPS)
    assert runs(ops)[2] < 600 and ops.size < 1600


@pytest.mark.parametrize("K", BLOCK_ROWS)
@pytest.mark.parametrize("name", BLOCK_CASES)
def test_block_case_conditions(name, K):
    assert block_conditions(name, K)
    s1, s2, ops, _ = case(name)
    blks = block_slices(ops, s2.size, K)
    # the blocks' moves and the column-0 rest are the whole path
    assert sum(hi - lo for *_, lo, hi in blks) + blks[-1][4] == ops.size
    rounds, windows = ckpt_model(name, K)
    assert rounds >= len(blks) and windows >= rounds


@pytest.mark.parametrize("name", sorted(ALONE))
def test_block_alone_conditions(name):
    s1, s2, ops, _ = case(name)
    row0, rows = ALONE[name]
    assert row0 + rows == s2.size and row0 % R == 0
    i, j = cells(ops)
    lo, hi = int(np.flatnonzero(i == row0)[-1]), ops.size
    blk = (1, row0, rows, s1.size, lo, hi)
    aimed, plain = block_model(ops, blk, 256, 512, True), block_model(ops, blk, 256, 512, False)
    if name == "up_run":
        assert runs(ops[lo:hi])[1] == 360 and aimed.rounds < plain.rounds
    else:
        assert runs(ops[lo:hi])[2] == 1100 and same_row_restarts(aimed) >= 3 and same_row_restarts(plain) >= 3
    # the global row of the block's row 0 moves the line: the same moves from row0 = 0 aim elsewhere
    assert any(nww.tb_shift(k, rows, s1.size, 256, 1, row0) != nww.tb_shift(k, rows, s1.size, 256, 1, 0)
               for k in range(1, 6))
