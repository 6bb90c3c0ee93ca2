"""CPU: the case lists of tests/test_batch_paths.py and the proof, from the checkers alone,
that their paths read every unrolled cell instance of the batch sweeps in every way a walk
can read it (tests/nw_dirmap.py says what an instance is and what a read is).

A list is built in code: candidate i of a family is a segment program drawn from the seed
(family, i); KEPT holds the indices a greedy pass kept -- a candidate stays only if it adds
an (edge, u, k, class) combination, read or read where a flipped bit shows -- so the lists
are deterministic and only the kept pairs are ever built.  `python tests/test_batch_paths_host.py`
(with oracle/ and the package on PYTHONPATH) runs the pass again and prints the KEPT table.
"""
import collections
import functools

import numpy as np
import pytest

import nw_dirmap as dm
import nw_gotoh
import nw_gotoh_matrix as gm
import nw_local as nl
import nw_walk
import nw_windows
import oracle

SCHEME, OPEN = (2, -9, -1), -2      # mismatch < 2 gap: a corner is cheaper than mismatches
LETTERS = list(range(1, 21)) + [nw_windows.UP_LETTER, nw_windows.LEFT_LETTER, nw_windows.JUNK1_HEAD,
                                nw_windows.JUNK1_TAIL, nw_windows.JUNK2_HEAD, nw_windows.JUNK2_TAIL]


def _matrix(seed, diag, off):
    rng = np.random.default_rng(seed)
    n = len(LETTERS)
    sc = rng.integers(off[0], off[1] + 1, (n, n))
    sc[np.arange(n), np.arange(n)] = rng.integers(diag[0], diag[1] + 1, n)
    assert (sc != sc.T).any()
    index = np.zeros(256, np.uint8)
    index[LETTERS] = np.arange(n)
    return sc.astype(np.int64), index


# (scores, index, ge, go).  INT8: every s - 2 ge fits int8, the kernel's bytes hold it; WIDE:
# 100 .. 120 on the diagonal under ge = -10, s - 2 ge up to 140 (submat_args' rule, restated
# by wide_form below)
MAT_INT8 = _matrix(61, (3, 6), (-12, -8)) + (-1, -2)
MAT_WIDE = _matrix(62, (100, 120), (-128, -90)) + (-10, -20)
MAT_LOCAL = _matrix(63, (3, 6), (-12, -8)) + (-1, -2)


def wide_form(sc, ge):
    """submat_args: the launch is WIDE when some s - 2 ge leaves int8."""
    v = sc - 2 * ge
    return bool((v < -128).any() or (v > 127).any())


Res = collections.namedtuple("Res", "score ops begin end hit bits")


def _sub_scheme(a, b):
    return np.where(a[None, :] == b[:, None], SCHEME[0], SCHEME[1]).astype(np.int64)


def check_linear(a, b):
    t = oracle.fill(a, b, SCHEME)
    ops = nw_walk.walk(a, b, t, SCHEME)
    return Res(int(t[-1, -1]), ops, (0, 0), (b.size, a.size), True, dm.linear_bits(t, _sub_scheme(a, b), SCHEME[2]))


def check_affine(a, b):
    tabs = nw_gotoh.fill(a, b, SCHEME, OPEN)
    ops = nw_gotoh.walk(a, b, SCHEME, OPEN, tabs)
    return Res(int(tabs[0][-1, -1]), ops, (0, 0), (b.size, a.size), True,
               dm.affine_bits(*tabs, _sub_scheme(a, b), SCHEME[2], OPEN))


def check_matrix(a, b, mat):
    sc, index, ge, go = mat
    tabs = gm.fill(a, b, sc, index, ge, go)
    ops = gm.walk(a, b, sc, index, ge, go, tabs)
    return Res(int(tabs[0][-1, -1]), ops, (0, 0), (b.size, a.size), True,
               dm.affine_bits(*tabs, gm.sub_table(a, b, sc, index), ge, go))


def check_local(a, b):
    sc, index, ge, go = MAT_LOCAL
    tabs = nl.fill(a, b, sc, index, ge, go)
    score, ei, ej = nl.best(tabs[0])
    ops, begin = nl.walk(a, b, sc, index, ge, go, tabs)
    return Res(score, ops, begin, (ei, ej), score > 0,
               dm.affine_bits(*tabs, gm.sub_table(a, b, sc, index), ge, go, local=True))


Family = collections.namedtuple("Family", "kind small seed variants")
FAMILIES = {
    "linear": Family(dm.LINEAR, True, 1, {"linear": check_linear}),
    "affine": Family(dm.AFFINE, True, 2, {"affine": check_affine}),
    "matrix": Family(dm.AFFINE, False, 3, {"int8": functools.partial(check_matrix, mat=MAT_INT8),
                                           "wide": functools.partial(check_matrix, mat=MAT_WIDE)}),
    "local": Family(dm.LOCAL, False, 4, {"local": check_local}),
}
TINY = 1_000_000   # local candidates from here on are tiny pairs: one stop and one end cell each

# the greedy pass's result (search(), below): 6000 tiny and 2000 program candidates for the local
# list, 1000 program candidates for the others
KEPT = {
    "linear": (
        0, 8, 9, 11, 14, 20, 21, 28, 32, 34, 35, 36, 39, 40, 49, 50, 51, 52, 54, 64, 67, 69, 70, 75, 79, 82, 112),
    "affine": (
        2, 3, 5, 6, 7, 9, 10, 11, 15, 16, 17, 20, 24, 27, 28, 30, 32, 33, 34, 35, 36, 37, 38, 42, 44, 46, 47,
        48, 49, 50, 51, 53, 59, 62, 65, 67, 68, 69, 71, 72, 76, 77, 78, 80, 86, 87, 88, 89, 95, 96, 97, 98, 99,
        100, 102, 103, 105, 106, 109, 110, 111, 114, 116, 117, 118, 119, 120, 122, 124, 126, 128, 129, 131, 132,
        134, 137, 140, 141, 145, 146, 147, 150, 154, 158, 160, 161, 162, 164, 166, 167, 170, 174, 175, 176, 178,
        179, 180, 182, 185, 186, 188, 190, 192, 193, 194, 196, 197, 203, 205, 206, 207, 210, 211, 212, 213, 216,
        219, 220, 225, 226, 227, 228, 231, 232, 234, 235, 236, 238, 239, 240, 242, 249, 252, 253, 255, 256, 257,
        264, 265, 269, 271, 273, 277, 285, 286, 287, 291, 296, 304, 305, 306, 311, 312, 313, 314, 316, 325, 329,
        330, 331, 337, 338, 352, 353, 356, 358, 364, 376, 379, 380, 385, 390, 391, 392, 400, 408, 416, 421, 438,
        448, 458, 487, 522, 528, 531, 543, 555, 629),
    "matrix": (
        0, 6, 10, 11, 15, 16, 20, 21, 24, 26, 27, 30, 31, 33, 38, 39, 42, 43, 44, 46, 47, 48, 51, 53, 54, 55,
        56, 60, 61, 62, 65, 66, 68, 69, 70, 72, 75, 76, 78, 80, 81, 82, 83, 84, 85, 86, 87, 92, 93, 94, 99, 103,
        105, 106, 107, 109, 110, 116, 118, 119, 121, 122, 123, 124, 125, 126, 128, 129, 130, 131, 134, 136, 139,
        140, 145, 146, 147, 152, 153, 155, 157, 158, 159, 160, 161, 162, 163, 165, 167, 169, 170, 172, 175, 176,
        180, 183, 184, 185, 188, 190, 191, 193, 195, 197, 201, 203, 204, 205, 207, 208, 209, 210, 211, 214, 218,
        219, 221, 223, 225, 228, 229, 230, 231, 233, 237, 239, 240, 242, 245, 247, 248, 249, 250, 251, 253, 256,
        260, 262, 263, 264, 265, 266, 271, 273, 276, 277, 278, 279, 283, 289, 290, 291, 293, 296, 297, 299, 300,
        301, 306, 307, 308, 311, 315, 322, 323, 324, 327, 333, 337, 339, 341, 342, 354, 366, 367, 371, 374, 378,
        398, 405, 407, 413, 414, 421, 422, 440, 452, 453, 460, 476, 505, 527, 623, 626),
    "local": (
        0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 14, 16, 17, 19, 21, 22, 23, 24, 26, 27, 28, 30, 35, 36, 37, 38,
        39, 40, 41, 42, 43, 45, 46, 48, 49, 50, 53, 54, 55, 56, 58, 59, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69,
        73, 75, 76, 77, 78, 80, 83, 85, 86, 87, 88, 89, 90, 91, 92, 94, 95, 97, 98, 99, 101, 102, 103, 104, 105,
        108, 109, 111, 113, 114, 115, 116, 117, 118, 119, 121, 122, 128, 130, 132, 133, 134, 136, 138, 139, 141,
        142, 143, 144, 145, 146, 148, 149, 150, 151, 152, 153, 154, 155, 156, 158, 160, 162, 163, 165, 166, 167,
        168, 171, 172, 173, 174, 175, 176, 177, 178, 181, 182, 184, 185, 186, 187, 188, 189, 190, 192, 194, 195,
        196, 198, 200, 201, 202, 203, 206, 207, 210, 211, 212, 213, 214, 215, 216, 217, 221, 223, 224, 226, 229,
        230, 231, 232, 233, 234, 236, 237, 239, 240, 241, 242, 243, 244, 247, 248, 251, 253, 254, 255, 256, 258,
        260, 261, 263, 264, 265, 268, 269, 270, 271, 272, 273, 274, 275, 277, 280, 286, 288, 289, 290, 291, 293,
        295, 296, 299, 300, 302, 303, 304, 305, 308, 310, 312, 313, 314, 316, 320, 321, 326, 328, 329, 330, 331,
        333, 334, 335, 338, 339, 343, 344, 347, 351, 353, 354, 355, 357, 361, 364, 369, 370, 373, 374, 375, 376,
        377, 378, 379, 380, 381, 386, 388, 389, 390, 401, 411, 419, 421, 422, 424, 427, 428, 447, 450, 461, 464,
        465, 466, 467, 475, 476, 478, 479, 490, 498, 499, 500, 507, 512, 514, 517, 528, 531, 532, 553, 580, 581,
        583, 585, 588, 600, 602, 603, 610, 623, 627, 639, 649, 671, 682, 714, 716, 728, 730, 731, 780, 812, 834,
        865, 1232, 1320, 1381, 1000001, 1000003, 1000004, 1000005, 1000006, 1000014, 1000015, 1000016, 1000017,
        1000018, 1000019, 1000020, 1000022, 1000023, 1000024, 1000025, 1000026, 1000027, 1000028, 1000031,
        1000034, 1000038, 1000040, 1000042, 1000043, 1000044, 1000045, 1000046, 1000055, 1000056, 1000057,
        1000058, 1000059, 1000063, 1000065, 1000066, 1000068, 1000069, 1000073, 1000074, 1000076, 1000078,
        1000079, 1000080, 1000081, 1000088, 1000090, 1000093, 1000094, 1000095, 1000096, 1000100, 1000105,
        1000106, 1000108, 1000110, 1000112, 1000116, 1000117, 1000119, 1000121, 1000125, 1000126, 1000127,
        1000128, 1000133, 1000134, 1000136, 1000140, 1000145, 1000149, 1000151, 1000153, 1000154, 1000159,
        1000160, 1000164, 1000172, 1000173, 1000174, 1000176, 1000179, 1000193, 1000194, 1000195, 1000196,
        1000197, 1000198, 1000204, 1000205, 1000211, 1000212, 1000213, 1000214, 1000215, 1000217, 1000220,
        1000223, 1000226, 1000230, 1000231, 1000234, 1000235, 1000237, 1000241, 1000242, 1000244, 1000245,
        1000246, 1000247, 1000248, 1000250, 1000254, 1000255, 1000262, 1000265, 1000266, 1000268, 1000270,
        1000271, 1000273, 1000274, 1000281, 1000282, 1000286, 1000289, 1000295, 1000298, 1000302, 1000303,
        1000306, 1000311, 1000317, 1000320, 1000322, 1000324, 1000330, 1000332, 1000338, 1000340, 1000345,
        1000347, 1000349, 1000352, 1000353, 1000354, 1000358, 1000359, 1000360, 1000361, 1000366, 1000368,
        1000369, 1000370, 1000371, 1000372, 1000373, 1000379, 1000380, 1000381, 1000382, 1000384, 1000385,
        1000387, 1000388, 1000395, 1000398, 1000406, 1000409, 1000412, 1000414, 1000415, 1000417, 1000420,
        1000428, 1000429, 1000432, 1000433, 1000437, 1000440, 1000447, 1000451, 1000455, 1000457, 1000460,
        1000467, 1000468, 1000469, 1000470, 1000471, 1000472, 1000478, 1000480, 1000481, 1000483, 1000484,
        1000497, 1000505, 1000507, 1000509, 1000510, 1000513, 1000514, 1000516, 1000517, 1000520, 1000528,
        1000534, 1000536, 1000539, 1000540, 1000541, 1000546, 1000550, 1000551, 1000556, 1000558, 1000570,
        1000575, 1000578, 1000579, 1000583, 1000589, 1000590, 1000597, 1000602, 1000605, 1000611, 1000613,
        1000619, 1000620, 1000621, 1000624, 1000626, 1000631, 1000636, 1000638, 1000640, 1000645, 1000646,
        1000656, 1000660, 1000663, 1000666, 1000671, 1000673, 1000675, 1000677, 1000681, 1000684, 1000694,
        1000695, 1000697, 1000698, 1000703, 1000707, 1000713, 1000718, 1000723, 1000728, 1000729, 1000738,
        1000739, 1000743, 1000747, 1000750, 1000758, 1000760, 1000764, 1000774, 1000776, 1000780, 1000783,
        1000787, 1000799, 1000812, 1000814, 1000815, 1000816, 1000825, 1000833, 1000834, 1000835, 1000844,
        1000849, 1000850, 1000851, 1000856, 1000858, 1000860, 1000869, 1000875, 1000881, 1000883, 1000884,
        1000894, 1000900, 1000911, 1000912, 1000922, 1000927, 1000928, 1000938, 1000942, 1000948, 1000957,
        1000996, 1000998, 1001000, 1001004, 1001013, 1001018, 1001023, 1001024, 1001031, 1001054, 1001060,
        1001067, 1001069, 1001078, 1001083, 1001089, 1001090, 1001095, 1001097, 1001100, 1001122, 1001138,
        1001141, 1001142, 1001154, 1001155, 1001156, 1001212, 1001219, 1001226, 1001263, 1001265, 1001273,
        1001317, 1001323, 1001347, 1001348, 1001363, 1001375, 1001381, 1001438, 1001454, 1001473, 1001476,
        1001487, 1001489, 1001503, 1001506, 1001512, 1001530, 1001531, 1001555, 1001569, 1001590, 1001616,
        1001654, 1001657, 1001680, 1001684, 1001693, 1001703, 1001731, 1001734, 1001737, 1001750, 1001774,
        1001789, 1001815, 1001850, 1001873, 1001888, 1001900, 1001917, 1001950, 1001990, 1001993, 1002028,
        1002060, 1002269, 1002279, 1002332, 1002387, 1002410, 1002486, 1002537, 1002750, 1002788, 1002792,
        1002827, 1002869, 1002874, 1002910, 1002917, 1003066, 1003402),
}


def candidate(name, i):
    """(s1, s2) of candidate i of a family."""
    fam = FAMILIES[name]
    rng = np.random.default_rng([fam.seed, i])
    if name == "local" and i >= TINY:
        # one short segment between junk: the begin cell is (jb, ja), the end cell (jb + m, ja + m)
        m, ja, jb = int(rng.integers(1, 13)), int(rng.integers(1, 10)), int(rng.integers(1, 200))
        ta, tb = int(rng.integers(1, 5)), int(rng.integers(0, 128))
        a, b = dm.pair([("M", m)], int(rng.integers(1 << 30)))
        return dm.junk(a, b, ja, jb, ta, tb)
    prog = dm.program(rng, (700 - 24, 330 - 24) if name == "local" else (700, 330))
    shared = bool(rng.random() < 0.35)
    a, b = dm.pair(prog, int(rng.integers(1 << 30)), small=fam.small, shared=shared)
    if name == "local":
        ja, jb, ta, tb = (int(x) for x in rng.integers(1, 13, 4))
        a, b = dm.junk(a, b, ja, jb, ta, tb)
    return a, b


def cell_of(rd):
    """(r, c) of a read."""
    _, u, k, _, p, l, it = rd
    return 64 * it + u - l, 256 * p + 4 * l + k + 1


def shows(rd, bits):
    """Whether the read's bit, flipped, changes the ops or the hit -- judged locally: an H,
    D / U / L, STOP or END read always (another op is emitted right there, the walk goes on
    where it stopped, the hit's row moves); an F / E read iff the cell the run moves to is an
    inner one whose H choice is not that run's state again (else the walk, back in H, re-
    enters the run at once and emits what it would have; on row 0 / column 0 the state is
    not looked at).  test_a_flipped_bit_shows holds this equal to a walk over flipped bits."""
    cls = rd[3]
    if cls[0] not in "FE":
        return True
    r, c = cell_of(rd)
    r2, c2, st = (r - 1, c, 1) if cls[0] == "F" else (r, c - 1, 2)
    return r2 >= 1 and c2 >= 1 and (int(bits[r2, c2]) & 3) != st


def evaluate(name, a, b):
    """{variant: (Res, reads, combinations read, combinations whose flip shows)}."""
    out = {}
    for v, check in FAMILIES[name].variants.items():
        res = check(a, b)
        rd = dm.reads(res.ops, res.begin, a.size, b.size, FAMILIES[name].kind, res.hit)
        out[v] = (res, rd, dm.combos(rd), {x[:4] for x in rd if shows(x, res.bits)})
    return out


def search(name, candidates):
    """The greedy pass: the indices of `candidates` that add a combination, then without
    those whose combinations the others hold too."""
    kept, seen = {}, collections.Counter()
    for i in candidates:
        ev = evaluate(name, *candidate(name, i))
        keys = {(v, x) for v, e in ev.items() for x in e[2]} | {(v, "shows", x) for v, e in ev.items() for x in e[3]}
        if any(k not in seen for k in keys):
            kept[i] = keys
            seen.update(keys)
    for i in sorted(kept, key=lambda i: len(kept[i])):
        if all(seen[k] >= 2 for k in kept[i]):
            seen.subtract(kept.pop(i))
    return sorted(kept), {k for k, n in seen.items() if n > 0}


@functools.lru_cache(maxsize=None)
def cases(name):
    """The family's pairs."""
    return tuple(candidate(name, i) for i in KEPT[name])


@functools.lru_cache(maxsize=None)
def _evaluated(name):
    return tuple(evaluate(name, a, b) for a, b in cases(name))


def results(name, variant):
    """Per pair (Res, reads, combinations read, combinations whose flip shows), from the checker alone."""
    return tuple(ev[variant] for ev in _evaluated(name))


VARIANTS = [(n, v) for n, f in FAMILIES.items() for v in f.variants]
ids = lambda nv: nv[1]


# ------------------------------------------------------------------ the lists
@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_lists_shapes(name):
    pairs = cases(name)
    assert len(pairs) == len(set(KEPT[name])) and all(a.size <= 700 and b.size <= 330 for a, b in pairs)
    assert all(1 <= a.size and 1 <= b.size for a, b in pairs)
    strips = collections.Counter((a.size + 255) // 256 for a, _ in pairs)
    assert min(strips[1], strips[2], strips[3]) >= 1, strips   # pairs of one, two and three strips
    # rows >= 127: an iteration that is not an edge one exists; 191 and 255: two and three of them
    for rows in (127, 191, 255):
        assert sum(b.size >= rows for _, b in pairs) >= 5
    if FAMILIES[name].small:
        # the batch's s1 holds at most kMaxPerm distinct bytes and both table bytes fit int8:
        # without NW_FLAG_NO_PROFILE the SUB_PERM kernels run, with it SUB_GEN -- on this same list
        assert len(set(np.concatenate([a for a, _ in pairs]).tolist())) <= dm.MAX_PERM
        assert all(-128 <= s - 2 * SCHEME[2] <= 127 for s in SCHEME[:2])


def test_the_matrices_forms():
    assert not wide_form(MAT_INT8[0], MAT_INT8[2]) and wide_form(MAT_WIDE[0], MAT_WIDE[2])
    assert not wide_form(MAT_LOCAL[0], 0)   # (the local kernels' bytes are s itself)


# ------------------------------------------------------------------ coverage: conditions, not measurements
@pytest.mark.parametrize("nv", VARIANTS, ids=ids)
def test_every_instance_is_read_in_every_way(nv):
    """linear 2 x 64 x 4 x 3 = 1536, affine and matrix 3584, local 3584 + 512 STOP + 512 END:
    all of them, no exclusion."""
    kind = FAMILIES[nv[0]].kind
    read = set().union(*(r[2] for r in results(*nv)))
    want = dm.all_combos(kind)
    assert len(want) == 2 * 64 * 4 * len(dm.CLASSES[kind])
    assert not want - read, sorted(want - read)[:20]


@pytest.mark.parametrize("nv", VARIANTS, ids=ids)
def test_secondary_conditions(nv):
    name, kind = nv[0], FAMILIES[nv[0]].kind
    res = results(*nv)
    fed, pub, last, first = set(), set(), set(), set()
    for (a, b), (_, rd, _, _) in zip(cases(name), res):
        nstrips, nblocks = (a.size + 255) // 256, b.size // 64 + 1
        for _, _, _, cls, p, l, it in rd:
            if p >= 1 and l == 0:
                fed.add(cls)        # a cell fed from the column scratch
            if l == 63 and p + 1 < nstrips:
                pub.add(cls)        # a cell whose H and E are published
            if it == nblocks:
                last.add(cls)
            if it == 0:
                first.add(cls)
    classes = set(dm.CLASSES[kind]) - {"STOP", "END"}   # (the stop and end cells' lanes: below)
    for got in (fed, pub, last, first):
        assert got >= classes, classes - got
    if kind == dm.LINEAR:
        return
    # an X corner: E left and F entered with no diag between (end -> begin: ups, then lefts)
    assert sum(_has(r[0].ops, [2, 1]) for r in res) >= 10
    if kind == dm.AFFINE:
        # an up run whose begin-side cell is on row 1: the walk returns to H on row 0 because F
        # can only have been opened there (F[0][c] is minus infinity)
        assert sum(any(x[3] == "F0" and cell_of(x)[0] == 1 for x in rd) for _, rd, _, _ in res) >= 3
    # A left run whose begin-side cell is on column 1 CANNOT be walked, in any pair: it is worth
    # H[r][0] + go + c ge = 2 go + (r + c) ge (local: go + c ge < 0), an up run from row 0 down
    # column c is worth the same, so F[r][c] >= E[r][c] wherever such a run ends, and in state H
    # the walk takes F before E (the inequality: test_no_left_run_can_end_on_column_1).  No list
    # reads E0 there:
    for _, rd, _, _ in res:
        assert not any(x[3] == "E0" and cell_of(x)[1] == 1 for x in rd)
    if kind == dm.LOCAL:
        ends = {(which, dm.coords(*cell, b.size)[4]) for (a, b), (r, _, _, _) in zip(cases(name), res) if r.hit
                for which, cell in (("begin", r.begin), ("end", r.end)) if min(cell) >= 1}
        assert {("begin", 0), ("begin", 63), ("end", 0), ("end", 63)} <= ends


def _has(ops, sub):
    """Whether the ops hold `sub` as a substring."""
    return bytes(sub) in bytes(np.asarray(ops, np.uint8))


@pytest.mark.parametrize("nv", [nv for nv in VARIANTS if nv[0] in ("affine", "matrix")], ids=ids)
def test_no_left_run_can_end_on_column_1(nv):
    """The proof behind the exclusion above: F[r][c] >= 2 go + (r + c) ge on every cell of every pair."""
    ge, go = (SCHEME[2], OPEN) if nv[0] == "affine" else FAMILIES[nv[0]].variants[nv[1]].keywords["mat"][2:]
    for a, b in cases(nv[0]):
        if nv[0] == "affine":
            F = nw_gotoh.fill(a, b, SCHEME, OPEN)[2]
        else:
            sc, index = FAMILIES[nv[0]].variants[nv[1]].keywords["mat"][:2]
            F = gm.fill(a, b, sc, index, ge, go)[2]
        r, c = np.mgrid[1:b.size + 1, 1:a.size + 1]
        assert (F[1:, 1:] >= 2 * go + (r + c) * ge).all()


# ------------------------------------------------------------------ reads() against a traced walk
@pytest.mark.parametrize("nv", VARIANTS, ids=ids)
def test_reads_are_what_a_walk_over_the_bits_reads(nv):
    """The device walks restated over the bits the checker's tables imply: the same ops and
    begin cell as the checker's own walk, and exactly the reads that reads() derives from
    the ops alone."""
    kind = FAMILIES[nv[0]].kind
    for (a, b), (res, rd, _, _) in zip(cases(nv[0]), results(*nv)):
        trace = []
        ops, begin = dm.walk_bits(res.bits, a.size, b.size, kind, res.end, trace=trace)
        np.testing.assert_array_equal(ops, res.ops)
        assert begin == tuple(res.begin)
        want = sorted((cell_of(x) + (x[3],)) for x in rd if x[3] != "END")
        assert sorted(trace) == want


# ------------------------------------------------------------------ the mutation argument, reference side
def _flipped(bits, cls):
    if cls in "DUL":
        return (bits + 1) % 3
    if cls[0] == "H":
        return (bits & 12) | ((bits & 3) + 1) % 3
    if cls == "STOP":
        return bits & 12
    return bits ^ (8 if cls[0] == "F" else 4)


@pytest.mark.parametrize("nv", VARIANTS, ids=ids)
def test_a_flipped_bit_shows(nv):
    """For every (edge, u, k, class) some pair of the list reads that instance in that way at a
    cell where the flipped bit changes the ops (or, for STOP, the begin cell): the next three
    ops of the walk from that cell differ.  END is the instance's `step` constant: any other
    value moves end_i of that pair.  And shows() is right where it says no: there the walk
    over the flipped bits emits the same ops."""
    kind = FAMILIES[nv[0]].kind
    chosen, silent = {}, []
    for n, ((a, b), (res, rd, _, _)) in enumerate(zip(cases(nv[0]), results(*nv))):
        for x in rd:
            if x[3] == "END":
                chosen.setdefault(x[:4], None)
            elif shows(x, res.bits):
                chosen.setdefault(x[:4], (n, x))
            elif len(silent) < 300:
                silent.append((n, x))
    assert set(chosen) == dm.all_combos(kind)

    def differs(n, x):
        (a, b), res = cases(nv[0])[n], results(*nv)[n][0]
        r, c = cell_of(x)
        state = {"F": 1, "E": 2}.get(x[3][0], 0)
        flip = (r, c, int(_flipped(int(res.bits[r, c]), x[3])))
        one = dm.walk_bits(res.bits, a.size, b.size, kind, (r, c), state=state, max_ops=3)
        two = dm.walk_bits(res.bits, a.size, b.size, kind, (r, c), flip=flip, state=state, max_ops=3)
        return one[0].tolist() != two[0].tolist() or one[1] != two[1]

    for key, pick in chosen.items():
        assert pick is None or differs(*pick), key
    assert not any(differs(n, x) for n, x in silent)


# ------------------------------------------------------------------ checker sanity on these lists
@pytest.mark.parametrize("nv", VARIANTS, ids=ids)
def test_path_score_is_the_score(nv):
    for (a, b), (res, _, _, _) in zip(cases(nv[0]), results(*nv)):
        if nv[0] == "linear":
            assert nw_walk.path_score(a, b, res.ops, SCHEME) == res.score
        elif nv[0] == "affine":
            assert nw_gotoh.path_score_affine(a, b, res.ops, SCHEME, OPEN) == res.score
        elif nv[0] == "matrix":
            assert gm.path_score(a, b, res.ops, *FAMILIES["matrix"].variants[nv[1]].keywords["mat"]) == res.score
        else:
            assert nl.path_score(a, b, res.ops, res.begin, *MAT_LOCAL) == (res.score, tuple(res.end))
            assert res.hit and res.score > 0


@pytest.mark.parametrize("name", ["affine", "matrix", "local"])
def test_row_fill_equals_the_cell_recurrence(name):
    small = sorted(cases(name), key=lambda p: p[0].size * p[1].size)[:4]   # (fill_cells is a Python loop per cell)
    for a, b in small:
        if name == "affine":
            got, want = nw_gotoh.fill(a, b, SCHEME, OPEN), nw_gotoh.fill_cells(a, b, SCHEME, OPEN)
        elif name == "matrix":
            got, want = gm.fill(a, b, *MAT_WIDE), gm.fill_cells(a, b, *MAT_WIDE)
        else:
            got, want = nl.fill(a, b, *MAT_LOCAL), nl.fill_cells(a, b, *MAT_LOCAL)
        for x, y in zip(got, want):
            np.testing.assert_array_equal(np.maximum(x, -(1 << 30)), np.maximum(y, -(1 << 30)))


# ------------------------------------------------------------------ the layout restated
@pytest.mark.parametrize("n1,n2", [(5, 3), (256, 64), (257, 127), (700, 330)])
def test_places_are_distinct_and_inside_the_block(n1, n2):
    r, c = np.mgrid[1:n2 + 1, 1:n1 + 1]
    for place, kind in ((dm.linear_place, dm.LINEAR), (dm.nibble_place, dm.AFFINE)):
        byte, shift = place(r, c, n2)
        assert byte.min() >= 0 and byte.max() < dm.dir_bytes(n1, n2, kind)
        assert np.unique(byte.ravel() * 8 + shift.ravel()).size == n1 * n2
    edge, u, k, p, l, it = dm.coords(r, c, n2)
    assert it.max() <= n2 // 64 + 1 and edge[it == n2 // 64 + 1].all() and edge[it == 0].all()
    assert ((64 * it + u - l == r) & (256 * p + 4 * l + k + 1 == c)).all()


# ------------------------------------------------------------------ the gap being closed
def existing_lists(name):
    """[(s1, s2, walk)]: the pair lists of the ops tests that were there before this module,
    each pair with the checker call that gives (ops, begin, hit) under the cost its test runs:
    test_batch.ops_pairs() (for the matrix and local families their own ops_pairs), the seam
    pairs, and the 200 pairs of test_scheme_range / test_local_range."""
    import nwhip
    import test_batch as tb
    import test_batch_affine as tba
    import test_batch_local as tbl
    import test_batch_matrix as tbm
    import test_local_range_host as lrh
    import test_scheme_range as tsr
    live = lambda pairs: [(a, b) for a, b in pairs if a.size and b.size]
    out = []
    if name == "linear":
        costs = [(tb.ops_pairs(), s) for s in tb.SCHEMES] + [(live(tsr.crowd(4)), (1, -1, -1))]
        for pairs, s in costs:
            out += [(a, b, lambda a, b, s=s: (nw_walk.walk(a, b, None, s), (0, 0), True)) for a, b in pairs]
    elif name == "affine":
        x, y = tba.seam_pair()
        costs = [(tb.ops_pairs(), s, go) for s in tb.SCHEMES for go in (-3, -11)]
        costs += [([(x, y), (y, x)], s, go) for s, go in [((1, -1, -1), -10), ((2, -1, -2), -5), ((1, 0, -1), -4)]]
        costs += [(live(tsr.crowd(4)), (1, -1, -1), -3)]
        for pairs, s, go in costs:
            out += [(a, b, lambda a, b, s=s, go=go: (nw_gotoh.walk(a, b, s, go), (0, 0), True)) for a, b in pairs]
    elif name == "matrix":
        m = tbm.matrix(20)
        sc = np.random.default_rng(47).integers(-4, -1, (4, 4))   # test_one_long_run_across_the_seams' matrix
        sc[np.arange(4), np.arange(4)] = 5
        seam = nwhip.SubMatrix([1, 2, 3, 4], sc)
        x, y = tbm.seam_pair()
        costs = [(tbm.ops_pairs20(), m, -1, -11), (tbm.ops_pairs20(), m, -2, -3), ([(x, y), (y, x)], seam, -1, -10),
                 (live(tsr.crowd(20)), m, -1, -11)]
        for pairs, m, ge, go in costs:
            out += [(a, b, lambda a, b, m=m, ge=ge, go=go: (gm.walk(a, b, m.scores, m.index, ge, go), (0, 0), True))
                    for a, b in pairs]
    else:
        def walk(a, b, m, ge, go):
            tabs = nl.fill(a, b, m.scores, m.index, ge, go)
            ops, begin = nl.walk(a, b, m.scores, m.index, ge, go, tabs)
            return ops, begin, nl.best(tabs[0])[0] > 0
        m, uni = tbl.matrix(20), nwhip.SubMatrix.uniform([1, 2, 3, 4], *tbl.UNI)
        # test_gap_runs_inside_a_local_path's two pairs: 300 lefts over the seam, 300 ups over the row blocks
        rng = np.random.default_rng(902)
        P, Q = rng.integers(3, 5, 10).astype(np.int8), rng.integers(3, 5, 10).astype(np.int8)
        a, b = tbl._bg(400, 60)
        tbl._put(a, 50, P), tbl._put(a, 360, Q), tbl._put(b, 20, np.concatenate([P, Q]))
        c, d = tbl._bg(60, 360)
        tbl._put(c, 20, np.concatenate([P, Q])), tbl._put(d, 15, P), tbl._put(d, 325, Q)
        costs = [(tbl.ops_pairs(), m, -1, -11), (tbl.ops_pairs(), m, -2, -3), (tbl.placed_pairs()[0], uni, -1, -11),
                 ([(a, b), (c, d)], nwhip.SubMatrix.uniform([1, 2, 3, 4], 100, -100), -1, -11),
                 (live(lrh.crowd()), lrh.matrix("UNI4")) + lrh.CROWD_COST]
        for pairs, m, ge, go in costs:
            out += [(a, b, lambda a, b, m=m, ge=ge, go=go: walk(a, b, m, ge, go)) for a, b in pairs]
    return out


def before(name):
    """{class: (combinations read in the plain variant, in the EDGE variant)} of existing_lists(name),
    and the total: DESIGN 6n's "before" columns (`python tests/test_batch_paths_host.py before`)."""
    kind = FAMILIES[name].kind
    read = set()
    for a, b, walk in existing_lists(name):
        ops, begin, hit = walk(a, b)
        read |= dm.combos(dm.reads(ops, begin, a.size, b.size, kind, hit))
    per = {cls: tuple(sum(1 for x in read if x[3] == cls and x[0] == e) for e in (False, True))
           for cls in dm.CLASSES[kind]}
    return per, len(read)


BEFORE = {"linear": 1154, "affine": 2067, "matrix": 2140, "local": 1696}   # before()'s totals, as DESIGN 6n records them


@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_gap_that_was_there(name):
    """The existing lists read this many of the combinations, and not all of them."""
    per, total = before(name)
    assert total == BEFORE[name] < len(dm.all_combos(FAMILIES[name].kind)), (total, per)


if __name__ == "__main__":
    import sys
    import textwrap
    if sys.argv[1:] == ["before"]:
        for fam in FAMILIES:
            per, total = before(fam)
            print(fam, total, "of", len(dm.all_combos(FAMILIES[fam].kind)))
            for cls, (plain, edge) in per.items():
                print(f"  {cls:5s} plain {plain:3d} / 256   EDGE {edge:3d} / 256")
        sys.exit(0)
    print("KEPT = {")
    for fam in FAMILIES:
        cands = list(range(TINY, TINY + 6000)) + list(range(2000)) if fam == "local" else list(range(1000))
        kept, _ = search(fam, cands)
        body = ", ".join(str(i) for i in kept)
        print(f'    "{fam}": (')
        print(textwrap.fill(body, 112, initial_indent=" " * 8, subsequent_indent=" " * 8) + "),")
    print("}")
