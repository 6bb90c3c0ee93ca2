"""Times of the batched alignment against a host loop over the one-pair entries;
writes profiles/batch_time.json.

Per shape: pairs, total cells, the batched calls (nw_score_batch: fill_ms and wall;
nw_align_batch: fill_ms, walk_ms and wall; medians of --reps runs after a warm-up),
GCUPS, and the wall time of the same pairs through a loop of nw_score and of nw_align
(medians of --loop-reps runs after a warm-up on the first pairs).  The loop is the
library's one-pair path, unchanged by the batch; its scores must equal the batch's.

  --shape 150 | 1000 | 8000 | mixed | all   one shape per process, so that a job can give
                                            each its own time limit; the JSON is merged

  --gap-open G      the affine-gap entries instead (nw_score_batch_affine, nw_align_batch_affine;
                    a gap of length L costs G + L * gap): per shape their times and GCUPS, the
                    linear entries timed in the same process right before them, and the ratio
                    of the two; no host loop (the one-pair entries have no affine form).
                    Writes profiles/batch_affine_time.json; profiles/batch_time.json stays.

  --matrix N        the matrix entries (nw_score_batch_matrix, nw_align_batch_matrix) on pairs over
                    a seeded random N-letter alphabet under a seeded symmetric int8 matrix with
                    entries in -4..11 (BLOSUM62's span), gap -1 and --gap-open (default -11); in
                    the same process the affine entries on 4-letter pairs of the same sizes (the
                    yardstick: code the matrix does not touch) and the two ratios.  Writes
                    profiles/batch_matrix_time.json.

  --local           the local entries (nw_score_batch_local, nw_align_batch_local) on pairs over 20
                    letters under a seeded symmetric matrix whose expected score on random
                    letters is negative (3..11 on the diagonal, -6..1 off it), gap -1 and
                    --gap-open (default -11); every pair holds a planted segment: a stretch of
                    s1 (a quarter to three quarters of the shorter side) stands in s2 with 10 %
                    substitutions and an indel run of 1..20 every 60 letters or so.  In the
                    same process the global matrix entries on the SAME pairs and matrix (the
                    yardstick) and the ratios.  Writes profiles/batch_local_time.json.

  --ends N [N ..]   the semi-global entries (nw_score_batch_semi, nw_align_batch_semi) with each of
                    these `ends` (3: all of s2 inside s1, 15: overlap, ..) on pairs over --matrix's
                    20-letter alphabet and matrix, gap -1 and --gap-open (default -11); every pair
                    holds a planted fit (--local's planted segments).  In the same process, before
                    them, the global matrix entries on the SAME pairs and matrix (the yardstick)
                    and the ratios.  Writes profiles/batch_semi_time.json.

  --band W [W ..]   the banded entries (nw_score_batch_banded, nw_align_batch_banded) with each of these
                    band widths (a width of 1000000 covers every table here) on --matrix's pairs and
                    matrix, gap -1 and --gap-open (default -11).  In the same process, before them,
                    the global matrix entries on the SAME pairs and matrix (the yardstick: code the
                    band does not touch) and the ratios, each next to the ratio predicted from the
                    iterations a strip sweeps (predict_band).  Writes
                    profiles/batch_banded_time.json.

  --gap2 O2,E2      the two-piece entries (nw_score_batch_dual, nw_align_batch_dual) on --matrix's pairs
                    and matrix: a run of L costs max(G + L * g, O2 + L * E2) with G = --gap-open
                    (default -4) and g = -2 (minimap2's -O4,24 -E2,1 with --gap2 -24,-1).  In the
                    same process, before them, the matrix entries on the SAME pairs and matrix under
                    piece 1 alone (the yardstick: code the second piece does not touch) and the
                    ratios, the score kernels' next to the ratio predicted from the instructions a
                    64-step iteration issues (predict_dual).  Writes
                    profiles/batch_dual_time.json.  (A value that starts with a minus sign is
                    written with the equals sign: --gap2=-24,-1.)

  --gap2 O2,E2 --band W [W ..]
                    the two-piece entries inside a band (nw_score_batch_dual_banded, nw_align_batch_
                    dual_banded) per width W on --gap2's pairs, matrix and costs.  In the same process,
                    before them, the unbanded two-piece entries on the SAME pairs (the yardstick: code
                    the band does not touch) and the ratios, the score kernels' next to the ratio
                    predicted from the iterations a strip sweeps, masked and plain, each weighted by
                    the instructions it issues (predict_dual_band).  Writes
                    profiles/batch_dual_banded_time.json.  --gap2 alone and --band alone are unchanged.

The score kernel's yardstick is the checkpoint sweep's pace on one huge table
(profiles/ckpt_time.json: 262144^2 in 20.62 ms); `fraction_of_sweep_pace` states it.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-needleman-wunsch_amd"))
import torch  # noqa: E402

import nwhip  # noqa: E402

SHAPES = {"150": (16384, 150, 150), "1000": (4096, 1000, 1000), "8000": (256, 8000, 8000), "mixed": (2048, 100, 4000)}
SWEEP_GCUPS = 262144 * 262144 / (20.62 * 1e6)  # profiles/ckpt_time.json

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="all")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--loop-reps", type=int, default=5)
ap.add_argument("--gap-open", type=int, default=None)
ap.add_argument("--matrix", type=int, default=None, nargs="?", const=20)
ap.add_argument("--local", action="store_true")
ap.add_argument("--ends", type=int, default=None, nargs="+")
ap.add_argument("--band", type=int, default=None, nargs="+")
ap.add_argument("--gap2", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.gap2 is not None:
    args.gap2 = tuple(int(x) for x in args.gap2.split(","))
    assert len(args.gap2) == 2
    if args.gap_open is None:
        args.gap_open = -4
if args.local or args.ends is not None or args.band is not None or args.gap2 is not None:
    args.matrix = 20
if args.matrix is not None and args.gap_open is None:
    args.gap_open = -11
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "batch_dual_banded_time.json"
                            if args.gap2 is not None and args.band is not None else
                            "batch_dual_time.json" if args.gap2 is not None else
                            "batch_banded_time.json" if args.band is not None else
                            "batch_semi_time.json" if args.ends is not None else
                            "batch_local_time.json" if args.local else
                            "batch_matrix_time.json" if args.matrix is not None else
                            "batch_time.json" if args.gap_open is None else "batch_affine_time.json")
scheme = (1, 0, -1)
med = statistics.median


def wall(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def make_pairs(name, letters=None):
    """The shape's pairs over the bytes 1..4, or over `letters` (same seed, same sizes)."""
    npairs, lo, hi = SHAPES[name]
    rng = np.random.default_rng(npairs)
    if name == "mixed":
        lens = rng.integers(lo, hi + 1, (npairs, 2))
    else:
        lens = np.tile([lo, hi], (npairs, 1))
    if letters is None:
        letters = np.arange(1, 5, dtype=np.int8)
    k = len(letters)
    return [(letters[rng.integers(0, k, int(a))], letters[rng.integers(0, k, int(b))]) for a, b in lens]


def make_matrix(n):
    """A seeded random n-letter alphabet and a seeded symmetric matrix with entries in -4..11."""
    rng = np.random.default_rng(62 + n)
    letters = np.sort(rng.choice(np.arange(1, 128), n, replace=False)).astype(np.int8)
    sc = rng.integers(-4, 12, (n, n))
    sc = np.triu(sc) + np.triu(sc, 1).T
    return letters, nwhip.SubMatrix(letters.tolist(), sc, other=int(letters[0]))


def make_local_matrix(n):
    """make_matrix's alphabet under a seeded symmetric matrix of negative expected score."""
    rng = np.random.default_rng(162 + n)
    letters = np.sort(np.random.default_rng(62 + n).choice(np.arange(1, 128), n, replace=False)).astype(np.int8)
    sc = rng.integers(-6, 2, (n, n))
    sc = np.triu(sc, 1) + np.triu(sc, 1).T + np.diag(rng.integers(3, 12, n))
    assert sc.mean() < -1
    return letters, nwhip.SubMatrix(letters.tolist(), sc, other=int(letters[0]))


def plant_segments(pairs, letters, seed):
    """Into every s2 a mutated copy of a stretch of its s1."""
    rng = np.random.default_rng(seed)
    out = []
    for a, b in pairs:
        b = b.copy()
        m = min(a.size, b.size)
        seg = int(rng.integers(m // 4, 3 * m // 4 + 1))
        src = a[int(rng.integers(0, a.size - seg + 1)):][:seg].copy()
        hit = rng.random(seg) < 0.1
        src[hit] = letters[rng.integers(0, len(letters), int(hit.sum()))]
        parts, at = [], 0
        while at < seg:
            nxt = min(seg, at + int(rng.integers(40, 81)))
            parts.append(src[at:nxt])
            run = int(rng.integers(1, 21))
            if rng.random() < 0.5:
                parts.append(letters[rng.integers(0, len(letters), run)])  # ups
                at = nxt
            else:
                at = nxt + run                                            # lefts
        cp = np.concatenate(parts)[:b.size]
        at2 = int(rng.integers(0, b.size - cp.size + 1))
        b[at2:at2 + cp.size] = cp
        out.append((a, b))
    return out


def time_entries(pairs, cells, score_f, align_f, key=lambda r: r):
    """(score entry, align entry, scores): medians of --reps calls after a warm-up each."""
    score_f(pairs, return_stats=True)
    rs = [wall(lambda: score_f(pairs, return_stats=True)) for _ in range(args.reps)]
    scores = rs[0][1][0]
    fill = med(r[1][1].fill_ms for r in rs)
    se = {"fill_ms": round(fill, 3), "wall_ms": round(med(r[0] for r in rs), 3),
          "gcups_kernel": round(cells / (fill * 1e6), 1), "workers": int(rs[0][1][1].waves)}
    align_f(pairs)
    ra = [wall(lambda: align_f(pairs)) for _ in range(args.reps)]
    st = ra[0][1][2]
    afill, awalk = med(r[1][2].fill_ms for r in ra), med(r[1][2].walk_ms for r in ra)
    assert np.array_equal(key(ra[0][1][0]), key(scores))
    ae = {"fill_ms": round(afill, 3), "walk_ms": round(awalk, 3), "fill_walk_ms": round(afill + awalk, 3),
          "wall_ms": round(med(r[0] for r in ra), 3), "gcups_kernel": round(cells / (afill * 1e6), 1),
          "gcups_fill_walk": round(cells / ((afill + awalk) * 1e6), 1), "chunks": int(st.chunks),
          "dir_bytes": int(st.dir_bytes), "peak_bytes": int(st.peak_bytes)}
    return se, ae, scores


def run_affine(name):
    go = args.gap_open
    pairs = make_pairs(name)
    cells = sum(a.size * b.size for a, b in pairs)
    e = {"shape": name, "pairs": len(pairs), "cells": int(cells), "gap_open": go,
         "lengths": "uniform %d..%d" % SHAPES[name][1:] if name == "mixed" else "%d x %d" % SHAPES[name][1:]}
    ls, la, _ = time_entries(pairs, cells, lambda p, **kw: nwhip.score_batch(p, scheme, **kw),
                             lambda p: nwhip.align_batch(p, scheme))
    s, a, _ = time_entries(pairs, cells, lambda p, **kw: nwhip.score_batch_affine(p, scheme, go, **kw),
                           lambda p: nwhip.align_batch_affine(p, scheme, go))
    e["linear_score_batch"], e["linear_align_batch"] = ls, la
    e["score_batch_affine"], e["align_batch_affine"] = s, a
    e["score_affine_over_linear"] = round(s["fill_ms"] / ls["fill_ms"], 2)
    e["align_fill_affine_over_linear"] = round(a["fill_ms"] / la["fill_ms"], 2)
    e["align_fill_walk_affine_over_linear"] = round(a["fill_walk_ms"] / la["fill_walk_ms"], 2)
    print(json.dumps(e), flush=True)
    return e


def run_matrix(name):
    go, ge = args.gap_open, -1
    letters, mat = make_matrix(args.matrix)
    pairs4 = make_pairs(name)
    pairs = make_pairs(name, letters)
    cells = sum(a.size * b.size for a, b in pairs)
    assert cells == sum(a.size * b.size for a, b in pairs4)
    e = {"shape": name, "pairs": len(pairs), "cells": int(cells), "gap_open": go, "gap": ge, "letters": args.matrix,
         "matrix_entries": [int(mat.scores.min()), int(mat.scores.max())],
         "lengths": "uniform %d..%d" % SHAPES[name][1:] if name == "mixed" else "%d x %d" % SHAPES[name][1:]}
    fs, fa, _ = time_entries(pairs4, cells, lambda p, **kw: nwhip.score_batch_affine(p, (1, 0, ge), go, **kw),
                             lambda p: nwhip.align_batch_affine(p, (1, 0, ge), go))
    s, a, _ = time_entries(pairs, cells, lambda p, **kw: nwhip.score_batch_matrix(p, mat, ge, go, **kw),
                           lambda p: nwhip.align_batch_matrix(p, mat, ge, go))
    e["score_batch_affine"], e["align_batch_affine"] = fs, fa
    e["score_batch_matrix"], e["align_batch_matrix"] = s, a
    e["score_matrix_over_affine"] = round(s["fill_ms"] / fs["fill_ms"], 2)
    e["align_fill_matrix_over_affine"] = round(a["fill_ms"] / fa["fill_ms"], 2)
    e["align_fill_walk_matrix_over_affine"] = round(a["fill_walk_ms"] / fa["fill_walk_ms"], 2)
    print(json.dumps(e), flush=True)
    return e


def run_local(name):
    go, ge = args.gap_open, -1
    letters, mat = make_local_matrix(20)
    pairs = plant_segments(make_pairs(name, letters), letters, 7 + len(name))
    cells = sum(a.size * b.size for a, b in pairs)
    e = {"shape": name, "pairs": len(pairs), "cells": int(cells), "gap_open": go, "gap": ge, "letters": 20,
         "matrix_entries": [int(mat.scores.min()), int(mat.scores.max())],
         "matrix_mean": round(float(mat.scores.mean()), 2),
         "lengths": "uniform %d..%d" % SHAPES[name][1:] if name == "mixed" else "%d x %d" % SHAPES[name][1:]}
    gs, ga, _ = time_entries(pairs, cells, lambda p, **kw: nwhip.score_batch_matrix(p, mat, ge, go, **kw),
                             lambda p: nwhip.align_batch_matrix(p, mat, ge, go))
    s, a, hits = time_entries(pairs, cells, lambda p, **kw: nwhip.score_batch_local(p, mat, ge, go, **kw),
                              lambda p: nwhip.align_batch_local(p, mat, ge, go), key=lambda h: h["score"])
    e["median_local_score"] = int(np.median(hits["score"]))
    e["score_batch_matrix"], e["align_batch_matrix"] = gs, ga
    e["score_batch_local"], e["align_batch_local"] = s, a
    e["score_local_over_matrix"] = round(s["fill_ms"] / gs["fill_ms"], 2)
    e["align_fill_local_over_matrix"] = round(a["fill_ms"] / ga["fill_ms"], 2)
    e["align_fill_walk_local_over_matrix"] = round(a["fill_walk_ms"] / ga["fill_walk_ms"], 2)
    print(json.dumps(e), flush=True)
    return e


def run_semi(name):
    go, ge = args.gap_open, -1
    letters, mat = make_matrix(20)
    pairs = plant_segments(make_pairs(name, letters), letters, 7 + len(name))
    cells = sum(a.size * b.size for a, b in pairs)
    e = {"shape": name, "pairs": len(pairs), "cells": int(cells), "gap_open": go, "gap": ge, "letters": 20,
         "matrix_entries": [int(mat.scores.min()), int(mat.scores.max())],
         "lengths": "uniform %d..%d" % SHAPES[name][1:] if name == "mixed" else "%d x %d" % SHAPES[name][1:]}
    gs, ga, glob = time_entries(pairs, cells, lambda p, **kw: nwhip.score_batch_matrix(p, mat, ge, go, **kw),
                                lambda p: nwhip.align_batch_matrix(p, mat, ge, go))
    e["score_batch_matrix"], e["align_batch_matrix"] = gs, ga
    e["median_global_score"] = int(np.median(glob))
    for ends in args.ends:
        s, a, hits = time_entries(pairs, cells, lambda p, **kw: nwhip.score_batch_semi(p, mat, ge, go, ends, **kw),
                                  lambda p: nwhip.align_batch_semi(p, mat, ge, go, ends), key=lambda h: h["score"])
        e["ends_%d" % ends] = {
            "median_score": int(np.median(hits["score"])), "score_batch_semi": s, "align_batch_semi": a,
            "score_semi_over_matrix": round(s["fill_ms"] / gs["fill_ms"], 3),
            "align_fill_semi_over_matrix": round(a["fill_ms"] / ga["fill_ms"], 3),
            "align_fill_walk_semi_over_matrix": round(a["fill_walk_ms"] / ga["fill_walk_ms"], 3)}
    print(json.dumps(e), flush=True)
    return e


# VALU instructions of the masked 64-step iteration over the matrix kernel's, from the ISA of
# the two score kernels
MASKED_OVER_PLAIN = 1.12


def band_iterations(n1, n2, w):
    """(masked, plain, all): the 64-step iterations the banded sweep runs with and without the
    mask, and those the matrix sweep runs, summed over the pair's strips (the geometry of
    csrc/nw_batch.h batch_banded_* and csrc/nw_batch_banded.hip banded_pair)."""
    dlo = max(min(0, n2 - n1) - w, -n1 - 1024)
    dhi = min(max(0, n2 - n1) + w, n2 + 1024)
    iters, nblocks = n2 // 64 + 2, n2 // 64 + 1
    slots = min(iters, (dhi - dlo + 319 + 63) // 64 + 2)
    masked = plain = 0
    for p in range((n1 + 255) // 256):
        c0 = 256 * p
        it0 = max(0, (c0 + dlo) >> 6)
        itl = min(nblocks, ((c0 + 319 + dhi) >> 6) + 1, it0 + slots - 1)
        for it in range(it0, itl + 1):
            if 64 * it - c0 - 319 >= dlo and 64 * it + 62 - c0 <= dhi:
                plain += 1
            else:
                masked += 1
    return masked, plain, ((n1 + 255) // 256) * iters


def predict_band(pairs, w):
    """The banded score kernel's time over the matrix score kernel's on the same pairs, from
    iteration counts alone: every iteration costs its VALU instructions."""
    m = pl = al = 0
    for a, b in pairs:
        x, y, z = band_iterations(a.size, b.size, w)
        m, pl, al = m + x, pl + y, al + z
    return round((m * MASKED_OVER_PLAIN + pl) / al, 3)


def run_banded(name):
    go, ge = args.gap_open, -1
    letters, mat = make_matrix(20)
    pairs = make_pairs(name, letters)
    cells = sum(a.size * b.size for a, b in pairs)
    e = {"shape": name, "pairs": len(pairs), "cells": int(cells), "gap_open": go, "gap": ge, "letters": 20,
         "lengths": "uniform %d..%d" % SHAPES[name][1:] if name == "mixed" else "%d x %d" % SHAPES[name][1:]}
    gs, ga, glob = time_entries(pairs, cells, lambda p, **kw: nwhip.score_batch_matrix(p, mat, ge, go, **kw),
                                lambda p: nwhip.align_batch_matrix(p, mat, ge, go))
    e["score_batch_matrix"], e["align_batch_matrix"] = gs, ga
    for w in args.band:
        s, a, sc = time_entries(pairs, cells, lambda p, **kw: nwhip.score_batch_banded(p, mat, ge, go, w, **kw),
                                lambda p: nwhip.align_batch_banded(p, mat, ge, go, w))
        pred, got = predict_band(pairs, w), round(s["fill_ms"] / gs["fill_ms"], 3)
        e["band_%d" % w] = {
            "scores_equal_global": int((sc == glob).sum()), "score_batch_banded": s, "align_batch_banded": a,
            "score_banded_over_matrix": got, "predicted_score_banded_over_matrix": pred,
            "explained": bool(abs(got - pred) <= 0.15),
            "align_fill_banded_over_matrix": round(a["fill_ms"] / ga["fill_ms"], 3),
            "align_fill_walk_banded_over_matrix": round(a["fill_walk_ms"] / ga["fill_walk_ms"], 3),
            "dir_bytes_banded_over_matrix": round(a["dir_bytes"] / ga["dir_bytes"], 4)}
    print(json.dumps(e), flush=True)
    return e


# Instructions a 64-step iteration of the score kernels issues, from their ISA (the narrow
# form, which these costs take): VALU + v_readlane + v_writelane of the plain iteration's
# block and of the EDGE iteration's, two-piece kernel and matrix kernel
DUAL_ITER = {"plain": 3710 + 384 + 189, "edge": 4769 + 384 + 189}
MATRIX_ITER = {"plain": 1721 + 256 + 126, "edge": 2466 + 256 + 126}


def predict_dual(pairs):
    """The two-piece score kernel's time over the matrix score kernel's on the same pairs: both
    run the same iterations, every iteration costs the instructions it issues."""
    plain = edge = 0
    for a, b in pairs:
        nblocks = b.size // 64 + 1
        e = sum(1 for it in range(nblocks + 1) if it == 0 or 64 * it + 63 > b.size)
        strips = (a.size + 255) // 256
        edge, plain = edge + strips * e, plain + strips * (nblocks + 1 - e)
    cost = lambda c: plain * c["plain"] + edge * c["edge"]
    return round(cost(DUAL_ITER) / cost(MATRIX_ITER), 3)


def run_dual(name):
    go, ge = args.gap_open, -2
    go2, ge2 = args.gap2
    letters, mat = make_matrix(20)
    pairs = make_pairs(name, letters)
    cells = sum(a.size * b.size for a, b in pairs)
    e = {"shape": name, "pairs": len(pairs), "cells": int(cells), "gap_open": go, "gap": ge, "gap_open2": go2,
         "gap2": ge2, "letters": 20, "matrix_entries": [int(mat.scores.min()), int(mat.scores.max())],
         "lengths": "uniform %d..%d" % SHAPES[name][1:] if name == "mixed" else "%d x %d" % SHAPES[name][1:]}
    gs, ga, glob = time_entries(pairs, cells, lambda p, **kw: nwhip.score_batch_matrix(p, mat, ge, go, **kw),
                                lambda p: nwhip.align_batch_matrix(p, mat, ge, go))
    dual = dict(gap=ge, gap_open=go, gap2=ge2, gap_open2=go2)
    s, a, sc = time_entries(pairs, cells, lambda p, **kw: nwhip.score_batch_dual(p, mat, **dual, **kw),
                            lambda p: nwhip.align_batch_dual(p, mat, **dual))
    assert (sc >= glob).all()   # (a second piece can only raise a score)
    pred, got = predict_dual(pairs), round(s["fill_ms"] / gs["fill_ms"], 3)
    e["score_batch_matrix"], e["align_batch_matrix"] = gs, ga
    e["score_batch_dual"], e["align_batch_dual"] = s, a
    e["pairs_the_second_piece_raises"] = int((sc > glob).sum())
    e["score_dual_over_matrix"], e["predicted_score_dual_over_matrix"] = got, pred
    e["explained"] = bool(abs(got - pred) <= 0.15)
    e["align_fill_dual_over_matrix"] = round(a["fill_ms"] / ga["fill_ms"], 3)
    e["align_fill_walk_dual_over_matrix"] = round(a["fill_walk_ms"] / ga["fill_walk_ms"], 3)
    e["dir_bytes_dual_over_matrix"] = round(a["dir_bytes"] / ga["dir_bytes"], 4)
    print(json.dumps(e), flush=True)
    return e


# Instructions a 64-step iteration of the banded two-piece score kernel issues, from its ISA (the
# narrow form): VALU + v_readlane + v_writelane of the four variants' blocks; the
# unbanded two-piece kernel's are DUAL_ITER
DUAL_BANDED_ITER = {("plain", "plain"): 3692 + 384 + 189, ("plain", "edge"): 4769 + 384 + 189,
                    ("masked", "plain"): 4986 + 384 + 189, ("masked", "edge"): 6048 + 384 + 189}


def dual_band_iterations(n1, n2, w):
    """{(masked / plain, edge / plain): count} of the iterations the banded two-piece sweep runs
    (the geometry of band_iterations), and {edge / plain: count} of those the unbanded one runs."""
    dlo = max(min(0, n2 - n1) - w, -n1 - 1024)
    dhi = min(max(0, n2 - n1) + w, n2 + 1024)
    iters, nblocks = n2 // 64 + 2, n2 // 64 + 1
    slots = min(iters, (dhi - dlo + 319 + 63) // 64 + 2)
    strips = (n1 + 255) // 256
    edge = lambda it: "edge" if it == 0 or 64 * it + 63 > n2 else "plain"
    got = {k: 0 for k in DUAL_BANDED_ITER}
    for p in range(strips):
        c0 = 256 * p
        it0 = max(0, (c0 + dlo) >> 6)
        itl = min(nblocks, ((c0 + 319 + dhi) >> 6) + 1, it0 + slots - 1)
        for it in range(it0, itl + 1):
            inside = 64 * it - c0 - 319 >= dlo and 64 * it + 62 - c0 <= dhi
            got[("plain" if inside else "masked", edge(it))] += 1
    full = {"edge": 0, "plain": 0}
    for it in range(iters):
        full[edge(it)] += strips
    return got, full


def predict_dual_band(pairs, w):
    """(the banded two-piece score kernel's time over the unbanded one's on the same pairs: every
    iteration costs the instructions it issues; the iterations: masked, plain, all)."""
    num = den = 0
    cnt = {"masked": 0, "plain": 0, "all": 0}
    for a, b in pairs:
        got, full = dual_band_iterations(a.size, b.size, w)
        num += sum(n * DUAL_BANDED_ITER[k] for k, n in got.items())
        den += sum(n * DUAL_ITER[k] for k, n in full.items())
        for (m, _), n in got.items():
            cnt[m] += n
        cnt["all"] += sum(full.values())
    return round(num / den, 3), cnt


def run_dual_banded(name):
    go, ge = args.gap_open, -2
    go2, ge2 = args.gap2
    letters, mat = make_matrix(20)
    pairs = make_pairs(name, letters)
    cells = sum(a.size * b.size for a, b in pairs)
    e = {"shape": name, "pairs": len(pairs), "cells": int(cells), "gap_open": go, "gap": ge, "gap_open2": go2,
         "gap2": ge2, "letters": 20,
         "lengths": "uniform %d..%d" % SHAPES[name][1:] if name == "mixed" else "%d x %d" % SHAPES[name][1:]}
    dual = dict(gap=ge, gap_open=go, gap2=ge2, gap_open2=go2)
    gs, ga, glob = time_entries(pairs, cells, lambda p, **kw: nwhip.score_batch_dual(p, mat, **dual, **kw),
                                lambda p: nwhip.align_batch_dual(p, mat, **dual))
    e["score_batch_dual"], e["align_batch_dual"] = gs, ga
    for w in args.band:
        s, a, sc = time_entries(pairs, cells,
                                lambda p, **kw: nwhip.score_batch_dual_banded(p, mat, band=w, **dual, **kw),
                                lambda p: nwhip.align_batch_dual_banded(p, mat, band=w, **dual))
        assert (sc <= glob).all()   # (a band can only lower a score)
        (pred, cnt), got = predict_dual_band(pairs, w), round(s["fill_ms"] / gs["fill_ms"], 3)
        assert a["dir_bytes"] == sum(nwhip.batch_dual_banded_dir_bytes(x.size, y.size, w) for x, y in pairs)
        e["band_%d" % w] = {
            "scores_equal_unbanded": int((sc == glob).sum()), "score_batch_dual_banded": s,
            "align_batch_dual_banded": a, "iterations": cnt,
            "score_banded_over_dual": got, "predicted_score_banded_over_dual": pred,
            "explained": bool(abs(got - pred) <= 0.15),
            "align_fill_banded_over_dual": round(a["fill_ms"] / ga["fill_ms"], 3),
            "align_fill_walk_banded_over_dual": round(a["fill_walk_ms"] / ga["fill_walk_ms"], 3),
            "dir_bytes_per_pair": int(a["dir_bytes"] // len(pairs)),
            "dir_bytes_banded_over_dual": round(a["dir_bytes"] / ga["dir_bytes"], 4)}
    print(json.dumps(e), flush=True)
    return e


def run(name):
    pairs = make_pairs(name)
    cells = sum(a.size * b.size for a, b in pairs)
    e = {"shape": name, "pairs": len(pairs), "cells": int(cells),
         "lengths": "uniform %d..%d" % SHAPES[name][1:] if name == "mixed" else "%d x %d" % SHAPES[name][1:]}
    # the batched calls
    nwhip.score_batch(pairs, scheme)
    rs = [wall(lambda: nwhip.score_batch(pairs, scheme, return_stats=True)) for _ in range(args.reps)]
    scores = rs[0][1][0]
    fill = med(r[1][1].fill_ms for r in rs)
    e["score_batch"] = {"fill_ms": round(fill, 3), "wall_ms": round(med(r[0] for r in rs), 3),
                        "gcups_kernel": round(cells / (fill * 1e6), 1), "workers": int(rs[0][1][1].waves),
                        "fraction_of_sweep_pace": round(cells / (fill * 1e6) / SWEEP_GCUPS, 3)}
    nwhip.align_batch(pairs, scheme)
    ra = [wall(lambda: nwhip.align_batch(pairs, scheme)) for _ in range(args.reps)]
    st = ra[0][1][2]
    afill, awalk = med(r[1][2].fill_ms for r in ra), med(r[1][2].walk_ms for r in ra)
    assert np.array_equal(ra[0][1][0], scores)
    e["align_batch"] = {"fill_ms": round(afill, 3), "walk_ms": round(awalk, 3), "wall_ms": round(med(r[0] for r in ra), 3),
                        "gcups_kernel": round(cells / (afill * 1e6), 1), "chunks": int(st.chunks),
                        "dir_bytes": int(st.dir_bytes), "peak_bytes": int(st.peak_bytes)}
    # the same pairs through the one-pair entries
    for a, b in pairs[:32]:
        nwhip.score_sweep(a, b, scheme)
        nwhip.align(a, b, scheme)
    ls = [wall(lambda: [nwhip.score_sweep(a, b, scheme).score for a, b in pairs]) for _ in range(args.loop_reps)]
    assert np.array_equal(np.array(ls[0][1], np.int32), scores)
    la = [wall(lambda: [nwhip.align(a, b, scheme)[0].score for a, b in pairs]) for _ in range(args.loop_reps)]
    assert np.array_equal(np.array(la[0][1], np.int32), scores)
    e["loop"] = {"reps": args.loop_reps, "nw_score_wall_ms": round(med(r[0] for r in ls), 1),
                 "nw_align_wall_ms": round(med(r[0] for r in la), 1)}
    e["score_loop_over_batch"] = round(e["loop"]["nw_score_wall_ms"] / e["score_batch"]["wall_ms"], 1)
    e["align_loop_over_batch"] = round(e["loop"]["nw_align_wall_ms"] / e["align_batch"]["wall_ms"], 1)
    print(json.dumps(e), flush=True)
    return e


rec = {"shapes": {}}
if os.path.exists(args.out):
    with open(args.out) as f:
        rec = json.load(f)
rec.update({"device": torch.cuda.get_device_name(0), "library": nwhip.version(), "scheme": list(scheme),
            "reps": args.reps, "sweep_yardstick_gcups": round(SWEEP_GCUPS, 1)})
for name in (list(SHAPES) if args.shape == "all" else [args.shape]):
    rec["shapes"][name] = (run_dual_banded(name) if args.gap2 is not None and args.band is not None else run_dual(name) if args.gap2 is not None else run_banded(name) if args.band is not None else run_semi(name) if args.ends is not None else run_local(name) if args.local else run_matrix(name) if args.matrix is not None else
                           run(name) if args.gap_open is None else run_affine(name))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
