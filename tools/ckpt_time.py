"""Times of the checkpoint sweep against its two yardsticks, and of the alignment
beyond HBM; writes profiles/ckpt_time.json (medians of --reps runs in one process).

  * 65536^2 and 262144^2, scheme (1, 0, -1), synth seeds 1 / 2: the sweep (nw_score),
    the stored fill of the same table (Context.fill, AUTO) and the compute-pace
    probe NW_FLAG_TIMING_ONLY | NW_FLAG_DEBUG_NO_STORE, which stores no usable table;
  * 524288^2: nw_align_ckpt with default options -- sweep, re-fill and traceback
    times, blocks, K, peak_bytes, re-filled cells / (n1 * n2).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-needleman-wunsch_amd"))
import torch  # noqa: E402

import nwhip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="65536,262144")
ap.add_argument("--big", type=int, default=524288, help="square aligned beyond HBM (0: skip)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ckpt_time.json"))
args = ap.parse_args()
scheme = (1, 0, -1)
med = statistics.median
rec = {"device": torch.cuda.get_device_name(0), "library": nwhip.version(), "scheme": list(scheme),
       "reps": args.reps, "squares": [], "beyond_hbm": None}


def gcups(n, ms):
    return round(n * n / (ms * 1e6), 1)


for n in (int(x) for x in args.sizes.split(",") if x):
    h1, h2 = nwhip.synth(1, n), nwhip.synth(2, n)
    nwhip.score_sweep(h1, h2, scheme)  # warm-up
    rs = [nwhip.score_sweep(h1, h2, scheme) for _ in range(args.reps)]
    sweep = med(r.kernel_ms for r in rs)
    ctx = nwhip.Context(0)
    d1, d2 = torch.from_numpy(h1).cuda(), torch.from_numpy(h2).cuda()
    tab = nwhip.Context.alloc_table(n, n)
    r0 = ctx.fill(d1, d2, tab, scheme)
    assert r0.score == rs[0].score, (r0.score, rs[0].score)
    fill = med(ctx.fill(d1, d2, tab, scheme).kernel_ms for _ in range(args.reps))
    probe_flags = nwhip.FLAG_TIMING_ONLY | nwhip.FLAG_DEBUG_NO_STORE
    ctx.fill(d1, d2, tab, scheme, flags=probe_flags)
    probe = med(ctx.fill(d1, d2, tab, scheme, flags=probe_flags).kernel_ms for _ in range(args.reps))
    e = {"n": n, "score": int(r0.score), "sweep_ms": round(sweep, 3), "sweep_gcups": gcups(n, sweep),
         "sweep_workers": int(rs[0].waves), "stored_fill_ms": round(fill, 3), "stored_fill_gcups": gcups(n, fill),
         "stored_fill_kernel": int(r0.kernel), "stored_fill_shape": [int(r0.substrips), int(r0.strip_waves)],
         "no_store_probe_ms": round(probe, 3), "no_store_probe_gcups": gcups(n, probe),
         "sweep_over_stored_fill": round(sweep / fill, 3)}
    print(json.dumps(e), flush=True)
    rec["squares"].append(e)
    del tab, d1, d2
    ctx.close()
    torch.cuda.empty_cache()

if args.big:
    n = args.big
    h1, h2 = nwhip.synth(1, n), nwhip.synth(2, n)
    nwhip.host_release()
    runs = []
    for _ in range(args.reps):
        al, ops, st = nwhip.align_ckpt(h1, h2, scheme)
        runs.append((al, st))
    al, st = runs[0]
    e = {"n": n, "score": int(al.score), "n_ops": int(al.n_ops), "blocks": int(st.blocks), "K": int(st.block_rows),
         "peak_bytes": int(st.peak_bytes), "ckpt_bytes": int(st.ckpt_bytes), "block_bytes": int(st.block_bytes),
         "sweep_ms": round(med(s.sweep_ms for _, s in runs), 3),
         "sweep_gcups": gcups(n, med(s.sweep_ms for _, s in runs)),
         "refill_ms": round(med(s.refill_ms for _, s in runs), 3),
         "traceback_ms": round(med(s.traceback_ms for _, s in runs), 3),
         "rounds": int(st.rounds), "windows": int(st.windows),
         "refill_cells_over_table": round(st.refill_cells / (n * n), 4)}
    print(json.dumps(e), flush=True)
    rec["beyond_hbm"] = e

with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print("wrote", args.out)
