"""Fill + on-device global traceback per table shape (nw_fill_device + nw_traceback),
rounds aimed at (0, 0) against diagonal rounds (no_aim), on the synthetic seeds 1
and 2 with the shipped scheme (1, 0, -1).  One JSON line per shape, then the same
figures for nw_sw_align at 65536 x 65536 (scheme (1, -1, -1), BASELINE config 5) as
the in-run yardstick.  --out also writes the lines to a file (profiles/align_time.json).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fast-needleman-wunsch_amd"))
import torch  # noqa: E402

import nwhip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="65536x65536,262144x262144,131072x32768,32768x131072", help="n1xn2,...")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--band", type=int, default=0)
ap.add_argument("--max-windows", type=int, default=0)
ap.add_argument("--no-sw", action="store_true", help="skip the nw_sw_align yardstick")
ap.add_argument("--out", default="")
args = ap.parse_args()
SCHEME = (1, 0, -1)
lines = []


def emit(rec):
    line = json.dumps(rec)
    lines.append(line)
    print(line, flush=True)


def leg(ctx, s1, s2, tab, no_aim):
    best = None
    for _ in range(args.reps):
        al, ops, st = ctx.traceback(s1, s2, tab, SCHEME, band=args.band, max_windows=args.max_windows, no_aim=no_aim)
        if best is None or al.traceback_ms < best["traceback_ms"]:
            best = {"traceback_ms": round(al.traceback_ms, 3), "n_ops": int(al.n_ops), "rounds": st.rounds,
                    "windows": st.windows, "tail_ops": int(st.tail_ops),
                    "ns_per_op": round(al.traceback_ms * 1e6 / max(int(al.n_ops), 1), 2), "score": int(al.score)}
    return best, ops


ctx = nwhip.Context(0)
for sh in args.shapes.split(","):
    n1, n2 = (int(x) for x in sh.split("x"))
    h1, h2 = nwhip.synth(1, n1), nwhip.synth(2, n2)
    s1, s2 = torch.from_numpy(h1).cuda(), torch.from_numpy(h2).cuda()
    tab = nwhip.Context.alloc_table(n1, n2)
    ctx.fill(s1, s2, tab, SCHEME)
    fill_ms = min(ctx.fill(s1, s2, tab, SCHEME).kernel_ms for _ in range(args.reps))
    aimed, ops = leg(ctx, s1, s2, tab, False)
    diagonal, ops2 = leg(ctx, s1, s2, tab, True)
    assert (ops == ops2).all() and nwhip.ops_score(h1, h2, ops, SCHEME) == aimed["score"]
    rec = {"what": "nw_fill_device + nw_traceback", "n1": n1, "n2": n2, "scheme": list(SCHEME),
           "fill_ms": round(fill_ms, 3)}
    rec.update(aimed)
    rec["no_aim"] = diagonal
    emit(rec)
    del tab, s1, s2
    torch.cuda.empty_cache()

if not args.no_sw:
    n = 65536
    h1, h2 = nwhip.synth(1, n), nwhip.synth(2, n)
    nwhip.sw_align(h1, h2, (1, -1, -1))
    best = None
    for _ in range(args.reps):
        al, ops = nwhip.sw_align(h1, h2, (1, -1, -1))
        if best is None or al.traceback_ms < best.traceback_ms:
            best = al
    emit({"what": "nw_sw_align (yardstick)", "n1": n, "n2": n, "scheme": [1, -1, -1], "fill_ms": round(best.fill_ms, 3),
          "traceback_ms": round(best.traceback_ms, 3), "n_ops": int(best.n_ops), "rounds": None, "windows": None,
          "ns_per_op": round(best.traceback_ms * 1e6 / max(int(best.n_ops), 1), 2), "score": int(best.score)})
    nwhip.host_release()

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
