# -*- coding: utf-8 -*-
"""Full likelihood matrix (configs[1] model) at growing batch sizes, kernel time from HIP events on the launch stream
(kernel alone, sustained clocks): does gh_loglik have a fixed cost per launch -- ramp + drain of the last waves -- beside
its rate per frame?  0.25, 0.5, 1, 2 and 4 M frames, `--repeats` measurements of `--launches` back-to-back launches each;
the straight line through the medians gives ns per frame (slope) and the fixed cost (intercept), to be read against the
spread (max - min) of the repeats at 1 M frames.  One JSON line at the end.

    python tools/time_loglik_n.py [--repeats 7] [--launches 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "speech-recognition_amd"))
import bench
from sr.recognition import _hip

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--launches", type=int, default=20)
args = ap.parse_args()

ctx = _hip.default_context()
wl = bench.synth_workload(1002, 10000)
W, n, M, D = wl["W"], wl["n"], wl["M"], wl["D"]
S = W * n
gmm = _hip.PackedGMM(ctx, wl["means"].reshape(S, M, D), wl["vars"].reshape(S, M, D), wl["w"].reshape(S, M))
base = _hip.Batch(ctx, feats=wl["X"], offsets=wl["off"])
off = wl["off"]
batches = []
for utts in (2500, 5000):      # the first quarter / half of the utterances
    batches.append(_hip.Batch(ctx, feats=wl["X"][:off[utts]], offsets=off[:utts + 1]))
batches += [base, base.tile(2), base.tile(4)]
e0, e1 = ctx.new_event(), ctx.new_event()
for _ in range(200):           # sustained clocks before the first measurement
    base.loglik(gmm, fetch=False)
ctx.sync()
rows = []
for b in batches:
    ms = []
    for _ in range(args.repeats):
        for _ in range(3):
            b.loglik(gmm, fetch=False)
        ctx.record(e0)
        for _ in range(args.launches):
            b.loglik(gmm, fetch=False)
        ctx.record(e1)
        ctx.sync()
        ms.append(ctx.elapsed_ms(e0, e1) / args.launches)
    rows.append(dict(frames=int(b.N), ms_median=float(np.median(ms)), ms_min=min(ms), ms_max=max(ms)))
    print("frames %9d  median %.4f ms  min %.4f  max %.4f  %.4f ns per frame" % (b.N, rows[-1]["ms_median"], min(ms), max(ms),
                                                                                 rows[-1]["ms_median"] * 1e6 / b.N), flush=True)
x = np.array([r["frames"] for r in rows], dtype=np.float64)
y = np.array([r["ms_median"] for r in rows])
slope, icpt = np.polyfit(x, y, 1)
at1m = next(r for r in rows if r["frames"] == base.N)
out = dict(tool="time_loglik_n", launches=args.launches, repeats=args.repeats, rows=rows, ns_per_frame=slope * 1e6,
           intercept_us=icpt * 1e3, spread_1m_us=(at1m["ms_max"] - at1m["ms_min"]) * 1e3,
           residual_us=[float(v) * 1e3 for v in (y - (slope * x + icpt))])
print(json.dumps(out), flush=True)
