#!/usr/bin/env python3
"""`result()` of an online session WITHOUT labels and WITHOUT paths: the end costs and the chosen end of every stream, which
is the end kernel (online_end_kernel, csrc/gh_online.hip) between two uploads and two read-backs.  `--streams` (default 4 096)
streams that have each taken one 20-frame tick, 5 states per word, 8 mixtures, D = 39, fp64: the narrow loop session at
W = 10 and the wide loop session at W = 40.  Host clock around the call, a device synchronise before it (the call ends in
its own); `--reps` timed calls after 20 warm-up calls, median with min and max.  Nothing is gated.
usage: time_online_result.py [--streams 4096] [--reps 300] [--out result.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-recognition_amd")):
    sys.path.insert(0, p)
import numpy as np
import bench
import sr.recognition as R
from sr.recognition import _hip
from sr.recognition.batch import ContinuousDecoder

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=4096)
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--out", default=None)
args = ap.parse_args()
U, n, M, D, TICK = args.streams, 5, 8, 39, 20
ctx = _hip.default_context(0)


def time_result(W):
    wl = bench.synth_workload(1000 + W, 1, W=W, n=n, M=M, D=D)
    means, vars_ = wl["means"], wl["vars"]
    rng = np.random.default_rng(W)
    hmms = []
    for i in range(W):
        h = R.HMM(n)
        h.gmm_states = []
        for s in range(n):
            g = R.GMM(means[i, s, 0].copy(), vars_[i, s, 0].copy(), M)
            g.update_models(means[i, s].copy(), vars_[i, s].copy(), wl["w"][i, s].copy())
            h.gmm_states.append(g)
        h.transitions = wl["trans"].copy()
        hmms.append(h)
    dec = ContinuousDecoder(hmms, grammar="loop", ctx=ctx)
    words = rng.integers(0, W, size=U)
    st = np.minimum(np.arange(TICK) * n // TICK, n - 1)
    idx = (words[:, None] * n + st[None, :]) * M + rng.integers(0, M, size=(U, TICK))
    X = means.reshape(-1, D)[idx] + np.sqrt(vars_).reshape(-1, D)[idx] * rng.standard_normal((U, TICK, D))
    on = dec.online(U, TICK)
    assert isinstance(on.session, _hip.OnlineWideSession) == (W > 16)
    on.push(np.arange(U), list(X))
    ms = []
    for rep in range(20 + args.reps):
        ctx.sync()
        t0 = time.perf_counter()
        out = on.session.result()
        ms.append((time.perf_counter() - t0) * 1e3)
    assert np.isfinite(out["end_cost"]).any() and (out["best_end"] >= 0).all()
    on.close()
    v = np.asarray(ms[20:])
    return dict(W=W, ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()), ms_p10=float(np.percentile(v, 10)),
                ms_p90=float(np.percentile(v, 90)))


out = dict(shape=dict(streams=U, n=n, M=M, D=D, frames_taken=TICK, reps=args.reps), narrow_loop_W10=time_result(10),
           wide_loop_W40=time_result(40))
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
