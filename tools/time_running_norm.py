#!/usr/bin/env python3
"""What the causal running normalisation (RunningNorm) costs a tick of online decode from audio, at the
serving size of tools/time_stream_frontend.py: the configs[4] model (10 words x 5 states, 8 mixtures, D = 39, fp64),
`--streams` (default 4 096) live streams, `--tick` (default 3 200) int16 samples per tick.

Two legs on the same audio, model and decoder, ALTERNATING in one process: `OnlineDecoder.push_audio` per tick through a
front-end with the fixed pair, and through one with a RunningNorm on that pair.  A run is `--ticks` ticks from a reset;
its figure is the median over the ticks behind the first (host clock around work that ends in a device synchronise).
Reported per leg: the median of `--runs` (default 7) runs with min and max; and once per leg, from HIP events
(gh_stream_profile), the device time of the "stack" phase, in which the running pass is counted.
DERIVED, not measured: per tick the pass reads and writes streams x 20 x 39 x 8 B once each (25.6 MB at 4 096) plus
streams x 624 B of carried sums (2.6 MB): far below a millisecond at any plausible rate -- the expected cost is one launch.
usage: time_running_norm.py [--streams 4096] [--tick 3200] [--ticks 8] [--runs 7] [--out profiles/running_norm_4096.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-recognition_amd")):
    sys.path.insert(0, p)
import numpy as np
import bench
import sr.recognition as R
from sr.feature import RunningNorm, StreamingFrontend, feature_stats
from sr.recognition import _hip
from sr.recognition.batch import ContinuousDecoder

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=4096)
ap.add_argument("--tick", type=int, default=3200)
ap.add_argument("--ticks", type=int, default=8)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()

W, n, M, D = 10, 5, 8, 39
U, TICK, NT, RATE = args.streams, args.tick, args.ticks, 16000
ctx = _hip.default_context(0)
wl = bench.synth_workload(1005, 1, W=W, n=n, M=M, D=D)
means, vars_, trans = wl["means"], wl["vars"], wl["trans"]
rng = np.random.default_rng(1006)
L = TICK * NT
tt = np.arange(L) / RATE
pcm = np.empty((U, L), dtype=np.int16)
for lo in range(0, U, 256):
    k = min(256, U - lo)
    f = 200.0 + 1800.0 * rng.random((k, 1)) + 400.0 * np.sin(2 * np.pi * rng.random((k, 1)) * tt * 3)
    x = 3000.0 * np.sin(2 * np.pi * f * tt) + 300.0 * rng.standard_normal((k, L))
    pcm[lo:lo + k] = np.clip(np.round(x), -32768, 32767).astype(np.int16)
pair = feature_stats(list(pcm[:64]), RATE)


def hmm(i):
    h = R.HMM(n)
    h.gmm_states = []
    for s in range(n):
        g = R.GMM(means[i, s, 0].copy(), vars_[i, s, 0].copy(), M)
        g.update_models(means[i, s].copy(), vars_[i, s].copy(), wl["w"][i, s].copy())
        h.gmm_states.append(g)
    h.transitions = trans.copy()
    return h


dec = ContinuousDecoder([hmm(i) for i in range(W)], grammar="loop", ctx=ctx)
ids = np.arange(U)
T_all = int(_hip.stream_frames_ready(L, 400, 160, True))
chunks = [[pcm[u, k * TICK:(k + 1) * TICK] for u in range(U)] for k in range(NT)]
ends = [None] * (NT - 1) + [np.ones(U, dtype=bool)]


def clock(fn):
    ctx.sync()
    t0 = time.perf_counter()
    r = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, r


legs = {}
for name, normalize in (("fixed", pair), ("running", RunningNorm(pair, prior_frames=100, min_std=0.1))):
    fe = StreamingFrontend(U, RATE, normalize=normalize, max_chunk=TICK)
    legs[name] = dict(fe=fe, on=dec.online(U, max_frames=T_all, frontend=fe), runs=[], ticks=[])


def run(leg):
    leg["on"].reset()
    return [clock(lambda: leg["on"].push_audio(ids, chunks[k], ends[k]))[0] for k in range(NT)]


for leg in legs.values():                                  # warm-up, not counted
    run(leg)
for r in range(args.runs):
    for leg in legs.values():
        t = run(leg)
        leg["ticks"].append(t)
        leg["runs"].append(float(np.median(t[1:])))
# the device time of the front-end's phases, one more run per leg with HIP events around them
for leg in legs.values():
    leg["on"].reset()
    leg["fe"].backend.profile(True)
    ph = []
    for k in range(NT):
        b = leg["fe"].push(ids, chunks[k], ends[k])
        ph.append(leg["fe"].backend.phase_ms())
        b.close()
    leg["fe"].backend.profile(False)
    leg["device"] = {key: float(np.median([p[key] for p in ph[1:]])) for key in ("upload", "mfcc", "stack", "carry")}

summary = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
fixed, running = summary(legs["fixed"]["runs"]), summary(legs["running"]["runs"])
stack_ms = legs["fixed"]["device"]["stack"]
outside = max(running["median"] - fixed["max"], fixed["min"] - running["median"], 0.0)
out = dict(shape=dict(W=W, n=n, M=M, D=D, streams=int(U), tick_samples=TICK, ticks=NT, runs=args.runs, sample_rate=RATE),
           push_audio_per_tick_ms=dict(fixed=fixed, running=running),
           running_minus_fixed_median_ms=running["median"] - fixed["median"],
           running_median_outside_fixed_range_by_ms=outside,
           outside_by_more_than_the_stack_phase=bool(outside > stack_ms),
           device_phase_ms={name: leg["device"] for name, leg in legs.items()},
           stack_phase_running_minus_fixed_ms=legs["running"]["device"]["stack"] - stack_ms,
           derived=dict(rows_mb_per_tick_each_way=U * 20 * D * 8 / 1e6, state_mb_per_tick_each_way=U * 2 * D * 8 / 1e6),
           runs_ms={name: leg["runs"] for name, leg in legs.items()},
           ticks_ms={name: leg["ticks"] for name, leg in legs.items()})
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
