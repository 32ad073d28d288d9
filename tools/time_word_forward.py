#!/usr/bin/env python3
"""The forward sweep of the isolated-word recogniser (gh_chain_forward, soft word streams) at the configs[1] shape: 10 words x
5 states, 8 mixtures, D = 39, fp64.

One-shot, `--utts` (default 10 000) utterances of 60 .. 120 frames, likelihoods resident before the clock; the legs alternate
in one process, median of `--reps` (default 7) with min - max:
  (a) `costs(batch)`      the Viterbi end costs: the yardstick (the parent has no forward sweep to compare against);
  (b) `soft_costs(batch)` the forward scores.
Online, `--streams` (default 4 096) streams taking `--tick` (default 20) frames per tick for `--ticks` (default 30) ticks, the
likelihoods of every tick resident before the clock:
  (c) `push` of a plain session against `push` of a soft session (Viterbi sweep + forward sweep), per tick.
Both are host clocks around work that ends in a device synchronise.  No ratio is required; DESIGN.md 4.25 derives what to
expect (per column and lane 8 exp and 4 log of the device library against 15 add / min: instruction bound, not HBM bound).
usage: time_word_forward.py [--utts 10000] [--streams 4096] [--tick 20] [--ticks 30] [--reps 7] [--out profiles/word_forward.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-recognition_amd")):
    sys.path.insert(0, p)
import numpy as np
import bench
import sr.recognition as R
from sr.recognition import _hip
from sr.recognition.batch import IsolatedWordRecognizer

ap = argparse.ArgumentParser()
ap.add_argument("--utts", type=int, default=10000)
ap.add_argument("--streams", type=int, default=4096)
ap.add_argument("--tick", type=int, default=20)
ap.add_argument("--ticks", type=int, default=30)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--distinct", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "word_forward.json"))
args = ap.parse_args()

W, n, M, D = 10, 5, 8, 39
ctx = _hip.default_context(0)
base = min(args.distinct, args.utts)
wl = bench.synth_workload(1101, base, W=W, n=n, M=M, D=D, tmin=60, tmax=120)
means, vars_, trans = wl["means"], wl["vars"], wl["trans"]
distinct = [wl["X"][wl["off"][u]:wl["off"][u + 1]] for u in range(base)]


def hmm(i):
    h = R.HMM(n)
    h.gmm_states = []
    for s in range(n):
        g = R.GMM(means[i, s, 0].copy(), vars_[i, s, 0].copy(), M)
        g.update_models(means[i, s].copy(), vars_[i, s].copy(), wl["w"][i, s].copy())
        h.gmm_states.append(g)
    h.transitions = trans.copy()
    return h


rec = IsolatedWordRecognizer([hmm(i) for i in range(W)], ctx=ctx)


def clock(fn):
    ctx.sync()
    t0 = time.perf_counter()
    r = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, r


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), reps=len(v))


# ---- one-shot: (a) and (b) alternate on one resident batch ----
xs = [distinct[u % base] for u in range(args.utts)]
b = _hip.Batch(ctx, xs, dtype=rec.dtype)
b.loglik(rec.gmm, fetch=False)
frames = int(np.sum(b.lengths))
costs = rec.costs(b)                       # (warm-up of both legs; costs() finds the matrix of the same model again)
soft = rec.soft_costs(b)
t_a, t_b = [], []
for _ in range(args.reps):
    t_a.append(clock(lambda: rec.lat.viterbi(b, want_path=False))[0])
    t_b.append(clock(lambda: rec.lat.chain_forward(b))[0])
b.close()
below = bool(np.all(soft <= costs))
agree = float(np.mean(np.argmin(soft, axis=1) == np.argmin(costs, axis=1)))

# ---- online: (c) a plain and a soft session take the same ticks ----
U, TICK, NT = args.streams, args.tick, args.ticks
long_ = bench.synth_workload(1102, min(base, U), W=W, n=n, M=M, D=D, tmin=NT * TICK, tmax=NT * TICK)
ldist = [long_["X"][long_["off"][u]:long_["off"][u + 1]] for u in range(min(base, U))]
ids = np.arange(U)
plain = _hip.WordStreamSession(ctx, rec.lat, U)
softs = _hip.WordStreamSession(ctx, rec.lat, U, soft=True)
t_plain, t_soft = [], []
for k in range(NT):
    tb = _hip.Batch(ctx, [ldist[u % len(ldist)][k * TICK:(k + 1) * TICK] for u in range(U)], dtype=rec.dtype)
    tb.loglik(rec.gmm, fetch=False)
    t_plain.append(clock(lambda: plain.push(tb, ids))[0])
    t_soft.append(clock(lambda: softs.push(tb, ids))[0])
    tb.close()
same_costs = bool(np.array_equal(plain.result()["costs"], softs.result()["costs"]))
plain.close()
softs.close()

out = dict(shape=dict(W=W, n=n, M=M, D=D, dtype="float64", utterances=args.utts, frames=frames, streams=U, tick_frames=TICK, ticks=NT),
           one_shot=dict(viterbi_costs=stats(t_a), forward_soft_costs=stats(t_b),
                         forward_over_viterbi=float(np.median(t_b) / np.median(t_a)),
                         forward_ns_per_column_and_lane=float(np.median(t_b) * 1e6 / (frames * W))),
           per_tick=dict(plain_push=stats(t_plain[1:]), soft_push=stats(t_soft[1:]),
                         soft_over_plain=float(np.median(t_soft[1:]) / np.median(t_plain[1:]))),
           bytes_per_stream=dict(extra_state_resident=8 * n * W, extra_state_in_and_out_per_tick=2 * 8 * n * W),
           soft_below_costs=below, soft_argmin_equals_viterbi_argmin=agree, soft_session_costs_equal_plain=same_costs)
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
