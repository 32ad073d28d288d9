#!/usr/bin/env python3
"""Online decode at serving size: the configs[4] model (10 words x 5 states, 8 mixtures, D = 39, fp64) and `--streams`
(default 4 096) live seven-word utterances taking `--tick` (default 20) frames per tick -- 0.2 s of audio at 100 frames/s.

Per tick (host clock around work that ends in a device synchronise, medians over the ticks in which every stream still
has frames): the whole `OnlineDecoder.push` call and its parts -- batch creation + upload, likelihoods, the online sweep
-- `result()` of all streams, and the streams one GPU sustains in real time (streams x tick duration / call time).

Two comparisons in the same process, on the same frames:
  (a) ONE-SHOT SWEEP: the online sweep summed over all ticks (`push_batch(first, count)` on the resident whole-utterance
      batch: the dynamic program alone) against the one-shot loop kernel on the complete utterances (`viterbi_labels`'s
      forward sweep + back-trace, and `viterbi(want_path=False)`: the sweep without decision bits);
  (b) RE-DECODING THE PREFIX: `push` + `result()` every tick against what a caller had to do without the online form:
      `decode_batch` on the prefix every tick (upload, likelihoods and decode of everything heard so far).
Both are reported, neither is gated.  Kernel times come from a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_online.py --no-prefix
(viterbi_online_kernel per tick and in total, viterbi_loop_kernel once, the likelihood kernel per tick).
usage: time_online.py [--streams 4096] [--tick 20] [--no-prefix] [--out result.json]"""
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
ap.add_argument("--tick", type=int, default=20)
ap.add_argument("--no-prefix", action="store_true", help="leave comparison (b)'s prefix decodes out (profiler runs)")
ap.add_argument("--out", default=None)
args = ap.parse_args()

K, W, n, M, D = 7, 10, 5, 8, 39
U, TICK = args.streams, args.tick
ctx = _hip.default_context(0)
wl = bench.synth_workload(1005, 1, W=W, n=n, M=M, D=D)
means, vars_, trans = wl["means"], wl["vars"], wl["trans"]
rng = np.random.default_rng(1005)
words = rng.integers(0, W, size=(U, K))
Tw = rng.integers(30, 61, size=(U, K))
seg_len = Tw.reshape(-1)
seg_off = np.concatenate([[0], np.cumsum(seg_len)])
seg = np.repeat(np.arange(len(seg_len)), seg_len)
t = np.arange(int(seg_off[-1])) - seg_off[seg]
st = np.minimum(t * n // seg_len[seg], n - 1)
idx = (words.reshape(-1)[seg] * n + st) * M + rng.integers(0, M, size=len(seg))
X = means.reshape(-1, D)[idx] + np.sqrt(vars_).reshape(-1, D)[idx] * rng.standard_normal((len(seg), D))
off = np.concatenate([[0], np.cumsum(Tw.sum(axis=1))]).astype(np.int64)
T = np.diff(off)
xs = [X[off[u]:off[u + 1]] for u in range(U)]


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
n_ticks = int(-(-T.max() // TICK))
full_ticks = int(T.min() // TICK)                       # ticks in which every stream still has a whole chunk
ids = np.arange(U)
chunks = [[x[k * TICK:(k + 1) * TICK] for x in xs] for k in range(n_ticks)]


def clock(fn):
    ctx.sync()
    t0 = time.perf_counter()
    r = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, r


# ---- the serving loop: push (and its parts) + result every tick; round 0 warms up ----
on = dec.online(U, int(T.max()))
rows = None
for rnd in range(2):
    on.reset()
    rows = []
    for k in range(n_ticks):
        ms_push, _ = clock(lambda: on.push(ids, chunks[k]))
        ms_result, res = clock(lambda: on.result())
        rows.append(dict(tick=k, push_ms=ms_push, result_ms=ms_result))
online_words = res[0]
# the parts of a push, on the same chunks (a second session so that the first keeps its results)
on2 = dec.online(U, int(T.max()))
for rnd in range(2):
    on2.reset()
    for k in range(n_ticks):
        ms_batch, b = clock(lambda: _hip.Batch(ctx, chunks[k], dtype=dec.dtype))
        ms_loglik, _ = clock(lambda: b.loglik(dec.gmm, fetch=False))
        ms_sweep, _ = clock(lambda: on2.push_batch(ids, b))
        b.close()
        rows[k].update(batch_upload_ms=ms_batch, loglik_ms=ms_loglik, online_sweep_ms=ms_sweep)
on2.close()

# ---- (a) the dynamic program alone: online sweep over all ticks against the one-shot loop kernel ----
whole = _hip.Batch(ctx, feats=X, offsets=off)
whole.loglik(dec.gmm, fetch=False)
row_word = np.where(dec.row_state >= 0, dec.row_state // n, -1).astype(np.int32)
ml = whole.lengths // (n - 1) + 2
on3 = dec.online(U, int(T.max()))
a = dict(online_sweep_all_ticks_ms=[], one_shot_labels_ms=[], one_shot_no_decisions_ms=[])
for rep in range(4):                                    # alternating; round 0 warms up
    on3.reset()
    ctx.sync()
    t0 = time.perf_counter()
    for k in range(n_ticks):
        first = np.minimum(k * TICK, T)
        on3.push_batch(ids, whole, first=first, count=np.minimum(TICK, T - first))
    ctx.sync()
    ms_on = (time.perf_counter() - t0) * 1e3
    ms_lab, one = clock(lambda: dec.lat.viterbi_labels(whole, row_word, max_labels=ml, as_lists=False, want_end_cost=False))
    ms_fwd, _ = clock(lambda: dec.lat.viterbi(whole, want_path=False, want_end_cost=False))
    if rep:
        a["online_sweep_all_ticks_ms"].append(ms_on)
        a["one_shot_labels_ms"].append(ms_lab)
        a["one_shot_no_decisions_ms"].append(ms_fwd)
w3, r3 = on3.result()
one_words = [one["labels_flat"][one["label_off"][u]:one["label_off"][u] + one["n_labels"][u]].tolist() for u in range(U)]
same = bool(w3 == one_words == online_words and np.array_equal(r3["best_end"], one["best_end"]))
on3.close()
whole.close()

# ---- (b) re-decoding the prefix every tick ----
prefix = None
if not args.no_prefix:
    prefix = []
    for k in range(n_ticks):
        pre = [x[:(k + 1) * TICK] for x in xs]

        def redo():
            b = _hip.Batch(ctx, pre, dtype=dec.dtype)
            try:
                return dec.decode_batch(b)[0]
            finally:
                b.close()
        ms, got = clock(redo)
        prefix.append(ms)
    same = same and got == online_words

med = lambda key, lo=0, hi=full_ticks: float(np.median([r[key] for r in rows[lo:hi]]))
tick_s = TICK / 100.0
out = dict(shape=dict(W=W, n=n, M=M, D=D, streams=int(U), tick_frames=TICK, ticks=n_ticks, full_ticks=full_ticks, frames=int(off[-1])),
           online_equals_one_shot=same,
           per_tick_ms=dict(push_call=med("push_ms"), batch_creation_and_upload=med("batch_upload_ms"), likelihoods=med("loglik_ms"),
                            online_sweep=med("online_sweep_ms"), result_first_tick=rows[0]["result_ms"],
                            result_last_full_tick=rows[full_ticks - 1]["result_ms"]),
           realtime_streams_per_gpu=dict(push_only=U * tick_s * 1e3 / med("push_ms"),
                                         push_and_result_every_tick=U * tick_s * 1e3 / (med("push_ms") + rows[full_ticks - 1]["result_ms"])),
           a_one_shot=dict({k: float(np.median(v)) for k, v in a.items()}, runs={k: [float(x) for x in v] for k, v in a.items()}),
           ticks=rows)
out["a_one_shot"]["online_over_one_shot_labels"] = out["a_one_shot"]["online_sweep_all_ticks_ms"] / out["a_one_shot"]["one_shot_labels_ms"]
if prefix is not None:
    tot_on = float(sum(r["push_ms"] + r["result_ms"] for r in rows))
    out["b_prefix"] = dict(prefix_decode_ms_per_tick=[float(x) for x in prefix], prefix_decode_total_ms=float(sum(prefix)),
                           online_push_and_result_total_ms=tot_on, prefix_over_online=float(sum(prefix)) / tot_on,
                           last_tick_prefix_over_online=float(prefix[-1]) / (rows[-1]["push_ms"] + rows[-1]["result_ms"]))
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
