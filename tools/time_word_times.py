#!/usr/bin/env python3
"""What word begin times cost at serving size: the configs[4] model (10 words x 5 states, 8 mixtures, D = 39, fp64, loop
grammar) and `--streams` (default 4 096) seven-word utterances, as tools/time_online.py and tools/time_settle.py.

  * `decode_batch` of all utterances as one resident batch (likelihoods computed before the clock starts): words only
    against `want_times=True`, median of `--reps` calls after two warm-up calls;
  * `OnlineDecoder` with all streams taking `--tick` (default 20) frames per tick: the `commit` call and the `result` call
    of every tick, with `times=False` and with `times=True`, medians over the ticks in which every stream still has frames
    (two rounds, the first warms up).
Host clock around calls that end in a device synchronise.  On a tree without word times only the words-only legs run (the
figure to hold the change's words-only legs against: they must lie within the run-to-run spread of that tree).
Derivable beforehand: times add 4 B per word of stores and copy-back, the same bytes as the labels themselves.
The result goes to --out, by default profiles/word_times_<streams>.json (profiles/word_times_4096.json at the serving size); a
run on the parent commit is kept beside it under a name of its own (profiles/word_times_parent_<k>.json).
usage: time_word_times.py [--streams 4096] [--tick 20] [--reps 9] [--out profiles/word_times_4096.json]"""
import argparse, inspect, json, os, sys, time
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
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "word_times_%d.json" % args.streams)

K, W, n, M, D = 7, 10, 5, 8, 39
U, TICK = args.streams, args.tick
HAS_TIMES = "want_times" in inspect.signature(ContinuousDecoder.decode_batch).parameters
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


def clock(fn):
    ctx.sync()
    t0 = time.perf_counter()
    r = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, r


# ---- decode_batch: words only against words with begins
batch = _hip.Batch(ctx, feats=X, offsets=off)
batch.loglik(dec.gmm, fetch=False)
legs = [("words_only", {})] + ([("with_times", dict(want_times=True))] if HAS_TIMES else [])
offline, decoded = {}, {}
for name, kw in legs:
    ms = []
    for rep in range(args.reps + 2):
        m, r = clock(lambda: dec.decode_batch(batch, **kw))
        ms.append(m)
    decoded[name] = r
    offline[name] = dict(median_ms=float(np.median(ms[2:])), min_ms=float(np.min(ms[2:])), max_ms=float(np.max(ms[2:])), reps=args.reps)
batch.close()
n_words = int(sum(len(w) for w in decoded["words_only"][0]))
same_words = (not HAS_TIMES) or decoded["with_times"][0] == decoded["words_only"][0]

# ---- online: commit and result per tick
n_ticks = int(-(-T.max() // TICK))
full_ticks = int(T.min() // TICK)
ids = np.arange(U)
chunks = [[x[k * TICK:(k + 1) * TICK] for x in xs] for k in range(n_ticks)]


def serve(on, timed):
    for rnd in range(2):
        on.reset()
        rows = []
        for k in range(n_ticks):
            on.push(ids, chunks[k])
            ms_commit, _ = clock(lambda: on.commit(ids, want_times=True) if timed else on.commit(ids))
            ms_result, res = clock(lambda: on.result(ids))
            rows.append(dict(tick=k, commit_ms=ms_commit, result_ms=ms_result))
    return rows, res


med = lambda rows, key: float(np.median([r[key] for r in rows[:full_ticks]]))
online, final = {}, {}
for name, timed in [("words_only", False)] + ([("with_times", True)] if HAS_TIMES else []):
    on = dec.online(U, max_frames=int(T.max()), **(dict(times=True) if timed else {}))
    rows, final[name] = serve(on, timed)
    on.close()
    online[name] = dict(commit_call_ms=med(rows, "commit_ms"), result_call_ms=med(rows, "result_ms"), ticks=rows)
checks = dict(decode_batch_words_equal=bool(same_words), online_equals_decode_batch=bool(final["words_only"][0] == decoded["words_only"][0]))
if HAS_TIMES:
    checks["online_begins_equal_decode_batch"] = bool(all(np.array_equal(a, b) for a, b in zip(final["with_times"][1]["begins"],
                                                                                                decoded["with_times"][1]["begins"])))
out = dict(shape=dict(W=W, n=n, M=M, D=D, streams=int(U), tick_frames=TICK, ticks=n_ticks, full_ticks=full_ticks, frames=int(off[-1]),
                      words=n_words, begin_bytes=4 * n_words),
           has_word_times=HAS_TIMES, checks=checks, decode_batch_ms=offline, online_per_tick_ms=online)
print(json.dumps({k: v for k, v in out.items() if k != "online_per_tick_ms"}))
print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "ticks"} for k, v in online.items()}))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
