#!/usr/bin/env python3
"""Online decode of a 64-word vocabulary WITH A LANGUAGE MODEL at serving size: a 64-word x 5-state model with 8 mixtures and
D = 39, a dense BigramModel over the 64 words (every pair allowed), fp64, and `--streams` (default 4 096) live seven-word
utterances taking `--tick` (default 20) frames per tick -- 0.2 s of audio at 100 frames/s.  More than 16 words under the
bigram grammar: `online_bigram(..., wide=True)` runs on the wide bigram session (gh_online_create_bigram_wide: a wave per
stream, four streams per block around one 32 KB LDS image of the word-to-word costs; 512 N B of state and 256 B of history
per frame and stream).

Three comparisons, each with its legs ALTERNATING in one process on the same frames (host clock around work that ends in
a device synchronise; `--reps` timed rounds after one warm-up round; median with min - max):
  (a) THE DYNAMIC PROGRAM ALONE: the carried wide bigram sweep summed over all ticks (`push_batch(first, count)` on the
      resident whole-utterance batch) against the one-shot wide bigram kernel with labels on the same likelihoods
      (`viterbi_labels`: forward sweep + back-trace), and beside it the carried wide LOOP sweep over the same ticks and
      likelihoods: the difference is what the LDS fill per block and the 64 x 64 min-plus step cost per tick;
  (b) A TICK OF SERVING: `push` per tick (batch creation + upload, likelihoods, carried sweep), over the ticks in which
      every stream still has a whole chunk, against a wide loop session fed the same chunks;
  (c) RE-DECODING THE PREFIX: `push` + `result()` every tick against what a caller had to do without the carried form:
      `decode_batch` on the prefix every tick (upload, likelihoods and decode of everything heard so far).
Everything is reported, nothing is gated.  Kernel times come from a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/time_online_bigram_wide.py --reps 1 --no-prefix
`--states` (default 5) sets the states per word: the register use of the carried sweep, and with it the waves per SIMD, differs
from one word size to the next.
usage: time_online_bigram_wide.py [--streams 4096] [--tick 20] [--reps 7] [--states 5] [--no-prefix]
                                  [--out profiles/online_bigram_wide_4096.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-recognition_amd")):
    sys.path.insert(0, p)
import numpy as np
import bench
import sr.recognition as R
from sr.langmodel import BigramModel
from sr.recognition import _hip
from sr.recognition.batch import ContinuousDecoder

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=4096)
ap.add_argument("--tick", type=int, default=20)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--states", type=int, default=5, help="states per word (2 .. 8)")
ap.add_argument("--no-prefix", action="store_true", help="leave comparison (c) out (profiler runs)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_bigram_wide_4096.json"))
args = ap.parse_args()

K, W, n, M, D = 7, 64, args.states, 8, 39
U, TICK, REPS = args.streams, args.tick, args.reps
ctx = _hip.default_context(0)
wl = bench.synth_workload(1064, 1, W=W, n=n, M=M, D=D)
means, vars_, trans = wl["means"], wl["vars"], wl["trans"]
rng = np.random.default_rng(1064)
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


hmms = [hmm(i) for i in range(W)]
# a language model with every pair allowed (add-one smoothing over random word strings): a dense 64 x 64 cost table
lm = BigramModel(W, smoothing=1.0).fit([list(rng.integers(0, W, size=K)) for _ in range(2000)])
dec = ContinuousDecoder(hmms, grammar="bigram", bigram=lm, ctx=ctx)
dec_l = ContinuousDecoder(hmms, grammar="loop", ctx=ctx)
assert "bigram_wide" in dec.lat.forms() and "loop" in dec_l.lat.forms()
Tmax = int(T.max())
n_ticks = int(-(-Tmax // TICK))
full_ticks = int(T.min() // TICK)                       # ticks in which every stream still has a whole chunk
ids = np.arange(U)
chunks = [[x[k * TICK:(k + 1) * TICK] for x in xs] for k in range(n_ticks)]


def clock(fn):
    ctx.sync()
    t0 = time.perf_counter()
    r = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, r


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(ms_median=float(np.median(v)), ms_min=float(v.min()), ms_max=float(v.max()), ms=[float(x) for x in v])


def labels_of(r):
    return [r["labels_flat"][r["label_off"][u]:r["label_off"][u] + r["n_labels"][u]].tolist() for u in range(U)]


# ---- (a) the dynamic program alone, on one resident likelihood matrix ----
whole = _hip.Batch(ctx, feats=X, offsets=off)
whole.loglik(dec.gmm, fetch=False)
ml = whole.lengths // (n - 1) + 2
row_word = np.where(dec.row_state >= 0, dec.row_state // n, -1).astype(np.int32)
a = dict(carried_bigram_wide_all_ticks=[], one_shot_bigram_wide_labels=[], carried_loop_wide_all_ticks=[])
on_a = dec.online_bigram(U, Tmax, wide=True)
on_l = dec_l.online(U, Tmax)
assert isinstance(on_a.session, _hip.OnlineBigramWideSession) and isinstance(on_l.session, _hip.OnlineWideSession)
firsts = [np.minimum(k * TICK, T) for k in range(n_ticks)]
one = None
for rep in range(REPS + 1):                             # round 0 warms up (code objects, scratch arenas)
    on_a.reset()
    on_l.reset()

    def sweep(on):
        for first in firsts:
            on.push_batch(ids, whole, first=first, count=np.minimum(TICK, T - first))
    ms_on, _ = clock(lambda: sweep(on_a))
    ms_one, one = clock(lambda: dec.lat.viterbi_labels(whole, row_word, max_labels=ml, as_lists=False, want_end_cost=False))
    ms_loop, _ = clock(lambda: sweep(on_l))
    if rep:
        a["carried_bigram_wide_all_ticks"].append(ms_on)
        a["one_shot_bigram_wide_labels"].append(ms_one)
        a["carried_loop_wide_all_ticks"].append(ms_loop)
wa, ra = on_a.result()
same = bool(wa == labels_of(one) and np.array_equal(ra["best_end"], one["best_end"]))
accuracy = float(np.mean([wa[u] == list(words[u]) for u in range(U)]))
on_a.close()
on_l.close()
whole.close()

print("(a) done", file=sys.stderr, flush=True)

# ---- (b) a tick of serving ----
b = dict(bigram_wide_push_per_tick=[], loop_wide_push_per_tick=[])
on_b = dec.online_bigram(U, Tmax, wide=True)
on_bl = dec_l.online(U, Tmax)
for rep in range(REPS + 1):
    on_b.reset()
    on_bl.reset()
    per, per_l = [], []
    for k in range(n_ticks):
        per.append(clock(lambda: on_b.push(ids, chunks[k]))[0])
        per_l.append(clock(lambda: on_bl.push(ids, chunks[k]))[0])
    if rep:
        b["bigram_wide_push_per_tick"].append(float(np.median(per[:full_ticks])))
        b["loop_wide_push_per_tick"].append(float(np.median(per_l[:full_ticks])))
same = same and on_b.result()[0] == wa
on_bl.close()

print("(b) done", file=sys.stderr, flush=True)

# ---- (c) push + result every tick against re-decoding the prefix every tick ----
c = None
if not args.no_prefix:
    c = dict(online_push_and_result_all_ticks=[], prefix_decode_all_ticks=[], online_last_tick=[], prefix_last_tick=[])
    for rep in range(REPS + 1):
        on_b.reset()
        tot = last = 0.0
        for k in range(n_ticks):
            last = clock(lambda: on_b.push(ids, chunks[k]))[0] + clock(lambda: on_b.result())[0]
            tot += last
        got_on = on_b.result()[0]
        ptot = plast = 0.0
        for k in range(n_ticks):
            pre = [x[:(k + 1) * TICK] for x in xs]

            def redo():
                bt = _hip.Batch(ctx, pre, dtype=dec.dtype)
                try:
                    return dec.decode_batch(bt)[0]
                finally:
                    bt.close()
            plast, got = clock(redo)
            ptot += plast
        same = same and got == got_on == wa
        print("(c) round %d of %d" % (rep, REPS), file=sys.stderr, flush=True)
        if rep:
            c["online_push_and_result_all_ticks"].append(tot)
            c["prefix_decode_all_ticks"].append(ptot)
            c["online_last_tick"].append(last)
            c["prefix_last_tick"].append(plast)
on_b.close()

tick_s = TICK / 100.0
out = dict(shape=dict(W=W, n=n, M=M, D=D, streams=int(U), tick_frames=TICK, ticks=n_ticks, full_ticks=full_ticks, frames=int(off[-1]),
                      state_bytes_per_stream=512 * n, history_bytes_per_stream=256 * Tmax, cost_image_bytes_per_block=32768,
                      streams_per_block=4),
           reps=REPS, online_equals_one_shot=same, sentence_accuracy=accuracy,
           a_dynamic_program={k: stats(v) for k, v in a.items()}, b_push_per_tick={k: stats(v) for k, v in b.items()})
A, B = out["a_dynamic_program"], out["b_push_per_tick"]
A["carried_over_one_shot_bigram_wide"] = A["carried_bigram_wide_all_ticks"]["ms_median"] / A["one_shot_bigram_wide_labels"]["ms_median"]
A["carried_bigram_over_carried_loop"] = A["carried_bigram_wide_all_ticks"]["ms_median"] / A["carried_loop_wide_all_ticks"]["ms_median"]
A["bigram_minus_loop_ms_per_tick"] = (A["carried_bigram_wide_all_ticks"]["ms_median"] - A["carried_loop_wide_all_ticks"]["ms_median"]) / n_ticks
B["realtime_streams_per_gpu_push_only"] = U * tick_s * 1e3 / B["bigram_wide_push_per_tick"]["ms_median"]
if c is not None:
    out["c_prefix"] = {k: stats(v) for k, v in c.items()}
    C = out["c_prefix"]
    C["prefix_over_online"] = C["prefix_decode_all_ticks"]["ms_median"] / C["online_push_and_result_all_ticks"]["ms_median"]
    C["last_tick_prefix_over_online"] = C["prefix_last_tick"]["ms_median"] / C["online_last_tick"]["ms_median"]
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
