#!/usr/bin/env python3
"""The settled prefix of a BIGRAM session at serving size: the configs[4] model (10 words x 5 states, 8 mixtures, D = 39,
fp64), the bigram model of tools/time_online_bigram.py (every pair allowed) and `--streams` (default 4 096) live seven-word
utterances taking `--tick` (default 20) frames per tick, as tools/time_settle.py.

  * `commit` per tick (the settle walk, the segment walk and the copy-back of the new words of all streams) on a bigram
    session that settles BESIDE a loop session of the same shape, in one process on the same frames, the two legs
    alternating: `--reps` (default 7) timed rounds after one warm-up round, each round's figure the median over the ticks
    in which every stream still has a whole chunk; median with min - max over the rounds.  The push in front of every
    commit is reported the same way.  Host clock around work that ends in a device synchronise.
  * the distribution of the UNSETTLED TAIL in frames (frames - settled_frames after each commit, all streams, every tick
    from the first in which the stream has an anchor) of both sessions: median, p99, max;
  * device bytes per stream of a bigram session with window = 2 x that p99 against one with max_frames = a 60 s utterance
    (6 000 frames), from the layout in include/gmmhmm.h: 128 N B of carried column, 64 B of open word, 16 B of anchor and
    64 B per record word (3 columns at N = 5 without skip arcs; the loop form: 4);
  * a pass through an `online_bigram(window=)` decoder of that size (or of the longest tail + one tick, if that is more:
    there is no forced commit): the same words.
Derivable beforehand: a commit reads one 64 B record row per 3 unsettled frames of a stream and the stream's 640 B column.
Everything is reported, nothing is gated.
usage: time_bigram_settle.py [--streams 4096] [--tick 20] [--reps 7] [--out profiles/online_bigram_settle_4096.json]"""
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
ap.add_argument("--out", default=None)
args = ap.parse_args()

K, W, n, M, D = 7, 10, 5, 8, 39
U, TICK, REPS = args.streams, args.tick, args.reps
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


hmms = [hmm(i) for i in range(W)]
lm = BigramModel(W, smoothing=1.0).fit([list(np.random.default_rng(7).integers(0, W, size=7)) for _ in range(500)])
dec_b = ContinuousDecoder(hmms, grammar="bigram", bigram=lm, ctx=ctx)
dec_l = ContinuousDecoder(hmms, grammar="loop", ctx=ctx)
assert "bigram" in dec_b.lat.forms() and "loop" in dec_l.lat.forms()
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


def serve(on):
    """One round of push + commit per tick: (push ms, commit ms) per tick, the unsettled tails, the largest of them."""
    on.reset()
    push, commit, tails, worst = [], [], [], 0
    for k in range(n_ticks):
        push.append(clock(lambda: on.push(ids, chunks[k]))[0])
        commit.append(clock(lambda: on.commit(ids))[0])
        settled = on.settled()[1]
        has = settled > 0
        tails.append((on.frames - settled)[has])
        worst = max(worst, int((on.frames - settled).max()))           # (streams without an anchor yet among them)
    return push, commit, np.concatenate(tails), worst


legs = dict(bigram=dec_b.online_bigram(U, max_frames=Tmax, settle=True), loop=dec_l.online(U, max_frames=Tmax))
per = {name: dict(push=[], commit=[]) for name in legs}
tails, worst = {}, {}
for rep in range(REPS + 1):                             # round 0 warms up (code objects, scratch arenas)
    for name, on in legs.items():
        push, commit, tails[name], worst[name] = serve(on)
        if rep:
            per[name]["push"].append(float(np.median(push[:full_ticks])))
            per[name]["commit"].append(float(np.median(commit[:full_ticks])))
    print("round %d of %d" % (rep, REPS), file=sys.stderr, flush=True)
final = {name: on.result()[0] for name, on in legs.items()}
settled_words = {name: on.settled()[0] for name, on in legs.items()}
for on in legs.values():
    on.close()
batch = _hip.Batch(ctx, feats=X, offsets=off)
one_shot = dict(bigram=dec_b.decode_batch(batch)[0], loop=dec_l.decode_batch(batch)[0])
batch.close()


def tail_stats(v):
    p50, p99, tmax = (int(np.percentile(v, q)) for q in (50, 99, 100))
    return dict(median=p50, p99=p99, max=tmax, samples=int(len(v)))


tail_b = tail_stats(tails["bigram"])
window = 2 * tail_b["p99"]
cpw_b, cpw_l = 32 // (n + 5), 32 // (n + 2)


def bytes_per_stream(words_of_history):
    return 128 * n + 64 + 16 + 64 * words_of_history


window_run = max(window, worst["bigram"] + TICK)        # (there is no forced commit: the pass must hold the longest tail + a tick)
win = dec_b.online_bigram(U, window=window_run)
serve(win)
final_w = win.result()[0]
win.close()
ok = bool(all(final[k] == one_shot[k] for k in final) and final_w == one_shot["bigram"] and
          all(s == f[:len(s)] for k in final for s, f in zip(settled_words[k], final[k])))
out = dict(shape=dict(W=W, n=n, M=M, D=D, streams=int(U), tick_frames=TICK, ticks=n_ticks, full_ticks=full_ticks, frames=int(off[-1])),
           reps=REPS, results_equal=ok,
           commit_per_tick={k: stats(v["commit"]) for k, v in per.items()}, push_per_tick={k: stats(v["push"]) for k, v in per.items()},
           unsettled_tail_frames=dict(bigram=tail_b, loop=tail_stats(tails["loop"]),
                                      bigram_max_before_the_first_anchor_too=worst["bigram"]),
           settled_words_at_the_end={k: float(np.mean([len(s) for s in v])) for k, v in settled_words.items()},
           commit_reads_bytes_per_stream=dict(median=64 * -(-tail_b["median"] // cpw_b) + 128 * n, p99=64 * -(-tail_b["p99"] // cpw_b) + 128 * n),
           device_bytes_per_stream=dict(window_frames=window, window_frames_of_the_windowed_pass=window_run,
                                        bigram_windowed=bytes_per_stream(-(-window // cpw_b) + 1),
                                        bigram_max_frames_60s=bytes_per_stream(-(-6000 // cpw_b)),
                                        loop_windowed_same_window=bytes_per_stream(-(-window // cpw_l) + 1)))
C = out["commit_per_tick"]
C["bigram_over_loop"] = C["bigram"]["ms_median"] / C["loop"]["ms_median"]
C["bigram_commit_over_bigram_push"] = C["bigram"]["ms_median"] / out["push_per_tick"]["bigram"]["ms_median"]
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
