#!/usr/bin/env python3
"""The settled prefix of a WIDE BIGRAM online decode at serving size: the model of tools/time_online_bigram_wide.py (64 words x
5 states, 8 mixtures, D = 39, a dense BigramModel over the 64 words, fp64) and `--streams` (default 4 096) live seven-word
utterances taking `--tick` (default 20) frames per tick, through `online_bigram(..., wide="settle")`
(gh_online_create_bigram_wide_settle: the settle walk over 64 word lanes with the hop through the word a record names).

Three legs ALTERNATING in one process on the same frames (host clock around work that ends in a device synchronise; `--reps`
timed rounds after one warm-up round; a round's figure is the median over the ticks in which every stream still has a whole
chunk; reported: the median of the rounds with min - max):
  * the wide bigram session that settles, full history (`max_frames=, settle=True`): the `push` call and the `commit` call
    behind it -- the settle walk, the segment walk and the copy-back of the new words of all streams;
  * the wide LOOP session that settles (`online(..., settle=True)` on the same word models), the same two calls: the figure
    to hold the first beside.  The expectation, not a gate: a commit costs about the same in both;
  * the wide bigram session with a window (`window=`): the same two calls through the ring of columns, and the same words.
From the warm-up round of the first leg, before the third is made:
  * the distribution of the UNSETTLED TAIL in frames (frames - settled_frames after each commit, all streams, every tick
    from the first in which the stream has an anchor): median, p99, max;
  * device bytes per stream of a session with window = 2 x that p99 against one with max_frames = a 60 s utterance
    (6 000 frames), from the layout in include/gmmhmm.h: 512 N B of carried column, 16 B of anchor and 256 B per column
    (window + 1 columns in the ring).  The windowed leg runs at that window, or at the longest tail + one tick if that is
    more: there is no forced commit.
Derivable beforehand: a commit reads 256 B per unsettled column and stream, and the stream's 512 N B column.  No pass mark.
usage: time_bigram_wide_settle.py [--streams 4096] [--tick 20] [--reps 7] [--out profiles/online_bigram_wide_settle_4096.json]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_bigram_wide_settle_4096.json"))
args = ap.parse_args()

K, W, n, M, D = 7, 64, 5, 8, 39
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
full_ticks = int(T.min() // TICK)
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
    """One round of push + commit per tick: per-tick rows, the unsettled tails, the longest tail, the final words."""
    on.reset()
    rows, tails, worst = [], [], 0
    for k in range(n_ticks):
        ms_push, _ = clock(lambda: on.push(ids, chunks[k]))
        ms_commit, new = clock(lambda: on.commit(ids))
        settled = on.settled()[1]
        has = settled > 0
        tails.append((on.frames - settled)[has])
        worst = max(worst, int((on.frames - settled).max()))              # (streams without an anchor yet among them)
        rows.append(dict(tick=k, push_ms=ms_push, commit_ms=ms_commit, streams_with_anchor=int(has.sum()),
                         new_words=int(sum(len(w) for w in new))))
    return rows, np.concatenate(tails), worst, on.result()[0]


med = lambda rows, key: float(np.median([r[key] for r in rows[:full_ticks]]))
full = dec.online_bigram(U, max_frames=Tmax, settle=True, wide="settle")
assert isinstance(full.session, _hip.OnlineBigramWideSession) and full.session.settles
rows, tails, worst, final = serve(full)                 # round 0 of the first leg: warms up, and says how long the tails are
settled_words = full.settled()[0]
p50, p99, tmax = (int(np.percentile(tails, q)) for q in (50, 99, 100))
loop = dec_l.online(U, max_frames=Tmax, settle=True)
assert isinstance(loop.session, _hip.OnlineWideSession) and loop.session.settles
rows_l, tails_l, _, final_l = serve(loop)               # round 0 of the second leg
window = 2 * p99
window_run = max(window, worst + TICK)                  # (there is no forced commit: the ring must hold the longest tail + a tick)
win = dec.online_bigram(U, window=window_run, wide="settle")
rows_w, _, _, final_w = serve(win)                      # round 0 of the third leg
legs = dict(push_call=[], commit_call=[], loop_push_call=[], loop_commit_call=[], windowed_push_call=[], windowed_commit_call=[])
same = True
for rep in range(REPS):
    rows, _, _, f1 = serve(full)
    rows_l, _, _, f2 = serve(loop)
    rows_w, _, _, f3 = serve(win)
    same = same and f1 == final and f2 == final_l and f3 == final
    for name, rr in (("", rows), ("loop_", rows_l), ("windowed_", rows_w)):
        legs[name + "push_call"].append(med(rr, "push_ms"))
        legs[name + "commit_call"].append(med(rr, "commit_ms"))
    print("round %d of %d" % (rep + 1, REPS), file=sys.stderr, flush=True)
for on in (full, loop, win):
    on.close()
batch = _hip.Batch(ctx, feats=X, offsets=off)
one_shot = dec.decode_batch(batch)[0]
one_shot_l = dec_l.decode_batch(batch)[0]
batch.close()


def bytes_per_stream(columns):
    return 512 * n + 16 + 256 * columns


per_tick = {k: stats(v) for k, v in legs.items()}
pl = [int(np.percentile(tails_l, q)) for q in (50, 99, 100)]
out = dict(shape=dict(W=W, n=n, M=M, D=D, streams=int(U), tick_frames=TICK, ticks=n_ticks, full_ticks=full_ticks, frames=int(off[-1])),
           reps=REPS,
           results_equal=bool(same and final == one_shot == final_w and final_l == one_shot_l and
                              all(s == f[:len(s)] for s, f in zip(settled_words, final))),
           per_tick_ms=per_tick,
           commit_over_push=per_tick["commit_call"]["ms_median"] / per_tick["push_call"]["ms_median"],
           commit_over_loop_commit=per_tick["commit_call"]["ms_median"] / per_tick["loop_commit_call"]["ms_median"],
           push_over_loop_push=per_tick["push_call"]["ms_median"] / per_tick["loop_push_call"]["ms_median"],
           windowed_commit_over_push=per_tick["windowed_commit_call"]["ms_median"] / per_tick["windowed_push_call"]["ms_median"],
           unsettled_tail_frames=dict(median=p50, p99=p99, max=tmax, max_before_the_first_anchor_too=worst, samples=int(len(tails))),
           unsettled_tail_frames_loop=dict(median=pl[0], p99=pl[1], max=pl[2], samples=int(len(tails_l))),
           settled_words_at_the_end=float(np.mean([len(s) for s in settled_words])),
           commit_reads_bytes_per_stream=dict(median=256 * p50 + 512 * n, p99=256 * p99 + 512 * n),
           device_bytes_per_stream=dict(window_frames=window, window_frames_of_the_third_leg=window_run, windowed=bytes_per_stream(window + 1),
                                        max_frames_60s=bytes_per_stream(6000)),
           ticks=rows, ticks_loop=rows_l, ticks_windowed=rows_w)
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
