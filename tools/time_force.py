#!/usr/bin/env python3
"""The forced commit (`online(..., max_tail=)`, gh_online_force) at serving size: the configs[4] model (10 words x 5 states,
8 mixtures, D = 39, fp64) and `--streams` (default 4 096) live seven-word utterances taking `--tick` (default 20) frames
per tick, as tools/time_settle.py.

Host clock around a `commit` call that ends in a device synchronise; a PASS is all ticks of the utterances, its figure the
median over the ticks in which every stream still has frames; the two decoders of a leg run their passes ALTERNATING in one
process, `--passes` (default 7) each after one warm-up pass each, and a leg reports the median of its passes with min and max.
  (a) nothing is forced: a window= decoder with `max_tail` = the longest natural tail against the same decoder without
      `max_tail`.  Expected: inside the other's min .. max -- the added work is one host comparison per commit.
  (b) streams are forced every tick: the same model with word_penalty = 50 and `max_tail` = 5, below the natural tails of
      this model (its traces do meet, 15 - 20 frames back), full history on both sides, against none.  The JSON holds the
      number of streams per tick whose commit pruned cells.
Derivable beforehand for (b): a forced stream reads its unsettled decision words twice more than a commit does, once down
and once up (16 B per 4 columns and lane at N = 5), and writes at most 16 N doubles.  No pass mark.
usage: time_force.py [--streams 4096] [--tick 20] [--passes 7] [--out result.json]"""
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
ap.add_argument("--passes", type=int, default=7)
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


hmms = [hmm(i) for i in range(W)]
n_ticks = int(-(-T.max() // TICK))
full_ticks = int(T.min() // TICK)
ids = np.arange(U)
chunks = [[x[k * TICK:(k + 1) * TICK] for x in xs] for k in range(n_ticks)]


def one_pass(on):
    """(median commit ms over the full ticks, median push ms, largest tail after a commit, streams forced per full tick)."""
    on.reset()
    commit_ms, push_ms, worst, forced = [], [], 0, []
    for k in range(n_ticks):
        ctx.sync()
        t0 = time.perf_counter()
        on.push(ids, chunks[k])
        ctx.sync()
        t1 = time.perf_counter()
        before = on.n_forced.copy()
        on.commit(ids)
        ctx.sync()
        t2 = time.perf_counter()
        push_ms.append((t1 - t0) * 1e3)
        commit_ms.append((t2 - t1) * 1e3)
        forced.append(int((on.n_forced - before).sum()))
        worst = max(worst, int((on.frames - on.settled()[1]).max()))
    return float(np.median(commit_ms[:full_ticks])), float(np.median(push_ms[:full_ticks])), worst, forced[:full_ticks]


def leg(plain, forcing):
    """Alternating passes of the two decoders; per decoder the median of its passes with min and max."""
    for on in (plain, forcing):
        one_pass(on)                                        # warm-up
    rows = {"without_max_tail": [], "with_max_tail": []}
    for _ in range(args.passes):
        rows["without_max_tail"].append(one_pass(plain))
        rows["with_max_tail"].append(one_pass(forcing))
    out = {}
    for key, r in rows.items():
        c = [x[0] for x in r]
        out[key] = dict(commit_ms=dict(median=float(np.median(c)), min=min(c), max=max(c)), push_ms_median=float(np.median([x[1] for x in r])),
                        largest_tail_after_a_commit=max(x[2] for x in r), streams_forced_per_full_tick=r[-1][3])
    return out


# ---- (a) nothing is forced
dec = ContinuousDecoder(hmms, grammar="loop", ctx=ctx)
probe = dec.online(U, max_frames=int(T.max()))
worst = one_pass(probe)[2]
words_ref = probe.result()[0]
probe.close()
window = worst + TICK
plain, forcing = dec.online(U, window=window), dec.online(U, window=window, max_tail=worst)
leg_a = leg(plain, forcing)
same_a = bool(plain.result()[0] == forcing.result()[0] == words_ref) and not forcing.n_forced.any()
plain.close(); forcing.close()

# ---- (b) every stream is forced every tick
stuck = ContinuousDecoder(hmms, grammar="loop", word_penalty=50.0, ctx=ctx)
M_TAIL = 5
plain, forcing = stuck.online(U, max_frames=int(T.max())), stuck.online(U, max_frames=int(T.max()), max_tail=M_TAIL)
leg_b = leg(plain, forcing)
settled_b = forcing.settled()
prefix_b = bool(all(s == f[:len(s)] for s, f in zip(settled_b[0], forcing.result()[0])))
plain.close(); forcing.close()

out = dict(shape=dict(W=W, n=n, M=M, D=D, streams=int(U), tick_frames=TICK, ticks=n_ticks, full_ticks=full_ticks, passes=args.passes),
           a_nothing_forced=dict(window=window, max_tail=worst, results_equal_and_nothing_forced=same_a, **leg_a),
           b_every_stream_forced=dict(word_penalty=50.0, max_tail=M_TAIL, settled_words_are_a_prefix_of_the_result=prefix_b,
                                      derived_extra_bytes_read_per_forced_stream=2 * 64 * (-(-M_TAIL // (32 // (n + 2))) + 1),
                                      derived_bytes_written_per_forced_stream_at_most=16 * n * 8, **leg_b))
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
