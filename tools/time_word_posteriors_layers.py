#!/usr/bin/env python3
"""What word posteriors and confidences cost on the K-layer lattice at serving size: the configs[4] model (10 words x 5
states, 8 mixtures, D = 39, fp64), K = 7 layers, and `--streams` (default 4 096) seven-word utterances as one resident batch,
the workload of tools/time_word_posteriors.py.  Likelihoods are computed before the clock starts.  The legs ALTERNATE inside
one process, `--reps` (default 7) rounds after two warm-up rounds; every figure is the median with min - max:

  (a)  decode_batch(want_times=True)                                  host clock, ends in a device synchronise
  (b)  decode_batch(want_confidence=True, layers=True)                the same decode + one gh_word_posteriors_layers call
  (c)  lat.forward_backward(b, want_occ=True, fetch_occ=False)        the generic row-per-lane kernel on the same batch: the
                                                                      kernel-level yardstick
  (c') lat.forward_backward(sub, want_matrices=True)                  what a caller had to do before: three [R, T] matrices
                                                                      per utterance to the host, on a sub-batch of `--sub`
                                                                      (default 64) utterances that fits; also scaled to the
                                                                      whole batch by frames (labelled as scaled)
  (d)  gh_word_posteriors_layers alone, by HIP events on the context's stream (everything the call enqueues: the span table
       up, the sweep, the results back), with the [N, W] posteriorgram copied out and without it

Derived, not measured: per frame the sweep stores and reloads 8 K N W B of alpha, reads 8 S B of emissions twice and writes
8 W B of posteriors -- 6.5 KB at 7 x 5 x 10.  Expectation, not a gate: (d) without the posteriorgram does a full
forward-backward like (c), so its median should not lie above (c)'s min - max.
The result goes to --out, by default profiles/word_posteriors_layers_<streams>.json.
usage: time_word_posteriors_layers.py [--streams 4096] [--reps 7] [--sub 64] [--out profiles/word_posteriors_layers_4096.json]"""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sub", type=int, default=64)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "word_posteriors_layers_%d.json" % args.streams)

K, W, n, M, D = 7, 10, 5, 8, 39
U = args.streams
SUB = min(args.sub, U)
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


def hmm(i):
    h = R.HMM(n)
    h.gmm_states = []
    for s in range(n):
        g = R.GMM(means[i, s, 0].copy(), vars_[i, s, 0].copy(), M)
        g.update_models(means[i, s].copy(), vars_[i, s].copy(), wl["w"][i, s].copy())
        h.gmm_states.append(g)
    h.transitions = trans.copy()
    return h


dec = ContinuousDecoder([hmm(i) for i in range(W)], n_layers=K, grammar="layers", ctx=ctx)
batch = _hip.Batch(ctx, feats=X, offsets=off)
batch.loglik(dec.gmm, fetch=False)
sub = _hip.Batch(ctx, feats=X[:off[SUB]], offsets=off[:SUB + 1])
sub.loglik(dec.gmm, fetch=False)
_, timed = dec.decode_batch(batch, want_times=True)
labels, begins = timed["labels"], timed["begins"]
e0, e1 = ctx.new_event(), ctx.new_event()


def host_clock(fn):
    ctx.sync()
    t0 = time.perf_counter()
    r = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, r


def by_events(fn):
    ctx.sync()
    ctx.record(e0)
    r = fn()
    ctx.record(e1)
    return ctx.elapsed_ms(e0, e1), r


def matrices_small():
    r = dec.lat.forward_backward(sub, want_matrices=True)
    return dict(logp=r["logp"])                                            # (the matrices are not kept between the rounds)


legs = [("a_decode_with_times", host_clock, lambda: dec.decode_batch(batch, want_times=True)),
        ("b_decode_with_confidence", host_clock, lambda: dec.decode_batch(batch, want_confidence=True, layers=True)),
        ("c_generic_forward_backward_occ", host_clock, lambda: dec.lat.forward_backward(batch, want_occ=True, fetch_occ=False)),
        ("c2_generic_matrices_sub_batch", host_clock, matrices_small),
        ("d_word_posteriors_with_post", by_events, lambda: dec.lat.word_posteriors_layers(batch, labels=labels, begins=begins)),
        ("d_word_posteriors_without_post", by_events,
         lambda: dec.lat.word_posteriors_layers(batch, labels=labels, begins=begins, want_post=False))]
ms = {name: [] for name, _, _ in legs}
last = {}
chunks = {}
for rep in range(args.reps + 2):
    for name, clock, fn in legs:
        m, last[name] = clock(fn)
        chunks[name] = ctx.last_chunks
        if rep >= 2:
            ms[name].append(m)
stat = lambda v: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), reps=len(v))
res = {name: dict(stat(v), launches=int(chunks[name])) for name, v in ms.items()}
full, lean = last["d_word_posteriors_with_post"], last["d_word_posteriors_without_post"]
conf_b = last["b_decode_with_confidence"][1]["confidence"]
post = full["post"]
live = np.isfinite(np.repeat(full["logp"], np.diff(off)))
checks = dict(words_equal=bool(last["b_decode_with_confidence"][0] == last["a_decode_with_times"][0]),
              confidences_equal=bool(all(np.array_equal(a, b) and np.array_equal(a, c)
                                         for a, b, c in zip(full["confidence"], lean["confidence"], conf_b))),
              logp_equal_generic=bool(np.allclose(full["logp"], last["c_generic_forward_backward_occ"]["logp"], rtol=1e-10, atol=0)),
              logp_equal_generic_sub_batch=bool(np.allclose(full["logp"][:SUB], last["c2_generic_matrices_sub_batch"]["logp"],
                                                            rtol=1e-10, atol=0)),
              rows_sum_to_one=float(np.max(np.abs(post[live].sum(axis=1) - 1.0))) if live.any() else None,
              mean_confidence=float(np.mean(np.concatenate(full["confidence"]))))
c, d = res["c_generic_forward_backward_occ"], res["d_word_posteriors_without_post"]
frames, sub_frames = int(off[-1]), int(off[SUB])
res["c2_generic_matrices_sub_batch"].update(utterances=int(SUB), frames=sub_frames,
                                            scaled_to_the_batch_by_frames_ms=res["c2_generic_matrices_sub_batch"]["median_ms"] * frames / sub_frames)
per_frame = 8 * K * n * W * 2 + 2 * 8 * W * n + 8 * W
out = dict(shape=dict(K=K, W=W, n=n, M=M, D=D, rows=1 + K * (W * n + 1), streams=int(U), frames=frames,
                      words=int(sum(len(l) for l in labels)), derived_bytes_per_frame=per_frame,
                      derived_gbytes=per_frame * frames / 1e9),
           checks=checks, ms=res, d_without_post_within_c_spread=bool(d["median_ms"] <= c["max_ms"]))
print(json.dumps(out))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f)
    f.write("\n")
sub.close()
batch.close()
