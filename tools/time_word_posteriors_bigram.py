#!/usr/bin/env python3
"""What word posteriors and confidences cost under a bigram grammar at serving size, at two sizes: the configs[4] model
(10 words x 5 states, 8 mixtures, D = 39, fp64; the workload of tools/time_word_posteriors.py) under a dense `BigramModel`,
and the 64-word model of tools/time_bigram_wide.py.  `--streams` (default 4 096) seven-word utterances as one resident
batch, likelihoods computed before the clock starts.  The legs ALTERNATE inside one process, `--reps` (default 7) rounds
after two warm-up rounds; every figure is the median with min - max:

  (a) decode_batch(want_times=True)                                   host clock, ends in a device synchronise
  (b) decode_batch(want_confidence=True, lm=True)                     the same decode + one gh_word_posteriors_bigram call
  (c) lat.forward_backward(b, want_matrices=True)                     what a caller has to do today (three [R, T] matrices
      per utterance to the host; the boundary correction on the host is NOT in the figure): the yardstick.  On the first
      `--generic-streams` utterances only (default 512 at 10 words, 128 at 64: the matrices of the whole batch are 2 GB and
      12 GB); its figure is also given scaled to the whole batch by frames, and marked as scaled
  (d) gh_word_posteriors_bigram alone, by HIP events on the context's stream (everything the call enqueues), with the
      [N, W] posteriorgram copied out and without it (log P and confidences only)
  (e) gh_word_posteriors of a loop decoder on the same likelihoods and the same span table: the floor, the same sweep
      without the W x W steps

Expectation, not a gate: (d) without out_post lies below (c)'s minimum scaled to the whole batch.
The results go to --out, by default profiles/word_posteriors_bigram_<streams>.json: {"10x5": ..., "64x5": ...}.
usage: time_word_posteriors_bigram.py [--streams 4096] [--reps 7] [--sizes 10x5,64x5] [--out FILE]"""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sizes", default="10x5,64x5")
ap.add_argument("--generic-streams", type=int, default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(ROOT, "profiles", "word_posteriors_bigram_%d.json" % args.streams)
ctx = _hip.default_context(0)
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


def run(W, n, seed, lm_seed, n_generic):
    K, M, D, U = 7, 8, 39, args.streams
    wl = bench.synth_workload(seed, 1, W=W, n=n, M=M, D=D)
    means, vars_, trans = wl["means"], wl["vars"], wl["trans"]
    rng = np.random.default_rng(seed)
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

    hmms = [hmm(i) for i in range(W)]
    # a language model with every pair allowed (add-one smoothing over random word strings): a dense W x W cost table
    lm_rng = np.random.default_rng(lm_seed)
    lm = BigramModel(W, smoothing=1.0).fit([list(lm_rng.integers(0, W, size=K)) for _ in range(2000)])
    dec = ContinuousDecoder(hmms, grammar="bigram", bigram=lm, ctx=ctx)
    loop = ContinuousDecoder(hmms, grammar="loop", ctx=ctx)
    batch = _hip.Batch(ctx, feats=X, offsets=off)
    batch.loglik(dec.gmm, fetch=False)
    ng = min(U, n_generic)
    sub = _hip.Batch(ctx, feats=X[:off[ng]], offsets=off[:ng + 1])
    sub.loglik(dec.gmm, fetch=False)
    _, timed = dec.decode_batch(batch, want_times=True)
    labels, begins = timed["labels"], timed["begins"]
    legs = [("a_decode_with_times", host_clock, lambda: dec.decode_batch(batch, want_times=True)),
            ("b_decode_with_confidence_lm", host_clock, lambda: dec.decode_batch(batch, want_confidence=True, lm=True)),
            ("c_generic_forward_backward_matrices_sub", host_clock, lambda: dec.lat.forward_backward(sub, want_matrices=True)["logp"]),
            ("d_word_posteriors_bigram_with_post", by_events, lambda: dec.lat.word_posteriors_bigram(batch, labels=labels, begins=begins)),
            ("d_word_posteriors_bigram_without_post", by_events,
             lambda: dec.lat.word_posteriors_bigram(batch, labels=labels, begins=begins, want_post=False)),
            ("e_loop_word_posteriors_without_post", by_events,
             lambda: loop.lat.word_posteriors(batch, labels=labels, begins=begins, want_post=False))]
    ms = {name: [] for name, _, _ in legs}
    last, chunks = {}, {}
    for rep in range(args.reps + 2):
        for name, clock, fn in legs:
            m, last[name] = clock(fn)
            chunks[name] = ctx.last_chunks
            if rep >= 2:
                ms[name].append(m)
    stat = lambda v: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), reps=len(v))
    res = {name: dict(stat(v), launches=int(chunks[name])) for name, v in ms.items()}
    frames, sub_frames = int(off[-1]), int(off[ng])
    scale = frames / sub_frames
    c = res["c_generic_forward_backward_matrices_sub"]
    res["c_scaled_to_the_whole_batch"] = dict(median_ms=c["median_ms"] * scale, min_ms=c["min_ms"] * scale, max_ms=c["max_ms"] * scale,
                                              scaled_by_frames=scale, streams=int(ng), frames=sub_frames)
    full, lean = last["d_word_posteriors_bigram_with_post"], last["d_word_posteriors_bigram_without_post"]
    conf_b = last["b_decode_with_confidence_lm"][1]["confidence"]
    post = full["post"]
    live = np.isfinite(np.repeat(full["logp"], np.diff(off)))
    checks = dict(words_equal=bool(last["b_decode_with_confidence_lm"][0] == last["a_decode_with_times"][0]),
                  confidences_equal=bool(all(np.array_equal(a, b) and np.array_equal(a, c_)
                                             for a, b, c_ in zip(full["confidence"], lean["confidence"], conf_b))),
                  logp_equal_generic=bool(np.allclose(full["logp"][:ng], last["c_generic_forward_backward_matrices_sub"], rtol=1e-10, atol=0)),
                  rows_sum_to_one=float(np.max(np.abs(post[live].sum(axis=1) - 1.0))) if live.any() else None,
                  mean_confidence=float(np.mean(np.concatenate(full["confidence"]))),
                  word_accuracy=float(np.mean([list(l) == list(w) for l, w in zip(last["a_decode_with_times"][0], words)])))
    d = res["d_word_posteriors_bigram_without_post"]
    out = dict(shape=dict(W=W, n=n, M=M, D=D, streams=int(U), frames=frames, words=int(sum(len(l) for l in labels)),
                          forms=sorted(dec.lat.forms())),
               checks=checks, ms=res, d_without_post_below_c_min=bool(d["median_ms"] < res["c_scaled_to_the_whole_batch"]["min_ms"]))
    batch.close()
    sub.close()
    return out


SIZES = {"10x5": (10, 5, 1005, 5, 512), "64x5": (64, 5, 1064, 64, 128)}
out = {}
for name in args.sizes.split(","):
    W, n, seed, lm_seed, ng = SIZES[name]
    out[name] = run(W, n, seed, lm_seed, args.generic_streams or ng)
    print(json.dumps({name: out[name]}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f)
    f.write("\n")
