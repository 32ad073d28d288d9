#!/usr/bin/env python3
"""Online isolated-word recognition at serving size: the configs[1] model (10 words x 5 states, 8 mixtures, D = 39, fp64)
and `--streams` (default 4 096) live utterances taking `--tick` (default 20) frames per tick -- 0.2 s of audio at 100
frames/s -- for `--ticks` (default 100) ticks.

Per tick, medians over the ticks after the first (which warms up):
  * the whole `OnlineWordRecognizer.push` call: host clock around work that ends in a device synchronise;
  * its parts as DEVICE times from HIP events on the context's stream: batch creation + upload, likelihoods, the carried
    sweep (the events bracket what each step enqueues; the host time of a step is listed beside it);
  * `result()` of all streams;
  * what a caller has to do without the online form: `recognize` on the prefix, at ticks 10 / 50 / 100;
  * the bytes a tick moves per stream, derived from the shape: the carried column in and out against the emissions.
The number to put beside `push_call` is `OnlineDecoder.push` at the same size from tools/time_online.py in the same session.
The streams cycle through `--distinct` (default 256) different utterances: the times do not depend on the values.
usage: time_online_words.py [--streams 4096] [--tick 20] [--ticks 100] [--no-prefix] [--out result.json]"""
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
ap.add_argument("--streams", type=int, default=4096)
ap.add_argument("--tick", type=int, default=20)
ap.add_argument("--ticks", type=int, default=100)
ap.add_argument("--distinct", type=int, default=256)
ap.add_argument("--no-prefix", action="store_true", help="leave the prefix recognitions out (profiler runs)")
ap.add_argument("--out", default=None)
args = ap.parse_args()

W, n, M, D = 10, 5, 8, 39
U, TICK, NT = args.streams, args.tick, args.ticks
ctx = _hip.default_context(0)
base = min(args.distinct, U)
wl = bench.synth_workload(1101, base, W=W, n=n, M=M, D=D, tmin=NT * TICK, tmax=NT * TICK)
means, vars_, trans = wl["means"], wl["vars"], wl["trans"]
distinct = [wl["X"][wl["off"][u]:wl["off"][u + 1]] for u in range(base)]
xs = [distinct[u % base] for u in range(U)]
truth = wl["words"][np.arange(U) % base]


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
ids = np.arange(U)
ev = [ctx.new_event() for _ in range(4)]


def clock(fn):
    ctx.sync()
    t0 = time.perf_counter()
    r = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, r


def chunks_of(k):
    return [x[k * TICK:(k + 1) * TICK] for x in xs]


# ---- the serving loop: push + result every tick ----
on = rec.online(U)
rows = []
for k in range(NT):
    ch = chunks_of(k)
    ms_push, _ = clock(lambda: on.push(ids, ch))
    ms_result, res = clock(lambda: on.result())
    rows.append(dict(tick=k, push_ms=ms_push, result_ms=ms_result))
online_words, online_costs = res[0], res[1]["costs"]
on.close()

# ---- the parts of a push, on the same chunks: device times between events, host times of the steps beside them ----
on2 = rec.online(U)
for k in range(NT):
    ch = chunks_of(k)
    ctx.sync()
    t0 = time.perf_counter()
    ctx.record(ev[0])
    b = _hip.Batch(ctx, ch, dtype=rec.dtype)
    ctx.record(ev[1])
    t1 = time.perf_counter()
    b.loglik(rec.gmm, fetch=False)
    ctx.record(ev[2])
    t2 = time.perf_counter()
    on2.push_batch(ids, b)
    ctx.record(ev[3])
    ctx.sync()
    t3 = time.perf_counter()
    b.close()
    rows[k].update(batch_upload_dev_ms=ctx.elapsed_ms(ev[0], ev[1]), loglik_dev_ms=ctx.elapsed_ms(ev[1], ev[2]),
                   carried_sweep_dev_ms=ctx.elapsed_ms(ev[2], ev[3]), batch_upload_host_ms=(t1 - t0) * 1e3,
                   loglik_enqueue_host_ms=(t2 - t1) * 1e3, sweep_enqueue_and_drain_host_ms=(t3 - t2) * 1e3)
w2, r2 = on2.result()
same = bool(np.array_equal(w2, online_words) and np.array_equal(r2["costs"], online_costs))
on2.close()

# ---- what a caller has to do today: recognize() on the prefix ----
prefix = None
if not args.no_prefix:
    prefix = {}
    for k in (10, 50, 100):
        if k > NT:
            continue
        pre = [x[:k * TICK] for x in distinct]
        pre = [pre[u % base] for u in range(U)]
        ms, got = clock(lambda: rec.recognize(pre))
        prefix[str(k)] = ms
        if k == NT:
            same = same and bool(np.array_equal(got[0], online_words) and np.allclose(got[1], online_costs, rtol=1e-12, atol=0.0))

med = lambda key: float(np.median([r[key] for r in rows[1:]]))
tick_s = TICK / 100.0
esz = np.dtype(rec.dtype).itemsize
out = dict(shape=dict(W=W, n=n, M=M, D=D, streams=int(U), tick_frames=TICK, ticks=NT, distinct_utterances=int(base)),
           online_equals_recognize=same, accuracy=float(np.mean(online_words == truth)),
           per_tick_ms=dict(push_call=med("push_ms"), result_all_streams=med("result_ms"),
                            device=dict(batch_creation_and_upload=med("batch_upload_dev_ms"), likelihoods=med("loglik_dev_ms"),
                                        carried_sweep=med("carried_sweep_dev_ms")),
                            host=dict(batch_creation_and_upload=med("batch_upload_host_ms"), likelihoods_enqueue=med("loglik_enqueue_host_ms"),
                                      sweep_enqueue_and_drain=med("sweep_enqueue_and_drain_host_ms"))),
           realtime_streams_per_gpu=dict(push_only=U * tick_s * 1e3 / med("push_ms"),
                                         push_and_result_every_tick=U * tick_s * 1e3 / (med("push_ms") + med("result_ms"))),
           bytes_per_stream_per_tick=dict(state_in_and_out=2 * 8 * n * W, emissions=TICK * n * W * esz,
                                          state_over_emissions=2 * 8 * n * W / float(TICK * n * W * esz),
                                          state_resident=8 * n * W),
           ticks=rows)
if prefix is not None:
    out["recognize_prefix_ms"] = prefix
    out["recognize_prefix_over_push_and_result"] = {k: v / (med("push_ms") + med("result_ms")) for k, v in prefix.items()}
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
