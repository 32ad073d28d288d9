#!/usr/bin/env python3
"""Online decode FROM AUDIO at serving size: the configs[4] model of tools/time_online.py (10 words x 5 states, 8 mixtures,
D = 39, fp64) and `--streams` (default 4 096) live streams that take `--tick` (default 3 200) int16 samples per tick --
0.2 s of audio at 16 kHz, 20 feature frames once the pipeline is full (the first tick gives 16: the front-end looks two
frames ahead and computes frames in pairs).

Per tick (host clock around work that ends in a device synchronise; medians over the ticks behind the first):
  * `OnlineDecoder.push_audio` as a whole, and its parts: `StreamingFrontend.push` (host packing + upload + MFCC + stack +
    carry, one synchronising call) with the DEVICE times of its phases from HIP events (upload, MFCC kernel, stack kernel,
    carry kernel: gh_stream_profile), the likelihoods and the online sweep;
  * the same tick through `OnlineDecoder.push` with ready-made feature frames (fetched from the front-end beforehand);
and once: `features_from_signals(normalize=)` on the same total audio in one shot, and whether the two decodes agree.
usage: time_stream_frontend.py [--streams 4096] [--tick 3200] [--ticks 8] [--out result.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-recognition_amd")):
    sys.path.insert(0, p)
import numpy as np
import bench
import sr.recognition as R
from sr.feature import StreamingFrontend, feature_stats, features_from_signals
from sr.recognition import _hip
from sr.recognition.batch import ContinuousDecoder

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=4096)
ap.add_argument("--tick", type=int, default=3200)
ap.add_argument("--ticks", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()

W, n, M, D = 10, 5, 8, 39
U, TICK, NT, RATE = args.streams, args.tick, args.ticks, 16000
ctx = _hip.default_context(0)
wl = bench.synth_workload(1005, 1, W=W, n=n, M=M, D=D)
means, vars_, trans = wl["means"], wl["vars"], wl["trans"]
rng = np.random.default_rng(1006)
# audio: noise with a tone whose pitch moves per stream and per 0.1 s (the numbers decoded do not matter, the work does)
L = TICK * NT
tt = np.arange(L) / RATE
pcm = np.empty((U, L), dtype=np.int16)
for lo in range(0, U, 256):
    k = min(256, U - lo)
    f = 200.0 + 1800.0 * rng.random((k, 1)) + 400.0 * np.sin(2 * np.pi * rng.random((k, 1)) * tt * 3)
    x = 3000.0 * np.sin(2 * np.pi * f * tt) + 300.0 * rng.standard_normal((k, L))
    pcm[lo:lo + k] = np.clip(np.round(x), -32768, 32767).astype(np.int16)
norm = feature_stats(list(pcm[:64]), RATE)


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
ids = np.arange(U)
T_all = int(_hip.stream_frames_ready(L, 400, 160, True))
chunks = [[pcm[u, k * TICK:(k + 1) * TICK] for u in range(U)] for k in range(NT)]
ends = [None] * (NT - 1) + [np.ones(U, dtype=bool)]


def clock(fn):
    ctx.sync()
    t0 = time.perf_counter()
    r = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, r


# ---- push_audio as a whole; round 0 warms up ----
fe = StreamingFrontend(U, RATE, normalize=norm, max_chunk=TICK)
on = dec.online(U, max_frames=T_all, frontend=fe)
rows = None
for rnd in range(2):
    on.reset()
    rows = [dict(tick=k, push_audio_ms=clock(lambda: on.push_audio(ids, chunks[k], ends[k]))[0]) for k in range(NT)]
audio_words, audio_info = on.result()
on.reset()
# ---- its parts, on the same chunks; the frames are kept for the feature-frame leg ----
fe.backend.profile(True)
frames = [None] * NT
for rnd in range(2):
    on.reset()
    for k in range(NT):
        ms_fe, b = clock(lambda: fe.push(ids, chunks[k], ends[k]))
        ph = fe.backend.phase_ms()
        ms_ll, _ = clock(lambda: b.loglik(dec.gmm, fetch=False))
        ms_sw, _ = clock(lambda: on.push_batch(ids, b))
        rows[k].update(frontend_push_ms=ms_fe, device_upload_ms=ph["upload"], device_mfcc_ms=ph["mfcc"], device_stack_ms=ph["stack"],
                       device_carry_ms=ph["carry"], loglik_ms=ms_ll, online_sweep_ms=ms_sw, frames_per_stream=int(b.lengths[0]))
        if rnd:
            frames[k] = b.features()
        b.close()
fe.backend.profile(False)
# ---- the same ticks through push with ready-made feature frames ----
on2 = dec.online(U, max_frames=T_all)
for rnd in range(2):
    on2.reset()
    for k in range(NT):
        rows[k]["push_features_ms"] = clock(lambda: on2.push(ids, frames[k]))[0]
feat_words, feat_info = on2.result()
# ---- the one-shot front-end on the same total audio ----
one = []
for rep in range(3):
    ms, b = clock(lambda: features_from_signals(list(pcm), RATE, normalize=norm))
    one.append(ms)
    if rep < 2:
        b.close()
one_words, one_info = dec.decode_batch(b)
streamed = np.concatenate([np.concatenate([frames[k][u] for k in range(NT)]) for u in range(0, U, max(1, U // 16))])
whole = np.concatenate([b.features()[u] for u in range(0, U, max(1, U // 16))])
b.close()
same = bool(audio_words == feat_words == one_words and np.array_equal(audio_info["best_end"], one_info["best_end"])
            and np.array_equal(streamed, whole))

med = lambda key: float(np.median([r[key] for r in rows[1:]]))
keys = ("push_audio_ms", "frontend_push_ms", "device_upload_ms", "device_mfcc_ms", "device_stack_ms", "device_carry_ms", "loglik_ms",
        "online_sweep_ms", "push_features_ms")
out = dict(shape=dict(W=W, n=n, M=M, D=D, streams=int(U), tick_samples=TICK, ticks=NT, sample_rate=RATE, frames_per_stream=T_all,
                      audio_mb_per_tick=U * TICK * 2 / 1e6),
           streamed_equals_one_shot=same,
           per_tick_ms={k[:-3]: med(k) for k in keys},
           first_tick_ms={k[:-3]: rows[0][k] for k in keys},
           realtime_streams_per_gpu=dict(push_audio=U * (TICK / RATE) * 1e3 / med("push_audio_ms"),
                                         push_features=U * (TICK / RATE) * 1e3 / med("push_features_ms")),
           one_shot_features_from_signals_ms=float(np.median(one)), one_shot_runs_ms=[float(x) for x in one],
           streamed_frontend_all_ticks_ms=float(sum(r["frontend_push_ms"] for r in rows)),
           ticks=rows)
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
