#!/usr/bin/env python3
"""Streaming endpoint detection at the serving size of the other online tools: `--streams` (default 4 096) live recordings at
16 kHz with the default config (frames of 320 samples every 160), `--tick` (default 3 200) int16 samples per tick, seeded
burst signals (noise with a tone burst of 0.4 .. 0.8 s about every 2 s; 64 distinct recordings, rolled per stream).

  (a) `StreamingEndpointer.push` per tick: call time (host clock around a device synchronise) and the DEVICE time of its
      phases from HIP events (upload, energy kernel, classifier kernel, carry kernel: gh_epstream_profile);
  (b) `detect_endpoints(max_segments=64)` on the prefix at ticks 10, 50 and 100: what a caller has to do today to learn the
      same at that tick -- and whether the streamed events up to there are the one-shot result;
  (c) `OnlineDecoder.push_recording` per tick against `push_audio` per tick on the same audio (configs[4] model of
      tools/time_online.py, `--decode-ticks` ticks): what the gate costs.  push_audio decodes ALL the audio as one utterance
      per stream, push_recording only what the gate lets through, so (c) is the cost of a live path with endpoints
      against one without, not the same work twice;
and the derivable figure: bytes a tick moves per stream.  No threshold is set on any of these.
usage: time_stream_endpoints.py [--streams 4096] [--tick 3200] [--ticks 100] [--decode-ticks 20] [--out result.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "speech-recognition_amd")):
    sys.path.insert(0, p)
import numpy as np
import bench
import sr.recognition as R
from sr.audio_capture import StreamingEndpointer, default_config, detect_endpoints
from sr.feature import StreamingFrontend, feature_stats
from sr.recognition import _hip
from sr.recognition.batch import ContinuousDecoder

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=4096)
ap.add_argument("--tick", type=int, default=3200)
ap.add_argument("--ticks", type=int, default=100)
ap.add_argument("--decode-ticks", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()

U, TICK, NT, ND, RATE = args.streams, args.tick, args.ticks, min(args.decode_ticks, args.ticks), 16000
ctx = _hip.default_context(0)
cfg = default_config(RATE)
rng = np.random.default_rng(2024)
L = TICK * NT
tt = np.arange(L) / RATE
base = []
for k in range(64):
    x = rng.normal(0.0, 50.0, size=L)
    a = int(rng.integers(RATE // 4, RATE))
    while a < L:
        b = min(L, a + int(rng.integers(4 * RATE // 10, 8 * RATE // 10)))
        x[a:b] += 4000.0 * np.sin(2 * np.pi * (200.0 + 25.0 * k) * tt[a:b])
        a = b + int(rng.integers(3 * RATE // 2, 5 * RATE // 2))
    base.append(np.clip(np.round(x), -32768, 32767).astype(np.int16))
pcm = np.empty((U, L), dtype=np.int16)
for u in range(U):
    pcm[u] = np.roll(base[u % 64], (u // 64) * 1600)
say = lambda *a: print(*a, file=sys.stderr, flush=True)
say("audio ready: %d streams x %d samples" % (U, L))
ids = np.arange(U)
chunk = lambda k: [pcm[u, k * TICK:(k + 1) * TICK] for u in range(U)]


def clock(fn):
    ctx.sync()
    t0 = time.perf_counter()
    r = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, r


spread = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v))

# ---- (a) push per tick, (b) detect_endpoints on the prefix ----
ep = StreamingEndpointer(U, dict(cfg), max_chunk=TICK)
ep.push(ids, chunk(0))                                    # warm-up: scratch and staging buffer grow once
ep.reset()
ep.backend.profile(True)
rows, events, prefix = [], [[] for _ in range(min(U, 256))], {}
for k in range(NT):
    c = chunk(k)
    ms, r = clock(lambda: ep.push(ids, c))
    ph = ep.backend.phase_ms()
    rows.append(dict(tick=k, push_ms=ms, device_upload_ms=ph["upload"], device_energy_ms=ph["energy"], device_classify_ms=ph["classify"],
                     device_carry_ms=ph["carry"], events=int(len(r["stream"]))))
    for s, kind, smp in zip(r["stream"], r["kind"], r["sample"]):
        if s < len(events):
            events[int(s)].append((int(kind), int(smp)))
    if k + 1 in (10, 50, 100):
        sigs = [pcm[u, :(k + 1) * TICK] for u in range(U)]
        runs = []
        for rep in range(2):
            ms1, det = clock(lambda: detect_endpoints(sigs, dict(cfg), max_segments=64))
            runs.append(ms1)
        same = True
        for u in range(len(events)):                       # the streamed events so far against the one-shot result of the prefix
            ns = int(det["n_segments"][u]) - int(det["open"][u])
            want = sorted([(0, int(x)) for x in det["start"][u, :int(det["n_segments"][u])]] + [(1, int(x)) for x in det["end"][u, :ns]],
                          key=lambda e: e[1])
            same = same and want == events[u]
        say("tick %d: push %.2f ms, detect_endpoints on the prefix %s ms, equal %s" % (k + 1, ms, runs, same))
        prefix[str(k + 1)] = dict(detect_endpoints_ms=runs, seconds_of_audio=(k + 1) * TICK / RATE, streamed_events_equal_one_shot=bool(same))
        del sigs
ep.backend.profile(False)
width, stride = ep.width, ep.stride
bytes_per_stream = dict(chunk_in=2 * TICK, carry_read_max=2 * (ep.carry_cap - 1), carry_write_max=2 * (ep.carry_cap - 1), state_in_out=64, slot=96,
                        energies_written_and_read=16 * (TICK // stride), counts_and_started_out=5)
bytes_per_stream["total"] = int(sum(bytes_per_stream.values()))
out = dict(shape=dict(streams=int(U), tick_samples=TICK, ticks=NT, sample_rate=RATE, width=width, stride=stride,
                      audio_mb_per_tick=U * TICK * 2 / 1e6, new_frames_per_tick=TICK // stride),
           push=dict(call_ms=spread([r["push_ms"] for r in rows[1:]]),
                     device_upload_ms=spread([r["device_upload_ms"] for r in rows[1:]]),
                     device_energy_ms=spread([r["device_energy_ms"] for r in rows[1:]]),
                     device_classify_ms=spread([r["device_classify_ms"] for r in rows[1:]]),
                     device_carry_ms=spread([r["device_carry_ms"] for r in rows[1:]]),
                     events_total=int(sum(r["events"] for r in rows))),
           prefix_detect_endpoints=prefix, bytes_per_tick_per_stream=bytes_per_stream, ticks=rows)
ep.close()

# ---- (c) push_recording against push_audio ----
if ND > 0:
    W, n, M, D = 10, 5, 8, 39
    wl = bench.synth_workload(1005, 1, W=W, n=n, M=M, D=D)

    def hmm(i):
        h = R.HMM(n)
        h.gmm_states = []
        for s in range(n):
            g = R.GMM(wl["means"][i, s, 0].copy(), wl["vars"][i, s, 0].copy(), M)
            g.update_models(wl["means"][i, s].copy(), wl["vars"][i, s].copy(), wl["w"][i, s].copy())
            h.gmm_states.append(g)
        h.transitions = wl["trans"].copy()
        return h

    dec = ContinuousDecoder([hmm(i) for i in range(W)], grammar="loop", ctx=ctx)
    norm = feature_stats(list(pcm[:64, :ND * TICK]), RATE)
    T_all = int(_hip.stream_frames_ready(ND * TICK, 400, 160, True))
    fe = StreamingFrontend(U, RATE, normalize=norm, max_chunk=TICK)
    on = dec.online(U, max_frames=T_all, frontend=fe)
    audio = []
    for rnd in range(2):                                  # round 0 warms up
        on.reset()
        audio = [clock(lambda: on.push_audio(ids, chunk(k)))[0] for k in range(ND)]
    on.close()
    fe.close()
    say("push_audio per tick: %s" % audio)
    ep = StreamingEndpointer(U, dict(cfg), max_chunk=TICK)
    fe = StreamingFrontend(U, RATE, normalize=norm, max_chunk=ep.max_piece)
    on = dec.online(U, max_frames=T_all, frontend=fe, endpointer=ep)
    rec, gate, n_utt = [], [], 0
    for rnd in range(2):
        on.reset()
        rec, n_utt = [], 0
        for k in range(ND):
            ms, utts = clock(lambda: on.push_recording(ids, chunk(k)))
            rec.append(ms)
            n_utt += len(utts)
    say("push_recording per tick: %s" % rec)
    on.reset()
    for k in range(ND):                                   # the gate alone: endpointer push + host logic, nothing decoded
        gate.append(clock(lambda: ep.gate(ids, chunk(k)))[0])
    out["push_recording"] = dict(decode_ticks=ND, push_audio_ms=spread(audio[1:]), push_recording_ms=spread(rec[1:]), gate_alone_ms=spread(gate[1:]),
                                 utterances_finished=int(n_utt), note="the audio crosses the host link twice in push_recording")
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
