#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""Timing of sr.audio_capture on the GPU: N recordings of 1 - 2 s (seeded noise floor + one tone burst) at each rate:
  endpoints      `detect_endpoints` (gh_endpoints: upload, energy + classifier kernels, indices back) -- CALL time
  features       `features_from_signals` without and with `endpoints=True` -- CALL time
  cpu            the restatement of tests/audio_capture_ref.py (vectorised energies + Python loop) on ONE core, on
                 `--cpu-n` of the recordings, scaled to N
Call times are device-event times over windows of at least `--window` seconds after a warm-up.  Kernel times come from
a run of this script under `rocprofv3 --kernel-trace --stats` (`--kernels-only`: a few calls, no CPU leg); given
`--kernel-stats <csv>` of such a run, the energy kernel's average is set against the time to read the samples once at
the plain read rate tools/hbm_stream.hip measures on the same card (`--read-rate` in TB/s, or tools/bin/hbm_stream is
run in a child process before this one touches the GPU).  Prints one JSON line.

    python tools/time_endpoints.py [--n 10000] [--rates 8000,16000] [--window 1.0]"""
import argparse
import csv
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speech-recognition_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def recordings(n, rate, seed=1):
    rng = np.random.default_rng(seed)
    pool = rng.normal(0.0, 60.0, size=8 * rate + 2 * rate)
    t = np.arange(2 * rate) / rate
    out = []
    for _ in range(n):
        ln = int(rng.integers(rate, 2 * rate + 1))
        o = int(rng.integers(0, 8 * rate))
        x = pool[o:o + ln].copy()
        a = int(rng.integers(rate // 5, ln // 2))
        b = min(ln - rate // 8, a + int(rng.integers(rate // 4, rate // 2)))
        if b > a:
            x[a:b] += rng.uniform(1500, 6000) * np.sin(2 * np.pi * rng.uniform(200, 900) * t[:b - a])
        out.append(np.clip(np.round(x), -32768, 32767).astype(np.int16))
    return out


def measured_read_rate():
    exe = os.path.join(ROOT, "tools", "bin", "hbm_stream")
    if not os.path.exists(exe):
        return None
    try:
        txt = subprocess.run([exe], stdout=subprocess.PIPE, text=True, timeout=120).stdout
    except (OSError, subprocess.TimeoutExpired):
        return None
    rates = [float(m) for m in re.findall(r"read ([0-9.]+) TB/s", txt)]
    return max(rates) if rates else None


def window(ctx, fn, seconds):
    """Average device-event time of fn() in ms over a window of at least `seconds` (after two warm-up calls)."""
    fn()
    fn()
    e0, e1 = ctx.new_event(), ctx.new_event()
    ctx.record(e0)
    t0, reps = time.perf_counter(), 0
    while reps < 3 or time.perf_counter() - t0 < seconds:
        fn()
        reps += 1
    ctx.record(e1)
    return ctx.elapsed_ms(e0, e1) / reps, reps


def kernel_rows(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            for key in ("ep_energy_kernel", "ep_classify_kernel", "mfcc_kernel"):
                if key in name:
                    rows.setdefault(key, []).append(dict(name=name, calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3,
                                                         min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--rates", default="8000,16000")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--cpu-n", type=int, default=300)
    ap.add_argument("--read-rate", type=float, default=None, help="plain HBM read rate of this card in TB/s (tools/hbm_stream.hip)")
    ap.add_argument("--kernels-only", action="store_true", help="three calls of each leg and nothing else (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a --kernels-only run under rocprofv3")
    args = ap.parse_args()
    read_rate = args.read_rate
    if read_rate is None and not args.kernels_only:
        read_rate = measured_read_rate()          # (a child process, before this one opens the GPU)
    import sr.audio_capture as AC
    from sr.feature import features_from_signals
    from sr.recognition import _hip
    import audio_capture_ref as A
    ctx = _hip.default_context()
    out = dict(n=args.n, read_rate_tb_s=read_rate if read_rate is not None else "not measured", rates={})
    for rate in [int(r) for r in args.rates.split(",")]:
        sigs = recordings(args.n, rate)
        n_bytes = 2 * sum(len(x) for x in sigs)
        cfg = AC.default_config(rate)
        der = A.derive(cfg)
        n_frames = sum(A.frame_count(len(x), der['samples per frame'], der['frame stride']) for x in sigs)

        def plain():
            features_from_signals(sigs, rate).close()

        def endpointed():
            features_from_signals(sigs, rate, endpoints=True).close()

        legs = dict(endpoints=lambda: AC.detect_endpoints(sigs, cfg), features_plain=plain, features_endpointed=endpointed)
        if args.kernels_only:
            for fn in legs.values():
                for _ in range(3):
                    fn()
            continue
        res = AC.detect_endpoints(sigs, cfg)
        r = dict(sample_bytes=n_bytes, frames=n_frames, segments=int(res["n_segments"].sum()), open=int(res["open"].sum()),
                 chunks=ctx.last_chunks)
        if read_rate is not None:
            r["read_once_us"] = n_bytes / (read_rate * 1e12) * 1e6
        for name, fn in legs.items():
            ms, reps = window(ctx, fn, args.window)
            r[name + "_call_ms"] = ms
            r[name + "_calls_in_window"] = reps
        b = features_from_signals(sigs, rate)
        e = features_from_signals(sigs, rate, endpoints=True)
        r["frames_plain"], r["frames_endpointed"] = int(b.N), int(e.N)
        b.close()
        e.close()
        sub = sigs[:args.cpu_n]
        t0 = time.perf_counter()
        for x in sub:
            A.detect(x, der)
        r["cpu_one_core_s_scaled"] = (time.perf_counter() - t0) * args.n / max(len(sub), 1)
        r["cpu_recordings_timed"] = len(sub)
        r["endpoints_call_vs_cpu"] = r["cpu_one_core_s_scaled"] * 1e3 / r["endpoints_call_ms"]
        out["rates"][str(rate)] = r
    if args.kernel_stats:
        out["kernels"] = kernel_rows(args.kernel_stats)
        # one energy launch per rate and call, rates in the order given: the csv averages over both when two rates ran
        if read_rate is not None and len(out["rates"]) == 1 and out["kernels"].get("ep_energy_kernel"):
            r = next(iter(out["rates"].values()))
            avg = sum(k["avg_us"] * k["calls"] for k in out["kernels"]["ep_energy_kernel"]) / \
                sum(k["calls"] for k in out["kernels"]["ep_energy_kernel"])
            r["energy_kernel_us"] = avg
            r["energy_kernel_share_of_read_rate"] = r["read_once_us"] / avg
    print(json.dumps(out))


if __name__ == "__main__":
    main()
