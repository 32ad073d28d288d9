# -*- coding: utf-8 -*-
"""Streaming endpoint detection on the GPU (csrc/gh_endpoint_stream.hip).

The contract is EXACT: whatever way a recording is cut into chunks, its stream's events, frames_done and per-frame
is_speech / level / background / energy are those of the one-shot `detect_endpoints(..., max_segments=8, want_frames=True)`
on the whole recording on the same device -- the same integer sums and the same fp64 operations in the same order, so there
is no tolerance and no recording is left out.  (`n_segments < 8` is asserted: the one-shot detector never stopped.)
G21 -- the reference's own record_callback -- is fed in its own chunks of 'samples per frame'; its second config frames
400 samples every 160, which a stream refuses (the frames fall behind the audio without bound), so those three recordings
are checked to be refused and the seven of the first config are streamed."""
import numpy as np
import pytest

import audio_capture_ref as A
import stream_endpoints_ref as S
from conftest import load_golden
from test_audio_capture_host import g21_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def AC():
    import sr.audio_capture as AC
    return AC


@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


def stream_all(ep, rng, signals, ids_of, plans, end_alone, skip=0.0, want_frames=True):
    """Feed signals[k] to stream ids_of[k] with the chunk lengths plans[k] (None: the recording sits this run out), all
    streams in the same push calls, ids permuted per push; with `skip` a live stream sits a tick out with that probability.
    end_alone[k]: the end flag comes on an empty chunk of its own.  Returns per recording (events, frames dict, frames_done)."""
    K = len(signals)
    plans = [None if p is None else list(p) + ([0] if alone or not p else []) for p, alone in zip(plans, end_alone)]
    pos, step = [0] * K, [0] * K
    events, frames, done = [[] for _ in range(K)], [[] for _ in range(K)], [0] * K
    while any(p is not None and step[k] < len(p) for k, p in enumerate(plans)):
        live = [int(k) for k in rng.permutation(K) if plans[k] is not None and step[k] < len(plans[k]) and rng.random() >= skip]
        chunks = [signals[k][pos[k]:pos[k] + plans[k][step[k]]] for k in live]
        end = [step[k] == len(plans[k]) - 1 for k in live]
        ids = [ids_of[k] for k in live]
        r = ep.push(ids, chunks, end, want_frames=want_frames)
        assert np.all(np.diff([ids.index(int(s)) for s in r["stream"]]) >= 0)      # ordered by position in ids
        for s, kind, sample, is_open in zip(r["stream"], r["kind"], r["sample"], r["open"]):
            events[ids_of.index(int(s))].append((int(kind), int(sample), bool(is_open)))
        for u, k in enumerate(live):
            if want_frames:
                frames[k].append({key: r[key][u].copy() for key in ("is_speech", "level", "background", "energy")})
            done[k] = int(r["frames_done"][u])
            pos[k] += plans[k][step[k]]
            step[k] += 1
        assert ep.samples[ids].tolist() == [pos[k] for k in live]
    cat = [{key: np.concatenate([f[key] for f in fr]) for key in ("is_speech", "level", "background", "energy")} if fr else None
           for fr in frames]
    return events, cat, done


# ------------------------------------------------------------------ 4: streaming equals one-shot, exactly
@pytest.mark.parametrize("name,raw", S.CONFIGS, ids=[c[0] for c in S.CONFIGS])
def test_streams_equal_the_one_shot_detector_exactly(AC, name, raw):
    cfg = A.derive(raw)
    width, stride, rate = cfg['samples per frame'], cfg['frame stride'], raw['sample rate']
    sigs, ids_of = S.recordings(raw, 40)
    assert len(set(ids_of)) == S.N_RECORDINGS and max(ids_of) < S.N_STREAMS
    one = AC.detect_endpoints(sigs, dict(raw), max_segments=8, want_frames=True)
    assert np.all(one["n_segments"] < 8)                   # the one-shot detector never stopped
    assert one["n_segments"].sum() >= 10 and one["open"].any()
    assert one["n_segments"][3] == 3 and one["frames_done"][0] == 0 and one["frames_done"][1] == 0 and 0 < one["frames_done"][2] < 11
    assert one["open"][4] or raw['forget factor'] == 5     # (that config's background catches up with a long burst: others are open)
    ep = AC.StreamingEndpointer(S.N_STREAMS, dict(raw), max_chunk=int(3.5 * rate))
    rng = np.random.default_rng(43)
    cuts = [S.cuttings(rng, len(x), width, stride, index) for index, x in enumerate(sigs)]
    for how in ("whole", "width", "1024", "random", "one"):
        ep.reset()
        plans = [c.get(how) for c in cuts]
        assert sum(p is not None for p in plans) == (len(S.SAMPLE_BY_SAMPLE) if how == "one" else S.N_RECORDINGS)
        alone = [bool(index % 2) for index in range(len(sigs))]
        events, frames, done = stream_all(ep, rng, sigs, ids_of, plans, alone, skip=0.2 if how == "random" else 0.0)
        for u, x in enumerate(sigs):
            if plans[u] is None:
                continue
            k = int(one["n_segments"][u])
            starts, ends, is_open = S.segments_of(events[u])
            assert starts == one["start"][u, :len(starts)].tolist() and ends == one["end"][u, :k].tolist(), (how, u)
            assert len(ends) == k and len(starts) == k and is_open == bool(one["open"][u]), (how, u)
            assert [o for _, _, o in events[u]] == [False] * (len(events[u]) - is_open) + [True] * is_open, (how, u)
            assert done[u] == int(one["frames_done"][u]) == A.frame_count(len(x), width, stride), (how, u)
            for key in ("is_speech", "level", "background", "energy"):
                np.testing.assert_array_equal(frames[u][key], one[key][u], err_msg="%s of recording %d, cutting %s" % (key, u, how))
    ep.close()


# ------------------------------------------------------------------ 5: G21
def test_g21_in_the_callbacks_own_chunks(AC):
    g = load_golden("G21_endpoints")
    cases = list(g21_cases(g))
    mine = [c for c in cases if c[4]['samples per frame'] % c[4]['frame stride'] == 0]
    other = [c for c in cases if c not in mine]
    assert len(mine) == 7 and len(other) == 3
    with pytest.raises(ValueError, match="detect_endpoints"):
        AC.StreamingEndpointer(3, dict(other[0][3]))
    raw, der = mine[0][3], mine[0][4]
    width = der['samples per frame']
    for cfg in (dict(raw), dict(der)):                     # as the user writes it, and already derived
        ep = AC.StreamingEndpointer(len(mine), cfg, max_chunk=width)
        sigs = [c[2] for c in mine]
        plans = [[min(width, len(x) - k) for k in range(0, len(x), width)] for x in sigs]
        events, _, _ = stream_all(ep, np.random.default_rng(5), sigs, list(range(len(mine))), plans, [False] * len(mine), want_frames=False)
        assert len(ep.backend.push(np.arange(0), np.zeros(0, dtype=np.int16), [0])["stream"]) == 0      # (an empty push is valid)
        for u, (si, pp, x, _, _) in enumerate(mine):
            starts, ends, is_open = S.segments_of(events[u])
            assert (starts[0] if starts else 0) == int(g[pp + "start"]), si
            first_end = ends[0] if ends and not (is_open and len(ends) == 1) else 0
            assert first_end == int(g[pp + "end"]), si
            # `started` after the first segment: the golden's detector stopped there; a stream goes on, so compare at that point
            assert (len(starts) > 0 and first_end == 0) == bool(g[pp + "started"]), si
        ep.close()
    assert raw == mine[0][3]                               # derived on a copy


def test_g21_started_flag_of_the_push(AC):
    """`started` as `push` returns it, on the two G21 recordings whose speech never ends and one that has none."""
    g = load_golden("G21_endpoints")
    for si, pp, x, raw, der in g21_cases(g):
        if si not in (3, 4, 5):
            continue
        ep = AC.StreamingEndpointer(1, dict(raw), max_chunk=len(x))
        r = ep.push([0], [x], [True])
        assert bool(r["started"][0]) == bool(g[pp + "started"]), si
        assert int(r["frames_done"][0]) == A.frame_count(len(x), der['samples per frame'], der['frame stride'])
        if g[pp + "started"]:
            assert r["kind"].tolist() == [0, 1] and r["sample"].tolist() == [int(g[pp + "start"]), len(x) - 1] and r["open"].tolist() == [False, True]
        else:
            assert len(r["kind"]) == 0
        ep.close()


# ------------------------------------------------------------------ 6: three bursts
def test_three_bursts_in_ticks_of_1024(AC):
    x = S.burst_signal(np.random.default_rng(0), 48000, 50, [(8000, 13000), (22000, 27000), (36000, 41000)])
    ep = AC.StreamingEndpointer(2)
    got = []
    for t in range(0, len(x), 1024):
        r = ep.push([1], [x[t:t + 1024]], [t + 1024 >= len(x)])
        got += list(zip(r["kind"].tolist(), r["sample"].tolist(), r["open"].tolist()))
    starts, ends, is_open = S.segments_of(got)
    assert list(zip(starts, ends)) == [(9920, 17280), (23920, 31280), (37920, 45280)] and not is_open
    assert [k for k, _, _ in got] == [0, 1] * 3
    ep.close()


# ------------------------------------------------------------------ 7: reset and refusals through the real library
def test_reset_and_refusals(AC, hip):
    rng = np.random.default_rng(7)
    x = S.burst_signal(rng, 12000, 50, [(2000, 6000)])                                 # 0.75 s of noise behind the burst: the segment ends
    ep = AC.StreamingEndpointer(3, max_chunk=6000)
    fresh = ep.push([1], [x[:6000]])
    fresh2 = ep.push([1], [x[6000:]], [True])
    want = [fresh[k].tolist() + fresh2[k].tolist() for k in ("kind", "sample", "open")]
    assert want[0] == [0, 1] and not any(want[2])
    ep.push([2, 0], [x[:5000], x[:100]])
    before = ep.samples
    assert before.tolist() == [100, 12000, 5000]
    for ids, chunks, end in (([0, 0], [x[:10], x[:10]], None),                         # an id named twice
                             ([0, 3], [x[:10], x[:10]], None),                         # an id out of range
                             ([0, 2], [x[:10], x[:6001]], None),                       # a chunk over max_chunk
                             ([0, 1], [x[:10], x[:10]], None),                         # audio after the end
                             ([0], [x[:10].astype(np.float32)], None)):                # a dtype that is not int16
        with pytest.raises(ValueError):
            ep.push(ids, chunks, end)
        assert ep.samples.tolist() == before.tolist()
        np.testing.assert_array_equal(ep.backend.samples(), before)                    # ... nor in the library
    # the library refuses on its own as well (the raw binding), and moves nothing
    z = np.zeros(20, dtype=np.int16)
    for ids, pcm, off in (([0, 0], z, [0, 10, 20]), ([0, 3], z, [0, 10, 20]), ([1], z, [0, 20]),
                          ([0, 2], np.zeros(6011, dtype=np.int16), [0, 10, 6011])):
        with pytest.raises(hip.BackendError):
            ep.backend.push(ids, pcm, off)
        np.testing.assert_array_equal(ep.backend.samples(), before)
    with pytest.raises(hip.BackendError):
        hip.EndpointStream(ep.ctx, 2, dict(ep.config, **{'samples per frame': 400, 'frame stride': 160}))
    # a reset id reproduces a fresh recording's result: stream 2 is 5000 samples into another one
    ep.reset([2])
    assert ep.samples.tolist() == [100, 12000, 0]
    a = ep.push([2], [x[:6000]])
    b = ep.push([0, 2], [x[100:200], x[6000:]], [False, True])
    assert [a[k].tolist() + b[k].tolist() for k in ("kind", "sample", "open")] == want
    assert b["stream"].tolist() == [2] and b["frames_done"].tolist() == [1, A.frame_count(12000, 160, 80)]
    ep.close()


# ------------------------------------------------------------------ 8: end to end
TICK = 3200


@pytest.fixture(scope="module")
def e2e(hip):
    """The recipe of test_gpu_stream_frontend.py's `e2e` fixture (3-word model, `feature_stats` normalisation) on six 16 kHz
    recordings with two bursts each; the last one ends while speech is open."""
    import sr.recognition as R
    from sr.feature import feature_stats
    from sr.recognition.batch import ContinuousDecoder
    from test_gpu_api import make_hmm
    ctx = hip.default_context()
    rng = np.random.default_rng(17)
    rate = 16000
    lens = [42000, 43333, 45000, 46111, 48000, 36000]                     # 0.75 s and more of noise behind the second burst
    sigs = [S.burst_signal(rng, n, 40, [(4000, 10000), (24000, 30000)], freq=300.0 + 150 * i, rate=rate) for i, n in enumerate(lens)]
    sigs[5] = S.burst_signal(rng, lens[5], 40, [(4000, 10000), (24000, 36000)], rate=rate)       # ... or speech up to the end
    norm = feature_stats(sigs, rate)
    W, n, M, D = 3, 4, 2, 39
    trans = np.full((n, n), np.inf)
    for i in range(n):
        trans[i, i] = -np.log(0.8) if i < n - 1 else 0.0
        if i < n - 1:
            trans[i + 1, i] = -np.log(0.2)
    hmms = [make_hmm(R, rng.normal(size=(n, M, D)), rng.uniform(0.5, 1.5, size=(n, M, D)), rng.dirichlet(np.ones(M), size=n), trans)
            for _ in range(W)]
    dec = ContinuousDecoder(hmms, grammar="loop", ctx=ctx)
    return dict(sigs=sigs, norm=norm, dec=dec, rate=rate)


@pytest.fixture(scope="module")
def offline(AC, e2e):
    """Per recording the offline utterances [(begin, stop, open, words, end_cost)]: trim_ranges of the one-shot detection, each
    slice through the one-shot front-end and decoder ALONE."""
    from sr.feature import features_from_signals
    sigs, dec = e2e["sigs"], e2e["dec"]
    cfg = AC.default_config(e2e["rate"])
    det = AC.detect_endpoints(sigs, dict(cfg), max_segments=8)
    assert det["n_segments"].tolist() == [2] * 6 and det["open"].tolist() == [False] * 5 + [True]
    begin, stop = AC.trim_ranges(det, [len(x) for x in sigs], dict(cfg))
    rec = np.repeat(np.arange(6), det["n_segments"])
    out = [[] for _ in sigs]
    for r, b, e in zip(rec, begin, stop):
        batch = features_from_signals([sigs[r][b:e]], e2e["rate"], normalize=e2e["norm"])
        words, info = dec.decode_batch(batch)
        out[r].append((int(b), int(e), bool(det["open"][r]) and len(out[r]) == 1, words[0], np.array(info["end_cost_flat"]), batch.lengths[0]))
        batch.close()
    return out


def ticks_of(sigs):
    for t in range(max(-(-len(s) // TICK) for s in sigs)):
        live = [k for k, s in enumerate(sigs) if t * TICK < len(s)]
        yield live, [sigs[k][t * TICK:(t + 1) * TICK] for k in live], [(t + 1) * TICK >= len(sigs[k]) for k in live]


@pytest.mark.parametrize("mode", ["max_frames", "window"])
def test_push_recording_decodes_like_the_offline_path(AC, hip, e2e, offline, mode):
    from sr.feature import StreamingFrontend
    dec, sigs, rate = e2e["dec"], e2e["sigs"], e2e["rate"]
    ep = AC.StreamingEndpointer(6, AC.default_config(rate), max_chunk=TICK)
    fe = StreamingFrontend(6, rate, normalize=e2e["norm"], max_chunk=ep.max_piece)
    longest = max(u[5] for per in offline for u in per)
    with pytest.raises(ValueError):
        dec.online(6, max_frames=longest, frontend=StreamingFrontend(6, rate, normalize=e2e["norm"], max_chunk=TICK), endpointer=ep)
    on = dec.online(6, frontend=fe, endpointer=ep, **({"max_frames": longest} if mode == "max_frames" else {"window": longest + 8}))
    got, costs = [[] for _ in sigs], {}
    real_result = on.result

    def spy(ids, want_path=False):                          # (push_recording returns the words; the end costs are the decoder's)
        words, info = real_result(ids, want_path=want_path)
        for k, c in zip(ids, info["end_cost"]):
            costs.setdefault(int(k), []).append(np.array(c))
        return words, info
    on.result = spy
    seen, compared = {}, 0
    for ids, chunks, end in ticks_of(sigs):
        for u in on.push_recording(ids, chunks, end):
            got[u["stream"]].append(u)
            if mode == "window":                            # what commit had settled of it is a prefix of its final words
                pre = seen.pop(u["stream"], [])
                assert u["words"][:len(pre)] == pre
                compared += 1
        if mode == "window":
            for k in ids:
                if on.frames[k]:
                    seen[k] = on.settled([k])[0][0]
    assert compared == (12 if mode == "window" else 0)
    for r, per in enumerate(offline):
        assert [(u["begin"], u["stop"], u["open"]) for u in got[r]] == [(b, e, o) for b, e, o, _, _, _ in per], r
        assert [u["words"] for u in got[r]] == [w for _, _, _, w, _, _ in per] and all(len(u["words"]) >= 1 for u in got[r]), r
        for c, (_, _, _, _, want, _) in zip(costs[r], per):
            np.testing.assert_allclose(c.reshape(-1), want, rtol=1e-12)
    assert on.frames.tolist() == [0] * 6 and fe.samples.tolist() == [0] * 6 and ep.samples.tolist() == [len(s) for s in sigs]
    on.close()
    fe.close()
    ep.close()
