# -*- coding: utf-8 -*-
"""The settled prefix and the windowed history of an online decode with a BIGRAM grammar on the device
(gh_online_create_bigram_settle; online_bigram_settle_kernel / online_bigram_segment_kernel in gh_online_settle.hip; the ring
store of viterbi_bigram_online_kernel), through `ContinuousDecoder.online_bigram(window=)` and `(max_frames=, settle=True)`.

C: the settled words after a commit; B: their begin frames (times=True).
  1. anchors are exact and maximal: at every tick settled_frames and C of a full-history and of a windowed session equal the
     restatement's (tests/online_settle_ref.py on tests/online_ref.py) on the batch's own fp64 likelihood matrix;
  2. prefix stability, device against device: C and B only ever extend, are a prefix of the session's own `result` now and at
     the end, and -- where the chosen end is finite -- of the result of a plain `online_bigram(max_frames)` session fed the
     same frames (bitwise the one-shot kernel, tests/test_gpu_online_bigram.py), whose words, begins, end costs and chosen
     ends the windowed `result` (settled + tail) equals as well;
  3. windowed == full history on long streams: window = the restatement's largest tail rounded up to a record word, streams
     long enough for the ring to wrap eight times;
  4. refusals through the real library; 5. recordings through a windowed decoder.
Every instantiated (n, skip) runs at W = 3 with 5 streams (a full row group of a wave and a partial one), W = 16 with
n = 5 and skip arcs makes every lane a hop target; the graph of W = 1 is a word loop to the library, and `online_bigram`
serves it from the loop session (same rows, same contract).  A stream is named in a tick while it still has frames to
take (its last tick included), like a caller that stops naming an utterance that has ended: the two utterances shorter
than a word, whose ends are +inf, then weigh as little in the tally of finite ends as they do in a served batch.
The conditions on the inputs (an anchor that advances at three ticks or more, a settled path through an entry row, 3/4 of
the (stream, tick) pairs with a finite chosen end) are asserted from the restatement BEFORE the device is compared."""
import numpy as np
import pytest

from online_ref import CarriedDecode
from online_settle_ref import SettledDecode
from test_gpu_online_bigram import M, D, audio_model, bigram_cpw, make_hmm, make_model, random_costs, ticks_of, word_trans, TICK  # noqa: F401
from test_gpu_online_settle import finite_end

pytestmark = pytest.mark.gpu

U, N_IDS = 5, 7
#          W   n  skip
SHAPES = ([(3, 2, False)] + [(3, n, s) for n in (3, 4, 5, 6, 7, 8, 12) for s in (False, True)] + [(3, 16, False)] +
          [(16, 5, True),      # every lane a hop target
           (1, 3, False)])     # one word: its entry row has one way in
LONG = [(3, 2, False), (3, 5, False), (16, 5, True), (3, 12, True), (1, 3, False)]       # CPW 4, 3, 2, 1, 4
assert {bigram_cpw(n, s) for _, n, s in SHAPES} == {4, 3, 2, 1} == {bigram_cpw(n, s) for _, n, s in LONG}
shape_id = lambda s: "W%d-n%d-%s" % (s[0], s[1], "skip" if s[2] else "plain")


def make_case(W, n, skip, seed=0):
    """Model, bigram costs with +inf pairs and starts, 5 utterances of 1 - 7 synthetic words (utterances 0 and 3 shorter than a
    word) after the recipe of test_gpu_online_settle.make_case, 5 long streams and the stream ids, scattered over 7.  No GPU."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(2300 + 77 * W + 2 * n + skip + 1000 * seed)
    means, vars_, w = make_model(rng, W, n)
    trans = [word_trans(rng, n, skip, last_self=rng.uniform(0.0, 0.3)) for _ in range(W)]
    B, init = random_costs(rng, W, rng.uniform(0.1, 0.3))

    def synth(words):
        segs = []
        for wd in words:
            Tw = int(rng.integers(n, 3 * n + 4))
            st = np.minimum(np.arange(Tw) * n // Tw, n - 1)
            comp = rng.integers(0, M, size=Tw)
            segs.append(means[wd, st, comp] + np.sqrt(vars_[wd, st, comp]) * rng.normal(size=(Tw, D)))
        return np.concatenate(segs)
    xs = []
    for u in range(U):
        if u % 3 == 0 and n > 2:
            xs.append(rng.normal(size=(int(rng.integers(2, max(3, n))), D)) * 2.0)      # shorter than any word
        else:
            xs.append(synth(rng.integers(0, W, size=rng.integers(1, 8) if u != 1 else 7)))
    ids = rng.permutation(N_IDS)[:U]
    graph, _ = packed_bigram_lattice(trans, n, B, init)
    nes = graph["row_state"] < 0
    return dict(W=W, n=n, skip=skip, means=means, vars=vars_, w=w, trans=trans, B=B, init=init, xs=xs, ids=ids, synth=synth,
                graph=graph, nes=nes, rw=np.where(nes, -1, graph["row_state"] // n), rng=rng,
                dense=dense_of(graph), ends=[int(e) for e in graph["end_rows"]])


def dense_of(graph):
    Rr = len(graph["row_state"])
    t = np.full((Rr, Rr), np.inf)
    t[graph["arc_to"], graph["arc_from"]] = graph["arc_cost"]
    return t


def live_schedule(rng, T, choices):
    """Ticks of (utterance indices still taking frames, column counts): 0- and 1-frame pushes, ranges that end inside a
    record word; an utterance leaves after the tick that ends it."""
    pos, out = np.zeros(len(T), dtype=np.int64), []
    while np.any(pos < T):
        live = np.flatnonzero(pos < T)
        cnt = np.minimum(rng.choice(choices, size=len(live)), T[live] - pos[live])
        out.append((live, cnt))
        pos[live] += cnt
    return out


def emissions(case, nll):
    """E [R, T] of the restatement from the rows [T, S] of a likelihood matrix (row_state = word * n + state)."""
    col = np.where(case["nes"], 0, case["graph"]["row_state"])
    return np.where(case["nes"][:, None], 0.0, np.asarray(nll, dtype=np.float64)[:, col].T)


def restate(case, E, chunks):
    """The restatement on the emission matrix E [R, T] of one stream fed in `chunks`: per tick dict(settled, words, tail:
    unsettled frames the history held before the commit, finite: the chosen end is a live cell, frames, entry: the
    settled path passes an entry row)."""
    cd = CarriedDecode(case["nes"], case["dense"], case["ends"])
    sd = SettledDecode(cd, case["rw"])
    t, out = 0, []
    for c in chunks:
        cd.push(E[:, t:t + c])
        t += int(c)
        tail = t - sd.settled_frames
        sd.commit()
        ec, bi, _ = cd.result()
        entry = False
        if sd.anchor is not None:
            rows = sd.path_from(sd.anchor[1], sd.anchor[0])[:, 0]
            entry = bool(np.any(case["nes"][rows] & (rows > 0)))
        out.append(dict(settled=sd.settled_frames, words=list(sd.words), tail=tail, frames=t, entry=entry,
                        finite=bool(bi >= 0 and np.isfinite(ec[bi]))))
    return out


def input_conditions(refs):
    """What the issue asks of the inputs, from the restatement alone: (most ticks at which one stream's anchor advances, a
    settled path passes an entry row, (stream, tick) pairs with >= 2 frames: finite, all)."""
    adv = max(sum(a["settled"] != b["settled"] for a, b in zip(r[1:], r[:-1])) + (r[0]["settled"] > 0) for r in refs)
    pairs = [tk for r in refs for tk in r if tk["frames"] >= 2]
    return adv, any(tk["entry"] for r in refs for tk in r), sum(tk["finite"] for tk in pairs), len(pairs)


def assert_input_conditions(refs):
    adv, entry, fin, pairs = input_conditions(refs)
    assert adv >= 3 and entry and 4 * fin >= 3 * pairs, (adv, entry, fin, pairs)


@pytest.fixture(scope="module")
def R():
    import sr.recognition as R
    return R


@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


def decoder_of(R, ctx, case, dtype=np.float64):
    from sr.recognition.batch import ContinuousDecoder
    hmms = [make_hmm(R, case["means"][i], case["vars"][i], case["w"][i], case["trans"][i]) for i in range(case["W"])]
    dec = ContinuousDecoder(hmms, grammar="bigram", bigram=case["B"], initial=case["init"], dtype=dtype, ctx=ctx)
    # (one word: its entry row is a loop row, the library sees the loop form and `online_bigram` serves it from the loop session)
    assert ("bigram" if case["W"] > 1 else "loop") in dec.lat.forms()
    np.testing.assert_array_equal(dec.row_state, case["graph"]["row_state"])
    assert list(dec.lat.end_rows[0]) == list(case["ends"])
    return dec


def per_stream_chunks(sched, u):
    return [int(cnt[list(live).index(u)]) for live, cnt in sched if u in live]


@pytest.fixture(scope="module", params=SHAPES, ids=shape_id)
def committed(request, R, hip, ctx):
    """Per shape: a full-history session that settles, a windowed one (window: the longest utterance, so nothing is ever
    refused) and a plain one, fed the 5 utterances in random column ranges with a commit after every push.  What the device
    said at every tick, and the restatement on the same likelihood matrix.  Computed once, shared by (1) and (2)."""
    case = make_case(*request.param)
    dec = decoder_of(R, ctx, case)
    rng = case["rng"]
    xs, ids, cpw = case["xs"], case["ids"], bigram_cpw(case["n"], case["skip"])
    b = hip.Batch(ctx, xs, dtype=np.float64)
    nll = b.loglik(dec.gmm, fetch=True)                                  # the matrix both sides decode
    T = np.asarray(b.lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(T)])
    sched = live_schedule(rng, T, [0, 1, 1, 2, 3, 5, 8, 13, 21])
    ref = [restate(case, emissions(case, nll[off[u]:off[u + 1]]), per_stream_chunks(sched, u)) for u in range(U)]
    assert_input_conditions(ref)                                         # before the device is looked at
    full = dec.online_bigram(N_IDS, max_frames=int(T.max()), settle=True, times=True)
    win = dec.online_bigram(N_IDS, window=-(-int(T.max()) // cpw) * cpw, times=True)
    plain = dec.online_bigram(N_IDS, max_frames=int(T.max()), times=True)
    assert full.settles and win.settles and not plain.settles and win.session.window and full.session.window is None
    pos = np.zeros(U, dtype=np.int64)
    ticks = []
    for live, cnt in sched:
        count = np.zeros(U, dtype=np.int64)
        count[live] = cnt
        for on in (full, win, plain):
            on.push_batch(ids, b, first=pos, count=count)                # (an utterance that has ended: 0 frames)
        pos = pos + count
        tick = dict(live=live, pos=pos.copy())
        for name, on in (("full", full), ("win", win)):
            new, new_t = on.commit(ids[live], want_times=True)
            words, frames = on.settled(ids[live])
            res, info = on.result(ids[live])
            tick[name] = dict(new=new, new_t=new_t, words=words, times=on.settled_times(ids[live]), frames=frames, result=res,
                              begins=[x.tolist() for x in info["begins"]], end_cost=info["end_cost"], best_end=info["best_end"])
        res, info = plain.result(ids[live])
        tick["plain"] = dict(result=res, begins=[x.tolist() for x in info["begins"]], end_cost=info["end_cost"],
                             best_end=info["best_end"], finite=finite_end(info))
        ticks.append(tick)
    final = plain.result(ids)
    assert final[0] == dec.decode_batch(b)[0]
    out = dict(case=case, ticks=ticks, ref=ref, sched=sched, T=T, final=final[0], final_begins=[x.tolist() for x in final[1]["begins"]],
               full_all=full.settled(ids)[0], win_all=win.settled(ids)[0])
    for on in (full, win, plain):
        on.close()
    b.close()
    return out


def test_anchors_are_exact_and_maximal(committed):
    ticks, ref = committed["ticks"], committed["ref"]
    k_of = [0] * U                                                        # the stream's own tick counter
    for tk in ticks:
        for i, u in enumerate(tk["live"]):
            want = ref[u][k_of[u]]
            assert want["frames"] == tk["pos"][u]
            for name in ("full", "win"):
                assert (int(tk[name]["frames"][i]), tk[name]["words"][i]) == (want["settled"], want["words"]), (name, u, k_of[u])
            k_of[u] += 1
    assert k_of == [len(r) for r in ref]


def test_prefix_stability_device_against_device(committed):
    ticks, final, final_begins = committed["ticks"], committed["final"], committed["final_begins"]
    compared = 0
    for name in ("full", "win"):
        before, before_t = [[] for _ in range(U)], [[] for _ in range(U)]
        for tk in ticks:
            d, p = tk[name], tk["plain"]
            np.testing.assert_array_equal(d["end_cost"], p["end_cost"])                  # bitwise
            np.testing.assert_array_equal(d["best_end"], p["best_end"])
            for i, u in enumerate(tk["live"]):
                C, Bt = d["words"][i], d["times"][i]
                assert C == before[u] + d["new"][i] and Bt == before_t[u] + d["new_t"][i]   # commits only ever extend
                assert len(C) == len(Bt) and d["frames"][i] <= max(tk["pos"][u] - 1, 0)
                assert C == d["result"][i][:len(C)] and Bt == d["begins"][i][:len(C)]   # ... and lead the session's own result
                if p["finite"][i]:
                    assert d["result"][i] == p["result"][i] and d["begins"][i] == p["begins"][i], (name, u)
                    assert C == p["result"][i][:len(C)] and Bt == p["begins"][i][:len(C)]
                    compared += len(C) > 0
                before[u], before_t[u] = C, Bt
        for u in range(U):                                                # the last commit of every stream against the final decode
            assert before[u] == final[u][:len(before[u])] and before_t[u] == final_begins[u][:len(before[u])]
    assert compared >= 6


def run_pair(hip, ctx, dec, case, dtype):
    """(3): a window= and a max_frames=, settle=True session on the same pushes of long streams."""
    rng = np.random.default_rng(5 + case["W"] + case["n"])
    n, cpw = case["n"], bigram_cpw(case["n"], case["skip"])
    xs = [case["synth"](rng.integers(0, case["W"], size=200))[:LONG_FRAMES + 3 * u] for u in range(U)]
    ids = case["ids"]
    b = hip.Batch(ctx, xs, dtype=dtype)
    nll = b.loglik(dec.gmm, fetch=True)
    T = np.asarray(b.lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(T)])
    sched = live_schedule(rng, T, [0, 1, 1, 2, 3, 5, 8, 13, 21, 34])
    ref = [restate(case, emissions(case, nll[off[u]:off[u + 1]]), per_stream_chunks(sched, u)) for u in range(U)]
    assert_input_conditions(ref)
    tail = max(tk["tail"] for r in ref for tk in r)
    window = -(-tail // cpw) * cpw
    ring_frames = (window // cpw + 1) * cpw
    assert T.min() >= 8 * ring_frames, "the streams must be long enough for the ring to wrap eight times: %d, %d" % (T.min(), ring_frames)
    full = dec.online_bigram(N_IDS, max_frames=int(T.max()), settle=True, times=True)
    win = dec.online_bigram(N_IDS, window=window, times=True)
    pos = np.zeros(U, dtype=np.int64)
    k_of = [0] * U
    compared = pairs = 0
    for live, cnt in sched:
        count = np.zeros(U, dtype=np.int64)
        count[live] = cnt
        for on in (full, win):
            on.push_batch(ids, b, first=pos, count=count)
        pos = pos + count
        new_f, new_w = full.commit(ids[live], want_times=True), win.commit(ids[live], want_times=True)
        assert new_f == new_w
        (wf, ff), (ww, fw) = full.settled(ids[live]), win.settled(ids[live])
        assert wf == ww and ff.tolist() == fw.tolist() == [ref[u][k_of[u]]["settled"] for u in live]
        assert wf == [ref[u][k_of[u]]["words"] for u in live]
        assert full.settled_times(ids[live]) == win.settled_times(ids[live])
        rf, info_f = full.result(ids[live])
        rw_, info_w = win.result(ids[live])
        np.testing.assert_array_equal(info_w["end_cost"], info_f["end_cost"])          # bitwise
        np.testing.assert_array_equal(info_w["best_end"], info_f["best_end"])
        np.testing.assert_array_equal(info_w["frames"], info_f["frames"])
        assert sorted(info_w) == sorted(info_f)
        ok = finite_end(info_f)
        for i, u in enumerate(live):
            pairs += pos[u] >= 2
            if ok[i]:
                assert rw_[i] == rf[i] and info_w["begins"][i].tolist() == info_f["begins"][i].tolist(), (u, k_of[u])
                compared += pos[u] >= 2
            k_of[u] += 1
    assert 4 * compared >= 3 * pairs and np.all(pos == T)
    final, fin_info = full.finish(ids)
    wfin, win_info = win.finish(ids)
    assert wfin == final and not win.frames.any() and win.settled()[0] == [[]] * N_IDS
    assert [x.tolist() for x in win_info["begins"]] == [x.tolist() for x in fin_info["begins"]]
    full.close()
    win.close()
    b.close()


LONG_FRAMES = 520


@pytest.mark.parametrize("shape", LONG, ids=shape_id)
def test_windowed_equals_full_history(R, hip, ctx, shape):
    case = make_case(*shape)
    run_pair(hip, ctx, decoder_of(R, ctx, case), case, np.float64)


def test_windowed_equals_full_history_fp32_likelihoods(R, hip, ctx):
    case = make_case(*LONG[1])
    run_pair(hip, ctx, decoder_of(R, ctx, case, dtype=np.float32), case, np.float32)


def test_refusals(R, hip, ctx):
    """A push past the window is refused as a whole with nothing moved, through the decoder and through the binding; a
    windowed decoder offers no paths and its session no `result`; the default session keeps refusing `commit`."""
    case = make_case(3, 5, False)
    dec = decoder_of(R, ctx, case)
    cpw = bigram_cpw(5, False)
    x = [case["synth"](case["rng"].integers(0, 3, size=30)) for _ in range(3)]
    window = 12 * cpw
    on = dec.online_bigram(n_streams=3, window=window, times=True)
    on.push([2, 0], [x[2][:window], x[0][:4]])                            # exactly the window is fine
    before = on.result()
    b = hip.Batch(ctx, [x[1][:3], x[2][window:window + 1]])
    b.loglik(dec.gmm, fetch=False)
    s = on.session
    with pytest.raises(ValueError, match="stream 2"):                     # through the decoder: before the GPU is touched
        on.push([1, 2], [x[1][:3], x[2][window:window + 1]])
    with pytest.raises(hip.BackendError, match="stream 2"):               # the binding itself: stream 1 must not move either
        s.push(b, [1, 2])
    for bad in ([1, 1], [3], [-1]):
        with pytest.raises(hip.BackendError):
            s.commit(bad)
        with pytest.raises(ValueError):
            on.commit(bad)
    with pytest.raises(hip.BackendError):
        s.tail([3])
    assert s.frames().tolist() == [4, 0, window] == on.frames.tolist()
    after = on.result()
    assert after[0] == before[0]
    np.testing.assert_array_equal(after[1]["end_cost"], before[1]["end_cost"])
    np.testing.assert_array_equal(after[1]["best_end"], before[1]["best_end"])
    with pytest.raises(ValueError):
        on.result([2], want_path=True)
    with pytest.raises(hip.Unsupported, match="tail"):
        s.result([2])
    for kw in (dict(), dict(max_frames=10, window=10), dict(settle=True)):
        with pytest.raises(ValueError):
            dec.online_bigram(3, **kw)
    with pytest.raises(ValueError):
        hip.OnlineBigramSession(ctx, dec.lat, 3)
    # a commit moves the window on; reset clears anchor and words, and the id then decodes a fresh utterance
    new = on.commit([2])
    words, frames = on.settled([2])
    assert words == new and frames[0] > 0 and len(words[0]) >= 1 and len(on.settled_times([2])[0]) == len(words[0])
    on.push([2], [x[2][window:window + int(frames[0])]])
    assert on.frames[2] == window + frames[0]
    on.reset([2])
    assert on.settled([2])[0] == [[]] and on.settled([2])[1].tolist() == [0] and on.frames[2] == 0
    fresh = x[1]
    for t in range(0, len(fresh), cpw + 1):
        on.push([2], [fresh[t:t + cpw + 1]])
        on.commit([2])
    assert on.frames[2] == len(fresh) > 3 * window
    assert on.finish([2])[0] == dec.decode([fresh])
    on.close()
    b.close()
    # a full-history session that settles still gives paths; the default one still refuses commit and tail
    row_word = np.where(dec.row_state >= 0, dec.row_state // 5, -1).astype(np.int32)
    st = hip.OnlineBigramSession(ctx, dec.lat, 2, 40, settle=True)
    assert st.settles and st.window is None and st.max_frames == 40
    st.close()
    plain = hip.OnlineBigramSession(ctx, dec.lat, 2, 40)
    assert not plain.settles
    for call in (plain.commit, plain.tail):
        with pytest.raises(hip.Unsupported):
            call([0], row_label=row_word)
    for call in (hip.OnlineSession.commit, hip.OnlineSession.tail):
        with pytest.raises(hip.BackendError, match="bigram"):
            call(plain, [0], row_label=row_word)
    plain.close()
    # graph forms: what gh_online_create_bigram refuses, gh_online_create_bigram_settle refuses
    from sr.recognition.continuous_speech import packed_loop_lattice
    lat = hip.Lattices(ctx, [packed_loop_lattice(case["trans"], 5, 0.0)[0]])
    for kw in (dict(max_frames=10, settle=True), dict(window=10)):
        with pytest.raises(hip.Unsupported):
            hip.OnlineBigramSession(ctx, lat, 4, **kw)
    lat.close()


def test_push_recording_through_a_windowed_bigram_decoder(hip, ctx, audio_model):
    """tests/test_gpu_online_bigram.py's recordings through `online_bigram(window=)`: a commit after every tick, and the
    utterances equal offline trim_ranges + decode_batch -- ranges, words and word begins."""
    import sr.audio_capture as AC
    import stream_endpoints_ref as S
    from sr.feature import StreamingFrontend, feature_stats, features_from_signals
    rng = np.random.default_rng(17)
    rate = 16000
    lens = [42000, 43333, 45000, 46111, 48000, 36000]
    six = [S.burst_signal(rng, k, 40, [(4000, 10000), (24000, 30000)], freq=300.0 + 150 * i, rate=rate) for i, k in enumerate(lens)]
    six[5] = S.burst_signal(rng, lens[5], 40, [(4000, 10000), (24000, 36000)], rate=rate)        # speech up to the end
    sigs = [six[0], six[5]]
    norm = feature_stats(sigs, rate)
    dec = audio_model
    cfg = AC.default_config(rate)
    det = AC.detect_endpoints(sigs, dict(cfg), max_segments=8)
    begin, stop = AC.trim_ranges(det, [len(x) for x in sigs], dict(cfg))
    offline, longest = [[], []], 0
    for r, bg, e in zip(np.repeat(np.arange(2), det["n_segments"]), begin, stop):
        batch = features_from_signals([sigs[r][bg:e]], rate, normalize=norm)
        words, info = dec.decode_batch(batch, want_times=True)
        offline[r].append((int(bg), int(e), bool(det["open"][r]) and len(offline[r]) == 1, words[0], [int(v) for v in info["begins"][0]]))
        longest = max(longest, int(batch.lengths[0]))
        batch.close()
    ep = AC.StreamingEndpointer(2, cfg, max_chunk=TICK)
    fe = StreamingFrontend(2, rate, normalize=norm, max_chunk=ep.max_piece)
    on = dec.online_bigram(2, window=-(-longest // 3) * 3, frontend=fe, endpointer=ep, times=True)
    got, settled_mid = [[], []], 0
    for ids, chunks, end in ticks_of(sigs):
        for u in on.push_recording(ids, chunks, end):
            got[u["stream"]].append(u)
        settled_mid += int(on.settled()[1].sum() > 0)
    for r in range(2):
        assert [(u["begin"], u["stop"], u["open"], u["words"], u["begins"]) for u in got[r]] == offline[r], r
        assert all(len(u["words"]) >= 1 for u in got[r])
    assert settled_mid >= 1                                               # frames were settled while an utterance was open
    assert on.frames.tolist() == [0, 0]
    on.close(); fe.close(); ep.close()
