# -*- coding: utf-8 -*-
"""The forced commit on the device: gh_online_force (csrc/gh_online_force.hip) and `online(..., max_tail=M)`.

Every case feeds tiny models (D = 3, 2 mixtures) and at most 100 frames per stream, and compares AT EVERY TICK with the
restatement (tests/online_force_ref.py) fed with the device's own likelihood matrix and the same chunks: the settled
words, settled_frames, the `pruned` counts and the end costs with assert_array_equal (+inf where pruned), the words and
begins of the tail, and that `result` gives the same words before and after the forcing of the same tick.

  1. every instantiated N x skip, both dtypes; 1, 3 and 16 words; 1, 4, 5 and 9 streams (partly filled four-stream waves),
     ragged lengths, a window of M + 9 (M + 9 >= the frames a stream needs before a word end is reachable: while the
     chosen end is +inf nothing can be forced, so the FIRST chunk of a stream carries those frames);
  1b. one-frame ticks: the forced column c* = T - 1 - M takes every position inside a decision word, and cells are pruned
     at every one of them (asserted), for every count of columns per word from 8 to 1;
  2. a ring of W = M + 9 that wraps at least eight times;
  3. a stuck stream (word_penalty = 50): the unforced restatement's tail exceeds the window, the session without
     `max_tail` raises the window ValueError as ever, the one with it runs to the end with tail <= M after every commit;
  4. `max_tail` larger than every natural tail: bitwise a session without it, `n_forced` all zero;
  5. a stream with one frame and a stream whose chosen end is +inf: untouched;
  6. a reused stream id against a fresh session;
  7. `push_recording` with a window and `max_tail`;
  8. `max_frames=` + `max_tail`: `result(want_path=True)` passes the anchor cell;
  9. refusals through the real library: bad arguments, and the other four session forms."""
import numpy as np
import pytest

from online_force_ref import chosen_end, force
from online_ref import CarriedDecode
from online_settle_ref import SettledDecode
from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu

M_, D_ = 2, 3
CHUNKS = (1, 2, 3, 4, 5, 6, 7, 8, 9)
#         W   n  skip   U  M
CASES = [(1, 2, False, 1, 1),
         (3, 3, False, 4, 4),
         (16, 3, True, 5, 7),
         (16, 4, False, 9, 1),
         (3, 4, True, 4, 4),
         (3, 5, False, 5, 7),
         (1, 5, True, 9, 1),
         (16, 6, False, 1, 4),
         (3, 6, True, 4, 7),
         (1, 7, False, 5, 1),
         (16, 7, True, 9, 4),
         (3, 8, False, 1, 7),
         (16, 8, True, 4, 1),
         (3, 12, False, 5, 4),
         (1, 12, True, 9, 7),
         (3, 16, False, 4, 7),
         (2, 16, True, 5, 4)]
CASE_IDS = ["W%d-n%d-%s-U%d-M%d" % (c[0], c[1], "skip" if c[2] else "plain", c[3], c[4]) for c in CASES]


def cpw_of(n, skip):
    return 32 // (n + 2 + (n - 2 if skip else 0))


def frames_to_an_end(n, skip):
    """Frames a stream needs before the last state of a word is reachable: its chosen end is +inf before."""
    return (n - 1 + 1) // 2 + 1 if skip else n


def word_trans(rng, n, skip):
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = rng.uniform(0.1, 2.0)
        if i < n - 1:
            t[i + 1, i] = rng.uniform(0.1, 2.0)
        if skip and i < n - 2:
            t[i + 2, i] = rng.uniform(0.1, 2.0)
    return t


def make_case(W, n, skip, U, M, penalty=50.0, T_max=100, seed=0):
    rng = np.random.default_rng(4000 + 100 * W + 10 * n + skip + seed)
    means = rng.normal(size=(W, n, M_, D_)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M_, D_))
    w = rng.dirichlet(np.ones(M_), size=(W, n))
    trans = [word_trans(rng, n, skip) for _ in range(W)]
    T = [T_max - 9 * u for u in range(U)]                                 # ragged: 100, 91, ... (9 streams: down to 28)
    xs = [rng.normal(size=(t, D_)) * 2.0 for t in T]
    nes, rw, rs, dense, ends = O.loop_grammar(trans, n, penalty)
    ids = rng.permutation(U + 3)[:U]                                      # scattered over a larger session
    return dict(W=W, n=n, skip=skip, U=U, M=M, penalty=penalty, means=means, vars=vars_, w=w, trans=trans, xs=xs, T=np.array(T),
                nes=nes, rw=rw, rs=rs, dense=dense, ends=ends, ids=ids, rng=rng)


def schedule(case, chunks=CHUNKS):
    """Ticks of frame counts [U]: chunk lengths 1 .. 9, a different phase per stream; the first chunk of a stream holds
    the frames it needs before a word end is reachable."""
    T, U = case["T"], case["U"]
    need = frames_to_an_end(case["n"], case["skip"])
    pos, out, k = np.zeros(U, dtype=np.int64), [], 0
    while np.any(pos < T):
        cnt = np.array([chunks[(k + 2 * u) % len(chunks)] for u in range(U)])
        cnt = np.where(pos == 0, np.maximum(cnt, need), cnt)
        cnt = np.minimum(cnt, T - pos)
        out.append(cnt)
        pos = pos + cnt
        k += 1
    return out


def emissions(case, nll):
    col = np.where(case["nes"], 0, case["rw"] * case["n"] + case["rs"])
    return np.where(case["nes"][:, None], 0.0, np.asarray(nll, dtype=np.float64)[:, col].T)


def restate(case, E, chunks, M, row_state):
    """The restatement of one stream: per tick a dict of everything the device is compared with."""
    from sr.recognition.batch import path_to_word_times
    cd = CarriedDecode(case["nes"], case["dense"], case["ends"])
    sd = SettledDecode(cd, case["rw"])
    t, out, begins = 0, [], []
    for c in chunks:
        cd.push(E[:, t:t + c])
        t += int(c)
        before = path_to_word_times(cd.result()[2], row_state, case["n"])
        finite = bool(np.isfinite(chosen_end(cd)[1]))
        n_before = len(sd.words)
        c_star = None
        if M is None:
            new, pruned = sd.commit(), 0
        else:
            new = sd.commit()
            pruned = 0
            if cd.t - sd.settled_frames > M:
                f = force(cd, sd, M)
                pruned, c_star = f["pruned"], None if f["cell"] is None else f["cell"][0]
                new = new + sd.commit()
        after = path_to_word_times(cd.result()[2], row_state, case["n"])
        if finite:
            assert after == before                                         # the chosen end survives
        out.append(dict(frames=cd.t, settled=sd.settled_frames, words=list(sd.words), new=new, pruned=pruned, finite=finite,
                        end_cost=cd.col[case["ends"]].copy(), result=after, c_star=c_star, anchor=sd.anchor))
    return out


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
    from test_gpu_online_settle import make_hmm
    hmms = [make_hmm(R, case["means"][i], case["vars"][i], case["w"][i], case["trans"][i]) for i in range(case["W"])]
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=case["penalty"], dtype=dtype, ctx=ctx)
    np.testing.assert_array_equal(dec.row_state, np.where(case["nes"], -1, case["rw"] * case["n"] + case["rs"]))
    assert list(dec.lat.end_rows[0]) == list(case["ends"])
    return dec


def spy_on_force(on):
    """Records what `session.force` returned: {stream: pruned} of the last commit."""
    seen = {}
    inner = on.session.force

    def force_(ids=None, max_tail=1):
        pruned = inner(ids, max_tail)
        seen.update({int(k): int(p) for k, p in zip(ids, pruned)})
        return pruned
    on.session.force = force_
    return seen


def run_against_restatement(hip, dec, case, on, sched, M, dtype=np.float64):
    """Feeds the case's streams to `on` by `sched` with a commit after every push and compares every tick with the
    restatement.  Returns the restatement's ticks per stream."""
    U, ids, xs = case["U"], case["ids"], case["xs"]
    b = hip.Batch(dec.ctx, xs, dtype=dtype)
    nll = b.loglik(dec.gmm, fetch=True)                                   # the matrix both sides decode
    off = np.concatenate([[0], np.cumsum(case["T"])])
    ref = [restate(case, emissions(case, nll[off[u]:off[u + 1]]), [int(c[u]) for c in sched], M, dec.row_state) for u in range(U)]
    seen = spy_on_force(on) if M is not None else {}
    pos = np.zeros(U, dtype=np.int64)
    n_forced = np.zeros(U, dtype=np.int64)
    for k, cnt in enumerate(sched):
        on.push_batch(ids, b, first=pos, count=cnt)                       # never refused for the window
        pos = pos + cnt
        before, info_b = on.result(ids)
        seen.clear()
        new, new_begins = on.commit(ids, want_times=True)
        words, frames = on.settled(ids)
        after, info = on.result(ids)
        times = on.settled_times(ids)
        np.testing.assert_array_equal(frames, [ref[u][k]["settled"] for u in range(U)])
        np.testing.assert_array_equal(info["end_cost"], np.array([ref[u][k]["end_cost"] for u in range(U)]))
        np.testing.assert_array_equal(info["frames"], [ref[u][k]["frames"] for u in range(U)])
        for u in range(U):
            r = ref[u][k]
            assert new[u] == r["new"] and words[u] == r["words"], (k, u)
            assert seen.get(int(ids[u]), 0) == r["pruned"], (k, u)
            n_forced[u] += r["pruned"] > 0
            assert len(new_begins[u]) == len(new[u]) and len(times[u]) == len(words[u])
            if r["finite"]:
                assert after[u] == before[u] == r["result"][0], (k, u)
                assert [int(v) for v in info["begins"][u]] == r["result"][1], (k, u)
                assert times[u] == r["result"][1][:len(times[u])]
                if M is not None:
                    assert r["frames"] - frames[u] <= M
        np.testing.assert_array_equal(on.n_forced[ids], n_forced)
    assert np.all(pos == case["T"])
    b.close()
    return ref


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", CASES, ids=CASE_IDS)
def test_every_instantiation_against_the_restatement(R, hip, ctx, shape, dtype):
    case = make_case(*shape)
    M, n, skip = case["M"], case["n"], case["skip"]
    window = M + 9
    assert frames_to_an_end(n, skip) <= window
    dec = decoder_of(R, ctx, case, dtype)
    on = dec.online(case["U"] + 3, window=window, max_tail=M, times=True)
    ref = run_against_restatement(hip, dec, case, on, schedule(case), M, dtype)
    on.close()
    forced = [t for r in ref for t in r if t["c_star"] is not None]
    assert sum(t["pruned"] > 0 for t in forced) >= 3                      # not vacuous: cells were pruned


@pytest.mark.parametrize("shape", [(3, 2, False, 5, 3), (3, 3, False, 1, 2), (16, 3, True, 4, 5), (3, 5, False, 5, 1), (2, 7, False, 1, 4),
                                   (3, 8, True, 4, 2), (2, 16, False, 1, 3)], ids=lambda c: "W%d-n%d-%s-U%d-M%d" % (c[0], c[1], "skip" if c[2] else "plain", c[3], c[4]))
def test_the_forced_column_at_every_position_inside_a_decision_word(R, hip, ctx, shape):
    case = make_case(*shape, T_max=60, seed=2)
    M, n, skip = case["M"], case["n"], case["skip"]
    cpw = cpw_of(n, skip)
    dec = decoder_of(R, ctx, case)
    on = dec.online(case["U"] + 3, window=max(M + 2, frames_to_an_end(n, skip)), max_tail=M, times=True)
    ref = run_against_restatement(hip, dec, case, on, schedule(case, chunks=(1, 1, 2)), M)
    on.close()
    assert {t["c_star"] % cpw for r in ref for t in r if t["pruned"] > 0} == set(range(cpw))


@pytest.mark.parametrize("shape", [(16, 8, True, 4, 1), (2, 16, True, 4, 1)], ids=["n8-skip", "n16-skip"])
def test_the_ring_wraps_eight_times(R, hip, ctx, shape):
    W, n, skip, U, M = shape
    case = make_case(W, n, skip, U, M, seed=1)
    case["T"][:] = case["T"][0]
    case["xs"] = [np.concatenate([x, x])[:case["T"][0]] for x in case["xs"]]
    window = M + 9
    ring_frames = (-(-window // cpw_of(n, skip)) + 1) * cpw_of(n, skip)
    assert case["T"].min() >= 8 * ring_frames
    dec = decoder_of(R, ctx, case)
    on = dec.online(U + 3, window=window, max_tail=M, times=True)
    run_against_restatement(hip, dec, case, on, schedule(case), M)
    assert on.n_forced.sum() >= 8
    on.close()


def test_a_stuck_stream_wedges_without_max_tail_and_runs_with_it(R, hip, ctx):
    case = make_case(5, 5, False, 4, 6)
    M, window = 6, 20
    dec = decoder_of(R, ctx, case)
    sched = schedule(case)
    # on the CPU first: unforced, the tail of every stream outgrows the window (the device's own likelihoods)
    b = hip.Batch(ctx, case["xs"], dtype=np.float64)
    nll = b.loglik(dec.gmm, fetch=True)
    b.close()
    off = np.concatenate([[0], np.cumsum(case["T"])])
    for u in range(case["U"]):
        natural = restate(case, emissions(case, nll[off[u]:off[u + 1]]), [int(c[u]) for c in sched], None, dec.row_state)
        assert max(t["frames"] - t["settled"] for t in natural) > window
    plain = dec.online(case["U"] + 3, window=window)
    with pytest.raises(ValueError, match="window"):
        for x in [case["xs"][0][t:t + 5] for t in range(0, 100, 5)]:
            plain.push([2], [x])
            plain.commit([2])
    assert plain.n_forced.tolist() == [0] * (case["U"] + 3)
    plain.close()
    on = dec.online(case["U"] + 3, window=window, max_tail=M, times=True)
    ref = run_against_restatement(hip, dec, case, on, sched, M)           # to the end, tail <= M after every commit
    assert all(sum(t["pruned"] > 0 for t in r) >= 5 for r in ref)
    on.close()


def test_a_bound_above_every_natural_tail_changes_nothing(R, hip, ctx):
    case = make_case(4, 3, True, 5, 60, penalty=0.0)
    dec = decoder_of(R, ctx, case)
    sched = schedule(case)
    T = int(case["T"].max())
    plain = dec.online(case["U"] + 3, max_frames=T, times=True)
    on = dec.online(case["U"] + 3, max_frames=T, max_tail=60, times=True)
    ref = run_against_restatement(hip, dec, case, on, sched, 60)
    assert max(t["frames"] - t["settled"] for r in ref for t in r) < 60 and sum(t["settled"] > 0 for r in ref for t in r) > 20
    run_against_restatement(hip, dec, case, plain, sched, None)
    assert not on.n_forced.any()
    a, ia = on.result(case["ids"], want_path=True)
    p, ip = plain.result(case["ids"], want_path=True)
    assert a == p and on.settled(case["ids"])[0] == plain.settled(case["ids"])[0]
    np.testing.assert_array_equal(ia["end_cost"], ip["end_cost"])
    np.testing.assert_array_equal(ia["best_end"], ip["best_end"])
    for x, y in zip(ia["paths"], ip["paths"]):
        np.testing.assert_array_equal(x, y)
    on.close()
    plain.close()


def test_one_frame_and_a_dead_end_are_untouched(R, hip, ctx):
    case = make_case(3, 5, False, 3, 1)
    dec = decoder_of(R, ctx, case)
    on = dec.online(4, window=10, max_tail=1)
    on.push([0, 1, 3], [case["xs"][0][:1], case["xs"][1][:3], case["xs"][2][:8]])     # one frame; no word end reachable; alive
    before = on.result()
    assert np.all(np.isinf(before[1]["end_cost"][:3])) and np.all(np.isfinite(before[1]["end_cost"][3]))
    s = on.session
    pruned = s.force([0, 1, 2, 3], 1)
    assert pruned[:3].tolist() == [0, 0, 0] and pruned[3] > 0
    after = on.result()
    assert after[0] == before[0]
    np.testing.assert_array_equal(after[1]["end_cost"][:3], before[1]["end_cost"][:3])
    assert np.isinf(after[1]["end_cost"][3]).sum() >= np.isinf(before[1]["end_cost"][3]).sum()
    assert s.force(None, 1).tolist() == [0, 0, 0, 0]                      # forcing twice prunes nothing more
    assert on.commit() is not None and on.n_forced.tolist() == [0, 0, 0, 0]   # (the decoder's own commit found nothing to force)
    assert on.frames[3] - on.settled([3])[1][0] <= 1
    on.close()


def test_a_reused_stream_id_equals_a_fresh_session(R, hip, ctx):
    case = make_case(5, 4, True, 2, 3)
    M, window = 3, 12
    dec = decoder_of(R, ctx, case)
    xa, xb = case["xs"][0][:60], case["xs"][1][:70]

    def feed(on, k, x):
        out = []
        for t in range(0, len(x), 7):
            on.push([k], [x[t:t + 7]])
            new = on.commit([k])
            words, info = on.result([k])
            out.append((new, words, on.settled([k])[1].tolist(), info["end_cost"].copy(), int(on.n_forced[k])))
        return out

    used = dec.online(3, window=window, max_tail=M)
    feed(used, 1, xa)
    assert used.n_forced[1] > 0
    used.finish([1])
    assert used.n_forced[1] == 0 and used.frames[1] == 0
    fresh = dec.online(3, window=window, max_tail=M)
    for g, w in zip(feed(used, 1, xb), feed(fresh, 1, xb)):
        assert g[:3] == w[:3] and g[4] == w[4]
        np.testing.assert_array_equal(g[3], w[3])
    assert used.n_forced[1] > 0
    used.close()
    fresh.close()


def test_full_history_with_max_tail_the_path_passes_the_anchor(R, hip, ctx):
    case = make_case(4, 4, False, 4, 5)
    M = 5
    dec = decoder_of(R, ctx, case)
    on = dec.online(case["U"] + 3, max_frames=int(case["T"].max()), max_tail=M, times=True)
    ref = run_against_restatement(hip, dec, case, on, schedule(case), M)
    words, info = on.result(case["ids"], want_path=True)
    for u in range(case["U"]):
        last = ref[u][-1]
        col, row = last["anchor"]
        assert last["frames"] - 1 - col <= M and last["pruned"] >= 0
        path = info["paths"][u]
        in_col = path[path[:, 1] == col]
        assert in_col[0, 0] == row                                        # the path arrives in the anchor cell
        assert words[u] == last["result"][0]
    assert on.n_forced.sum() >= 8
    on.close()


def test_push_recording_with_a_window_and_max_tail(R, hip, ctx):
    """Two recordings of two bursts each through `push_recording` with a window far shorter than an utterance: without
    `max_tail` the decoder refuses a piece; with it every utterance comes out, with the unforced decoder's ranges, the tail
    is bounded after every tick, and utterances were forced on the way."""
    import sr.audio_capture as AC
    import stream_endpoints_ref as S
    from sr.feature import StreamingFrontend, feature_stats
    from sr.recognition.batch import ContinuousDecoder
    from test_gpu_online_settle import make_hmm
    rng = np.random.default_rng(17)
    rate, TICK = 16000, 3200
    sigs = [S.burst_signal(rng, k, 40, [(4000, 20000), (30000, 42000)], freq=300.0 + 150 * i, rate=rate) for i, k in enumerate([46000, 48000])]
    norm = feature_stats(sigs, rate)
    W, n, d = 3, 4, 39
    trans = word_trans(rng, n, False)
    hmms = [make_hmm(R, rng.normal(size=(n, M_, d)), rng.uniform(0.5, 1.5, size=(n, M_, d)), rng.dirichlet(np.ones(M_), size=n), trans)
            for _ in range(W)]
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=50.0, ctx=ctx)
    cfg = AC.default_config(rate)

    def run(**kw):
        ep = AC.StreamingEndpointer(2, cfg, max_chunk=TICK)
        fe = StreamingFrontend(2, rate, normalize=norm, max_chunk=ep.max_piece)
        on = dec.online(2, frontend=fe, endpointer=ep, times=True, **kw)
        got, forced, tails = [], 0, []
        try:
            for t in range(-(-48000 // TICK)):
                live = [k for k in range(2) if t * TICK < len(sigs[k])]
                got += on.push_recording(live, [sigs[k][t * TICK:(t + 1) * TICK] for k in live], [(t + 1) * TICK >= len(sigs[k]) for k in live])
                forced = max(forced, int(on.n_forced.sum()))
                tails.append(int((on.frames - on.settled()[1]).max()))
        finally:
            on.close(); fe.close(); ep.close()
        return got, forced, tails

    probe = AC.StreamingEndpointer(2, cfg, max_chunk=TICK)
    M = 10
    window = M + probe.max_piece // 160 + 4                               # room for the largest piece the gate hands out
    probe.close()
    full, _, natural = run(window=400)
    assert len(full) >= 2 and max(natural) > window                       # utterances whose tails outgrow the window
    with pytest.raises(ValueError, match="reset these streams"):
        run(window=window)
    got, forced, tails = run(window=window, max_tail=M)
    assert [(u["stream"], u["begin"], u["stop"], u["open"]) for u in got] == [(u["stream"], u["begin"], u["stop"], u["open"]) for u in full]
    assert all(len(u["words"]) >= 1 and len(u["begins"]) == len(u["words"]) for u in got)
    assert forced >= 1 and max(tails) <= M


def test_refusals_through_the_library(R, hip, ctx):
    from sr.recognition.continuous_speech import packed_bigram_lattice, packed_lattice, packed_loop_lattice
    case = make_case(3, 3, False, 2, 2)
    dec = decoder_of(R, ctx, case)
    on = dec.online(3, window=12, max_tail=2)
    on.push([0, 2], [case["xs"][0][:10], case["xs"][1][:10]])
    s = on.session
    before = on.result()
    for ids, m in (([0], 0), ([0], -1), ([0, 0], 2), ([3], 2), ([-1], 2)):
        with pytest.raises(hip.BackendError):
            s.force(ids, m)
    after = on.result()
    assert after[0] == before[0]
    np.testing.assert_array_equal(after[1]["end_cost"], before[1]["end_cost"])        # a refused call has pruned nothing
    assert s.force([], 2).tolist() == []
    for kw in (dict(window=12, max_tail=0), dict(window=12, max_tail=12), dict(max_frames=12, max_tail=-1)):
        with pytest.raises(ValueError, match="max_tail"):
            dec.online(3, **kw)
    on.close()
    # the other four session forms: each refused with a sentence of its own
    rng = np.random.default_rng(3)
    wt4, wt17 = [word_trans(rng, 3, False) for _ in range(4)], [word_trans(rng, 3, False) for _ in range(17)]
    said = []
    for cls, graph, kw in ((hip.OnlineBigramSession, packed_bigram_lattice(wt4, 3, rng.uniform(0.5, 3.0, size=(4, 4)), None)[0], dict(window=10)),
                           (hip.OnlineWideSession, packed_loop_lattice(wt17, 3, 0.0)[0], dict(window=10)),
                           (hip.OnlineBigramWideSession, packed_bigram_lattice(wt17, 3, rng.uniform(0.5, 3.0, size=(17, 17)), None)[0], dict(window=10)),
                           (hip.OnlineLayersSession, packed_lattice(wt4, 3, [list(range(4))] * 2)[0], dict(max_frames=10))):
        lat = hip.Lattices(ctx, [graph])
        sess = cls(ctx, lat, 2, **kw)
        with pytest.raises(hip.Unsupported, match="not built yet") as e:
            hip.OnlineSession.force(sess, [0], 2)
        said.append(str(e.value))
        sess.close()
        lat.close()
    assert len(set(said)) == 4
