# -*- coding: utf-8 -*-
"""The settled prefix of an online decode on the device (gh_online_settle.hip: gh_online_commit, gh_online_tail,
gh_online_create_window) and the ring-addressed history of gh_viterbi_online.hip.

L_k: the one-shot labels of the first k frames of a stream; C: the settled words after a commit.
  4. prefix stability, device against device: after every push, commit; C is a prefix of L_k of the same prefix now and of
     the final decode, and commits only ever extend;
  5. anchors are exact and maximal: settled_frames and C equal the restatement's (tests/online_settle_ref.py) on the batch's
     own fp64 likelihood matrix with the same chunking, for every stream at every tick;
  6. windowed == full history: the same pushes to a window= and a max_frames= session, both committing every tick: end
     costs and chosen ends bitwise equal, words equal, over streams at least 3 x the window long (the ring has wrapped);
  7. refusals through the real library;
  8. configs[4]'s model end to end through `push`, 40 streams in 20-frame ticks.
Streams whose end costs are all +inf are outside the stability contract (include/gmmhmm.h): where the chosen end of a
stream is +inf its one-shot labels come from a back-trace over dead cells, and (4) and the words of (6) leave that
stream out AT THAT TICK; its anchor, its settled words (5) and its end costs (6) are compared all the same.
Shapes: the smallest that reach every code path, from NARROW in test_gpu_online.py."""
import numpy as np
import pytest

from online_ref import CarriedDecode
from online_settle_ref import SettledDecode
from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu

#          W   n  skip   penalty
SHAPES = [(1, 2, False, 0.0),     # one word, widest CPW
          (16, 3, True, 1.0),     # all lanes, skip bits
          (10, 5, False, 0.0),    # configs[4]'s form
          (5, 8, True, 0.0),
          (4, 12, False, 0.5),    # N > 8
          (2, 16, True, 2.0)]
U, N_IDS, M, D = 13, 17, 2, 6
assert U % 4 != 0


def word_trans(rng, n, skip=False, last_self=0.0):
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = rng.uniform(0.05, 0.6) if i < n - 1 else last_self
        if i < n - 1:
            t[i + 1, i] = rng.uniform(0.8, 2.5)
        if skip and i < n - 2 and rng.random() < 0.6:
            t[i + 2, i] = rng.uniform(1.5, 4.0)
    return t


def cpw_of(n, skip):
    return 32 // (n + 2 + (n - 2 if skip else 0))


def make_case(W, n, skip, penalty):
    """Model, 13 utterances of 1 - 7 synthetic words (two shorter than a word) as test_gpu_online.py builds them, 13 long
    streams (those utterances one after the other, cut at 110 + 7 n frames and a few) and the stream ids, scattered over 17.  No GPU."""
    rng = np.random.default_rng(1300 + 77 * W + n)
    means = rng.normal(size=(W, n, M, D)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M, D))
    w = rng.dirichlet(np.ones(M), size=(W, n))
    trans = [word_trans(rng, n, skip, last_self=rng.uniform(0.0, 0.3)) for _ in range(W)]
    xs, n_words = [], []
    for u in range(U):
        if u % 9 == 0:
            xs.append(rng.normal(size=(int(rng.integers(2, max(3, n))), D)) * 2.0)      # shorter than any word
            n_words.append(0)
            continue
        segs = []
        words = rng.integers(0, W, size=rng.integers(1, 8))
        for wd in words:
            Tw = int(rng.integers(n, 3 * n + 4))
            st = np.minimum(np.arange(Tw) * n // Tw, n - 1)
            comp = rng.integers(0, M, size=Tw)
            segs.append(means[wd, st, comp] + np.sqrt(vars_[wd, st, comp]) * rng.normal(size=(Tw, D)))
        xs.append(np.concatenate(segs))
        n_words.append(len(words))
    long_xs = [np.concatenate([xs[(u + k) % U] for k in range(1, U)])[:110 + 7 * n + u] for u in range(U)]
    ids = rng.permutation(N_IDS)[:U]
    nes, rw, rs, T_, ends = O.loop_grammar(trans, n, penalty)
    return dict(W=W, n=n, skip=skip, penalty=penalty, means=means, vars=vars_, w=w, trans=trans, xs=xs, n_words=n_words,
                long_xs=long_xs, ids=ids, nes=nes, rw=rw, rs=rs, dense=T_, ends=ends, rng=rng)


def schedule(rng, T, choices):
    """Ticks of column counts [U] that feed utterances of T [U] frames: 0- and 1-frame pushes, ranges that end inside a
    decision word."""
    pos, out = np.zeros(len(T), dtype=np.int64), []
    while np.any(pos < T):
        cnt = np.minimum(rng.choice(choices, size=len(T)), T - pos)
        out.append(cnt)
        pos = pos + cnt
    return out


def restate(case, E, chunks):
    """The restatement on the emission matrix E [R, T] of one stream fed in `chunks`: per tick (settled_frames, settled
    words, unsettled frames the history held before the commit)."""
    cd = CarriedDecode(case["nes"], case["dense"], case["ends"])
    sd = SettledDecode(cd, case["rw"])
    t, out = 0, []
    for c in chunks:
        cd.push(E[:, t:t + c])
        t += int(c)
        tail = t - sd.settled_frames
        sd.commit()
        out.append((sd.settled_frames, list(sd.words), tail))
    return out


def emissions(case, nll):
    """E [R, T] of the restatement from the rows [T, S] of a likelihood matrix (state of word w, local state s: w n + s)."""
    col = np.where(case["nes"], 0, case["rw"] * case["n"] + case["rs"])
    return np.where(case["nes"][:, None], 0.0, np.asarray(nll, dtype=np.float64)[:, col].T)


def window_of(case, ticks_per_stream):
    """The restatement's largest unsettled tail, rounded up to a decision word."""
    cpw = cpw_of(case["n"], case["skip"])
    tail = max(t[2] for ticks in ticks_per_stream for t in ticks)
    return -(-tail // cpw) * cpw


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


def make_hmm(R, means, vars_, w, trans):
    h = R.HMM(means.shape[0])
    h.gmm_states = []
    for s in range(means.shape[0]):
        g = R.GMM(means[s, 0].copy(), vars_[s, 0].copy(), means.shape[1])
        g.update_models(means[s].copy(), vars_[s].copy(), w[s].copy())
        h.gmm_states.append(g)
    h.transitions = trans.copy()
    h.mu, h.sigma = means[:, 0].copy(), vars_[:, 0].copy()
    return h


def decoder_of(R, ctx, case, dtype=np.float64):
    from sr.recognition.batch import ContinuousDecoder
    hmms = [make_hmm(R, case["means"][i], case["vars"][i], case["w"][i], case["trans"][i]) for i in range(case["W"])]
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=case["penalty"], dtype=dtype, ctx=ctx)
    assert "loop" in dec.lat.forms()
    np.testing.assert_array_equal(dec.row_state, np.where(case["nes"], -1, case["rw"] * case["n"] + case["rs"]))
    assert list(dec.lat.end_rows[0]) == list(case["ends"])
    return dec


def finite_end(info):
    """Per stream: its chosen end is a live cell (the stability contract covers the stream at this tick)."""
    be = info["best_end"]
    return np.array([b >= 0 and np.isfinite(info["end_cost"][i, b]) for i, b in enumerate(be)])


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "W%d-n%d-%s" % (s[0], s[1], "skip" if s[2] else "plain"))
def committed(request, R, hip, ctx):
    """One full-history session per shape, fed its 13 utterances in random column ranges with a commit after every push:
    what the device said at every tick, the one-shot decodes of the same prefixes, and the restatement on the same
    likelihood matrix.  Computed once, shared by (4) and (5)."""
    case = make_case(*request.param)
    dec = decoder_of(R, ctx, case)
    rng = case["rng"]
    xs, ids = case["xs"], case["ids"]
    b = hip.Batch(ctx, xs, dtype=np.float64)
    nll = b.loglik(dec.gmm, fetch=True)                                  # the matrix both sides decode
    T = np.asarray(b.lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(T)])
    sched = schedule(rng, T, [0, 1, 1, 2, 3, 5, 8, 13, 21])
    on = dec.online(n_streams=N_IDS, max_frames=int(T.max()))
    row_word = np.where(dec.row_state >= 0, dec.row_state // case["n"], -1).astype(np.int32)
    pos = np.zeros(U, dtype=np.int64)
    ticks = []
    for cnt in sched:
        on.push_batch(ids, b, first=pos, count=cnt)
        pos = pos + cnt
        new = on.commit(ids)
        words, frames = on.settled(ids)
        res_words, info = on.result(ids)
        some = np.flatnonzero(pos > 0)
        one_shot = [None] * U
        if len(some):
            pb = hip.Batch(ctx, [xs[u][:pos[u]] for u in some], dtype=np.float64)
            pb.loglik(dec.gmm, fetch=False)
            lab = dec.lat.viterbi_labels(pb, row_word)
            for u, l in zip(some, lab["labels"]):
                one_shot[u] = [int(v) for v in l]
            pb.close()
        ticks.append(dict(pos=pos.copy(), new=new, words=words, frames=frames, result=res_words, one_shot=one_shot,
                          finite=finite_end(info)))
    final = [[int(v) for v in l] for l in dec.lat.viterbi_labels(b, row_word)["labels"]]
    assert on.result(ids)[0] == final
    ref = [restate(case, emissions(case, nll[off[u]:off[u + 1]]), [int(c[u]) for c in sched]) for u in range(U)]
    on.close()
    b.close()
    return dict(case=case, ticks=ticks, final=final, ref=ref, sched=sched, T=T)


def test_prefix_stability_device_against_device(committed):
    ticks, final = committed["ticks"], committed["final"]
    before = [[] for _ in range(U)]
    compared = 0
    for tk in ticks:
        for u in range(U):
            C = tk["words"][u]
            assert C == before[u] + tk["new"][u]                          # commits only ever extend
            assert tk["frames"][u] <= max(tk["pos"][u] - 1, 0)
            assert C == final[u][:len(C)]
            if tk["one_shot"][u] is not None:
                assert tk["result"][u] == tk["one_shot"][u]               # (online == one-shot on the prefix, as ever)
                if tk["finite"][u]:
                    assert C == tk["one_shot"][u][:len(C)]
                    compared += len(C) > 0
            before[u] = C
    assert compared > 0


def test_anchors_are_exact_and_maximal(committed):
    case, ticks, ref, sched = committed["case"], committed["ticks"], committed["ref"], committed["sched"]
    for k, tk in enumerate(ticks):
        for u in range(U):
            assert (int(tk["frames"][u]), tk["words"][u]) == (ref[u][k][0], ref[u][k][1]), (k, u)
    # not vacuous: at least half of the multi-word streams have an anchor before their last push
    multi = [u for u in range(U) if case["n_words"][u] >= 2]
    early = 0
    for u in multi:
        last = max(k for k, c in enumerate(sched) if c[u] > 0)
        early += any(ref[u][k][0] > 0 for k in range(last))
    assert len(multi) >= 4 and 2 * early >= len(multi)


def run_pair(hip, ctx, dec, case, dtype):
    """(6): a window= and a max_frames= session on the same pushes of the long streams."""
    rng = np.random.default_rng(5 + case["W"])
    xs, ids = case["long_xs"], case["ids"]
    b = hip.Batch(ctx, xs, dtype=dtype)
    nll = b.loglik(dec.gmm, fetch=True)
    T = np.asarray(b.lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(T)])
    sched = schedule(rng, T, [0, 1, 1, 2, 3, 5, 8, 13])
    ref = [restate(case, emissions(case, nll[off[u]:off[u + 1]]), [int(c[u]) for c in sched]) for u in range(U)]
    window = window_of(case, ref)
    assert window % cpw_of(case["n"], case["skip"]) == 0 and max(t[2] for r in ref for t in r) <= window
    assert T.min() >= 3 * window, "the streams must be at least 3 x the window long: the ring has to wrap"
    full = dec.online(n_streams=N_IDS, max_frames=int(T.max()))
    win = dec.online(n_streams=N_IDS, window=window)
    pos = np.zeros(U, dtype=np.int64)
    compared = 0
    for k, cnt in enumerate(sched):
        for on in (full, win):
            on.push_batch(ids, b, first=pos, count=cnt)
        pos = pos + cnt
        new_f, new_w = full.commit(ids), win.commit(ids)
        assert new_f == new_w
        (wf, ff), (ww, fw) = full.settled(ids), win.settled(ids)
        assert wf == ww and ff.tolist() == fw.tolist() == [ref[u][k][0] for u in range(U)]
        assert wf == [ref[u][k][1] for u in range(U)]
        rf, info_f = full.result(ids)
        rw_, info_w = win.result(ids)
        np.testing.assert_array_equal(info_w["end_cost"], info_f["end_cost"])          # bitwise
        np.testing.assert_array_equal(info_w["best_end"], info_f["best_end"])
        np.testing.assert_array_equal(info_w["frames"], info_f["frames"])
        assert sorted(info_w) == sorted(info_f)
        live = finite_end(info_f)
        for u in range(U):
            if live[u]:
                assert rw_[u] == rf[u], (k, u)
                compared += 1
    assert compared >= U * len(sched) * 3 // 4 and np.all(pos == T)
    final = full.finish(ids)[0]
    assert win.finish(ids)[0] == final and not win.frames.any() and win.settled()[0] == [[]] * N_IDS
    full.close()
    win.close()
    b.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "W%d-n%d-%s" % (s[0], s[1], "skip" if s[2] else "plain"))
def test_windowed_equals_full_history(R, hip, ctx, shape):
    case = make_case(*shape)
    run_pair(hip, ctx, decoder_of(R, ctx, case), case, np.float64)


def test_windowed_equals_full_history_fp32_likelihoods(R, hip, ctx):
    case = make_case(*SHAPES[2])
    run_pair(hip, ctx, decoder_of(R, ctx, case, dtype=np.float32), case, np.float32)


def test_refusals(R, hip, ctx):
    from sr.recognition.batch import ContinuousDecoder
    from sr.recognition.continuous_speech import packed_lattice, packed_bigram_lattice
    case = make_case(4, 3, False, 0.5)
    dec = decoder_of(R, ctx, case)
    xs, n = case["long_xs"], case["n"]
    cpw = cpw_of(n, False)
    window = 5 * cpw
    on = dec.online(n_streams=3, window=window)
    on.push([2, 0], [xs[2][:window], xs[0][:4]])                          # exactly the window is fine
    before = on.result()
    b = hip.Batch(ctx, [xs[1][:3], xs[2][window:window + 1]])
    b.loglik(dec.gmm, fetch=False)
    s = on.session
    with pytest.raises(ValueError, match="stream 2"):                     # through the decoder: before the GPU is touched
        on.push([1, 2], [xs[1][:3], xs[2][window:window + 1]])
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
    with pytest.raises(ValueError):
        dec.online(3)
    with pytest.raises(ValueError):
        dec.online(3, max_frames=10, window=10)
    # a commit moves the window on; reset clears anchor and words, and the id then decodes a fresh utterance
    new = on.commit([2])
    words, frames = on.settled([2])
    assert words == new and frames[0] > 0 and len(words[0]) >= 1
    on.push([2], [xs[2][window:window + int(frames[0])]])
    assert on.frames[2] == window + frames[0]
    on.reset([2])
    assert on.settled([2])[0] == [[]] and on.settled([2])[1].tolist() == [0] and on.frames[2] == 0
    fresh = xs[3]
    for t in range(0, len(fresh), cpw + 1):
        on.push([2], [fresh[t:t + cpw + 1]])
        on.commit([2])
    assert on.frames[2] == len(fresh) > 3 * window
    assert on.finish([2])[0] == dec.decode([fresh])
    on.close()
    b.close()
    # graph forms: what gh_online_create refuses, gh_online_create_window refuses
    wt = case["trans"]
    rng = np.random.default_rng(3)
    for graph in (packed_lattice(wt, n, [list(range(4))] * 3)[0],
                  packed_bigram_lattice(wt, n, rng.uniform(0.5, 3.0, size=(4, 4)), None)[0]):
        lat = hip.Lattices(ctx, [graph])
        with pytest.raises(hip.Unsupported):
            hip.OnlineSession(ctx, lat, 4, window=10)
        lat.close()


# ------------------------------------------------------------------------------------------- configs[4], end to end
K5, W5, N5, M5, D5, U5, TICK = 7, 10, 5, 8, 39, 40, 20


def test_configs4_model_end_to_end(R, hip, ctx):
    """40 streams of seven-word utterances in 20-frame ticks through `push` (likelihoods per tick), a window= and a
    max_frames= decoder side by side with a commit after every tick: (4) and (6) hold, and the settled words are the
    restatement's on the likelihood matrix of the whole utterances."""
    import bench
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(1005)
    wl = bench.synth_workload(1005, 1, W=W5, n=N5, M=M5, D=D5)
    means, vars_, trans = wl["means"], wl["vars"], wl["trans"]
    xs = []
    for u in range(U5):
        segs = []
        for wd in rng.integers(0, W5, size=K5):
            Tw = int(rng.integers(30, 61))
            st = np.minimum(np.arange(Tw) * N5 // Tw, N5 - 1)
            comp = rng.integers(0, M5, size=Tw)
            segs.append(means[wd, st, comp] + np.sqrt(vars_[wd, st, comp]) * rng.standard_normal((Tw, D5)))
        xs.append(np.concatenate(segs))
    hmms = [make_hmm(R, means[i], vars_[i], wl["w"][i], trans) for i in range(W5)]
    dec = ContinuousDecoder(hmms, grammar="loop", ctx=ctx)
    nes, rw, rs, dense, ends = O.loop_grammar([trans] * W5, N5, 0.0)
    case = dict(n=N5, skip=False, nes=nes, rw=rw, rs=rs, dense=dense, ends=ends)
    T = np.array([len(x) for x in xs])
    n_ticks = int(-(-T.max() // TICK))
    b = hip.Batch(ctx, xs, dtype=np.float64)
    nll = b.loglik(dec.gmm, fetch=True)
    off = np.concatenate([[0], np.cumsum(T)])
    ref = [restate(case, emissions(case, nll[off[u]:off[u + 1]]), [len(xs[u][k * TICK:(k + 1) * TICK]) for k in range(n_ticks)])
           for u in range(U5)]
    final = dec.decode_batch(b)[0]
    b.close()
    window = window_of(case, ref)
    assert T.min() >= 3 * window
    ids = np.random.default_rng(8).permutation(U5)
    full, win = dec.online(U5, max_frames=int(T.max())), dec.online(U5, window=window)
    before = [[] for _ in range(U5)]
    for k in range(n_ticks):
        chunks = [x[k * TICK:(k + 1) * TICK] for x in xs]
        for on in (full, win):
            on.push(ids, chunks)
        new_f, new_w = full.commit(ids), win.commit(ids)
        assert new_f == new_w
        (wf, ff), (ww, fw) = full.settled(ids), win.settled(ids)
        assert wf == ww == [ref[u][k][1] for u in range(U5)] and ff.tolist() == fw.tolist() == [ref[u][k][0] for u in range(U5)]
        rf, info_f = full.result(ids)
        rw_, info_w = win.result(ids)
        np.testing.assert_array_equal(info_w["end_cost"], info_f["end_cost"])
        np.testing.assert_array_equal(info_w["best_end"], info_f["best_end"])
        live = finite_end(info_f)
        for u in range(U5):
            assert wf[u] == before[u] + new_f[u] and wf[u] == final[u][:len(wf[u])]
            if live[u]:
                assert rw_[u] == rf[u] and wf[u] == rf[u][:len(wf[u])]
            before[u] = wf[u]
    assert live.all() and rf == final == rw_
    assert np.mean([len(wf[u]) >= K5 - 2 for u in range(U5)]) > 0.9       # most words are final before the audio ends
    full.close()
    win.close()
