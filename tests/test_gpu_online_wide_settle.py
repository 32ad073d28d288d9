# -*- coding: utf-8 -*-
"""The settled prefix of an online decode of MORE THAN 16 WORDS on the device (gh_online_create_wide_settle,
csrc/gh_online_wide_settle.hip: the settle walk over 64 word lanes, the segment walk over the wide history) and the ring of
columns of csrc/gh_viterbi_online_wide.hip.  The opt-in: `dec.online(..., settle=True)`.

L_k: the one-shot labels of the first k frames of a stream; C: the settled words after a commit.
  1. anchors are exact and maximal: settled_frames and C equal the restatement's (tests/online_settle_ref.py) on the batch's
     own fetched fp64 likelihood matrix with the same chunking, for every stream at every tick;
  2. prefix stability, device against device: commits only extend, C is a prefix of the final labels and of L_k where the
     chosen end is finite, `result` equals L_k at every tick (full history + settle leaves gh_online_result alone);
  3. windowed == full history: the same pushes to a window= and a max_frames= session, both committing every tick: end
     costs, chosen ends and frames bitwise equal, settled words and frames the restatement's, result words equal, over
     streams at least 3 x the window long; once with fp32 likelihoods;
  4. word begins after the ring has wrapped eight times;
  5. ties across DPP rows: one model in words 3, 19, 35 and 51, integer costs, one frame per push;
  6. a stream id reused after `finish`;
  7. refusals through the real library;
  8. `push_recording` through a windowed wide decoder.
Streams whose end costs are all +inf are outside the stability contract (include/gmmhmm.h): (2) and the words of (3) leave
such a stream out AT THAT TICK; its anchor, its settled words and its end costs are compared all the same.
Shapes: the WIDE list of tests/test_gpu_online_wide.py; cases as `make_case` of tests/test_gpu_online_settle.py builds them."""
import numpy as np
import pytest

from online_ref import CarriedDecode
from online_settle_ref import SettledDecode
from online_wide_settle_ref import WideSettle, WideSweep
from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu

#        W   n  skip   penalty
WIDE = [(17, 5, False, 0.5),      # one lane past the first DPP row
        (40, 3, True, 1.0),       # a boundary inside a row, skip bits
        (64, 5, False, 0.0),      # a full wave
        (33, 8, True, 2.0),
        (17, 2, False, 0.0),      # the smallest mask
        (64, 8, True, 1.0)]       # the widest record
U, N_IDS, M, D = 13, 17, 2, 6
shape_id = lambda s: "W%d-n%d-%s" % (s[0], s[1], "skip" if s[2] else "plain")


def word_trans(rng, n, skip=False, last_self=0.0, integer=False):
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = (float(rng.integers(0, 3)) if integer else rng.uniform(0.05, 0.6)) if i < n - 1 else last_self
        if i < n - 1:
            t[i + 1, i] = float(rng.integers(1, 4)) if integer else rng.uniform(0.8, 2.5)
        if skip and i < n - 2 and rng.random() < 0.6:
            t[i + 2, i] = rng.uniform(1.5, 4.0)
    return t


def synth(rng, means, vars_, words):
    W, n = means.shape[:2]
    segs = []
    for wd in words:
        Tw = int(rng.integers(n, 3 * n + 4))
        st = np.minimum(np.arange(Tw) * n // Tw, n - 1)
        comp = rng.integers(0, means.shape[2], size=Tw)
        segs.append(means[wd, st, comp] + np.sqrt(vars_[wd, st, comp]) * rng.normal(size=(Tw, means.shape[3])))
    return np.concatenate(segs)


def make_case(W, n, skip, penalty):
    """Model, 13 utterances of 1 - 7 synthetic words (two shorter than a word), 13 long streams (those utterances one after
    the other, cut at 110 + 7 n frames and a few) and the stream ids, scattered over 17.  No GPU."""
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
        words = rng.integers(0, W, size=rng.integers(1, 8))
        xs.append(synth(rng, means, vars_, words))
        n_words.append(len(words))
    long_xs = [np.concatenate([xs[(u + k) % U] for k in range(1, U)])[:110 + 7 * n + u] for u in range(U)]
    ids = rng.permutation(N_IDS)[:U]
    nes, rw, rs, T_, ends = O.loop_grammar(trans, n, penalty)
    return dict(W=W, n=n, skip=skip, penalty=penalty, means=means, vars=vars_, w=w, trans=trans, xs=xs, n_words=n_words,
                long_xs=long_xs, ids=ids, nes=nes, rw=rw, rs=rs, dense=T_, ends=ends, rng=rng)


def schedule(rng, T, choices):
    """Ticks of column counts that feed utterances of T frames: 0- and 1-frame pushes among them."""
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


@pytest.fixture(scope="module", params=WIDE, ids=shape_id)
def committed(request, R, hip, ctx):
    """One full-history session that settles per shape, fed its 13 utterances in random column ranges with a commit after
    every push: what the device said at every tick, the one-shot decodes of the same prefixes, and the restatement on the
    same likelihood matrix.  Computed once, shared by (1) and (2)."""
    case = make_case(*request.param)
    dec = decoder_of(R, ctx, case)
    rng = case["rng"]
    xs, ids = case["xs"], case["ids"]
    b = hip.Batch(ctx, xs, dtype=np.float64)
    nll = b.loglik(dec.gmm, fetch=True)                                  # the matrix both sides decode
    T = np.asarray(b.lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(T)])
    sched = schedule(rng, T, [0, 1, 1, 2, 3, 5, 8, 13, 21])
    on = dec.online(n_streams=N_IDS, max_frames=int(T.max()), settle=True)
    assert isinstance(on.session, hip.OnlineWideSession) and on.session.settles and on.wide and on.settles
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
    paths = on.result(ids, want_path=True)[1]["paths"]                   # full history: the paths are still there
    ref_paths = dec.lat.viterbi(b, want_path=True)["paths"]
    for u in range(U):
        np.testing.assert_array_equal(paths[u], ref_paths[u])
    ref = [restate(case, emissions(case, nll[off[u]:off[u + 1]]), [int(c[u]) for c in sched]) for u in range(U)]
    on.close()
    b.close()
    return dict(case=case, ticks=ticks, final=final, ref=ref, sched=sched, T=T)


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


def run_pair(hip, ctx, dec, case, dtype, streams=U):
    """(3): a window= and a max_frames= session on the same pushes of the first `streams` long streams.  The window is the
    restatement's largest unsettled tail on the device's own matrix (one column per decision word: nothing to round)."""
    rng = np.random.default_rng(5 + case["W"])
    xs, ids = case["long_xs"][:streams], case["ids"][:streams]
    b = hip.Batch(ctx, xs, dtype=dtype)
    nll = b.loglik(dec.gmm, fetch=True)
    T = np.asarray(b.lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(T)])
    sched = schedule(rng, T, [0, 1, 1, 2, 3, 5, 8, 13])
    ref = [restate(case, emissions(case, nll[off[u]:off[u + 1]]), [int(c[u]) for c in sched]) for u in range(streams)]
    window = max(t[2] for r in ref for t in r)
    assert T.min() >= 3 * window, "the streams must be at least 3 x the window long: the ring has to wrap"
    full = dec.online(n_streams=N_IDS, max_frames=int(T.max()), settle=True)
    win = dec.online(n_streams=N_IDS, window=window, settle=True)
    assert win.session.window == window and win.session.settles
    pos = np.zeros(streams, dtype=np.int64)
    compared = 0
    for k, cnt in enumerate(sched):
        for on in (full, win):
            on.push_batch(ids, b, first=pos, count=cnt)
        pos = pos + cnt
        new_f, new_w = full.commit(ids), win.commit(ids)
        assert new_f == new_w
        (wf, ff), (ww, fw) = full.settled(ids), win.settled(ids)
        assert wf == ww and ff.tolist() == fw.tolist() == [ref[u][k][0] for u in range(streams)]
        assert wf == [ref[u][k][1] for u in range(streams)]
        rf, info_f = full.result(ids)
        rw_, info_w = win.result(ids)
        np.testing.assert_array_equal(info_w["end_cost"], info_f["end_cost"])          # bitwise
        np.testing.assert_array_equal(info_w["best_end"], info_f["best_end"])
        np.testing.assert_array_equal(info_w["frames"], info_f["frames"])
        assert sorted(info_w) == sorted(info_f)
        live = finite_end(info_f)
        for u in range(streams):
            if live[u]:
                assert rw_[u] == rf[u], (k, u)
                compared += 1
    assert compared >= streams * len(sched) * 3 // 4 and np.all(pos == T)
    final = full.finish(ids)[0]
    assert win.finish(ids)[0] == final and not win.frames.any() and win.settled()[0] == [[]] * N_IDS
    full.close()
    win.close()
    b.close()


@pytest.mark.parametrize("shape", WIDE, ids=shape_id)
def test_windowed_equals_full_history(R, hip, ctx, shape):
    case = make_case(*shape)
    # (the restatement of 13 long streams of the 64 x 8 graph alone takes about 9 s on a CPU: 7 of them)
    run_pair(hip, ctx, decoder_of(R, ctx, case), case, np.float64, streams=7 if shape[0] * shape[1] == 512 else U)


def test_windowed_equals_full_history_fp32_likelihoods(R, hip, ctx):
    case = make_case(*WIDE[1])
    run_pair(hip, ctx, decoder_of(R, ctx, case, dtype=np.float32), case, np.float32)


def test_begins_after_the_ring_has_wrapped_eight_times(R, hip, ctx):
    """times=True on five streams at least 8 x the window long: the windowed decoder's commit(want_times=True),
    settled_times and result begins equal the full-history decoder's, and `path_to_word_times` of its path -- absolute
    columns, whatever the ring has overwritten."""
    from sr.recognition.batch import path_to_word_times
    case = make_case(*WIDE[1])
    dec = decoder_of(R, ctx, case)
    rng = np.random.default_rng(88)
    S = 5
    xs = [synth(rng, case["means"], case["vars"], rng.integers(0, case["W"], size=40))[:300 + 3 * u] for u in range(S)]
    ids = case["ids"][:S]
    b = hip.Batch(ctx, xs, dtype=np.float64)
    nll = b.loglik(dec.gmm, fetch=True)
    T = np.asarray(b.lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(T)])
    sched = schedule(rng, T, [1, 2, 3, 5, 8])
    ref = [restate(case, emissions(case, nll[off[u]:off[u + 1]]), [int(c[u]) for c in sched]) for u in range(S)]
    window = max(t[2] for r in ref for t in r)
    assert T.min() >= 8 * window, (int(T.min()), window)
    full = dec.online(n_streams=N_IDS, max_frames=int(T.max()), settle=True, times=True)
    win = dec.online(n_streams=N_IDS, window=window, settle=True, times=True)
    pos = np.zeros(S, dtype=np.int64)
    late_words = 0
    for k, cnt in enumerate(sched):
        for on in (full, win):
            on.push_batch(ids, b, first=pos, count=cnt)
        pos = pos + cnt
        (nf, bf), (nw, bw) = full.commit(ids, want_times=True), win.commit(ids, want_times=True)
        assert nf == nw and bf == bw
        late_words += sum(1 for bl in bw for v in bl if v >= 4 * window)
        assert win.settled_times(ids) == full.settled_times(ids)
        assert win.settled(ids)[0] == full.settled(ids)[0] == [ref[u][k][1] for u in range(S)]
        if k % 4 == 0 or k == len(sched) - 1:
            rf, info_f = full.result(ids)
            rw_, info_w = win.result(ids)
            rp, info_p = full.result(ids, want_path=True)
            live = finite_end(info_f)
            for u in range(S):
                if live[u]:
                    assert rw_[u] == rf[u] == rp[u]
                    wt = path_to_word_times(info_p["paths"][u], dec.row_state, dec.n)
                    assert info_w["begins"][u].tolist() == info_f["begins"][u].tolist() == list(wt[1])
                    C, Ct = win.settled([ids[u]])[0][0], win.settled_times([ids[u]])[0]
                    assert C == list(wt[0])[:len(C)] and Ct == list(wt[1])[:len(C)]
    assert np.all(pos == T) and late_words >= S                          # words settled long after the ring first wrapped
    assert live.all()
    full.close()
    win.close()
    b.close()


def test_ties_across_dpp_rows_go_to_the_lowest_word(R, hip, ctx):
    """One model copied into words 3, 19, 35 and 51 of a 52-word loop with integer transition costs, one frame per push and
    a commit after every push: whenever a copy's last state is the column's best, `cand == rm` holds in four lanes of four
    different 16-lane rows, and the hop must take the lowest.  Anchors and words equal the restatement; the bit-level
    restatement counts the tied hop columns the walks pass."""
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(5203)
    W, n = 52, 3
    copies = [3, 19, 35, 51]
    means = rng.normal(size=(W, n, M, D)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M, D))
    w = rng.dirichlet(np.ones(M), size=(W, n))
    trans = [word_trans(rng, n, integer=True) for _ in range(W)]
    for c in copies[1:]:
        means[c], vars_[c], w[c], trans[c] = means[3], vars_[3], w[3], trans[3]
    nes, rw, rs, dense, ends = O.loop_grammar(trans, n, 1.0)
    case = dict(W=W, n=n, nes=nes, rw=rw, rs=rs, dense=dense, ends=ends)
    dec = ContinuousDecoder([make_hmm(R, means[i], vars_[i], w[i], trans[i]) for i in range(W)], grammar="loop", word_penalty=1.0, ctx=ctx)
    S = 6
    xs = [synth(rng, means, vars_, [int(v) if k % 2 else int(rng.choice(copies)) for k, v in enumerate(rng.integers(0, W, size=7))])
          for _ in range(S)]
    ids = np.arange(S)[::-1].copy()
    b = hip.Batch(ctx, xs, dtype=np.float64)
    nll = b.loglik(dec.gmm, fetch=True)
    T = np.asarray(b.lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(T)])
    on = dec.online(n_streams=S, max_frames=int(T.max()), settle=True)
    got = [[] for _ in range(S)]
    for t in range(int(T.max())):
        on.push_batch(ids, b, first=np.minimum(t, T), count=(t < T).astype(np.int64))
        on.commit(ids)
        words, frames = on.settled(ids)
        for u in range(S):
            got[u].append((int(frames[u]), words[u]))
    final = on.result(ids)[0]
    on.close()
    b.close()
    tied = 0
    for u in range(S):
        E = emissions(case, nll[off[u]:off[u + 1]])
        chunks = [int(t < T[u]) for t in range(int(T.max()))]
        ref = restate(case, E, chunks)
        assert got[u] == [(r[0], r[1]) for r in ref], u
        assert got[u][-1][1] == final[u][:len(got[u][-1][1])]
        sw = WideSweep(dense, W, n)
        ws = WideSettle(sw)
        for k, c in enumerate(chunks):
            sw.push(E[:, k:k + c] if c else E[:, :0])
            ws.commit()
            assert (ws.settled_frames, ws.words) == (ref[k][0], ref[k][1])
        rows = lambda eq: sum(1 for q in range(4) if (eq >> (16 * q)) & 0xffff)
        tied += len({j for j, hops, eq in ws.passed if rows(eq) >= 2})
    assert tied >= 10, tied


def test_a_reused_stream_equals_a_fresh_session(R, hip, ctx):
    """A windowed stream is finished and its id takes a SHORTER utterance: no stale anchor, no stale ring -- settled words
    and frames at every tick and the final result equal a fresh session's."""
    case = make_case(*WIDE[0])
    dec = decoder_of(R, ctx, case)
    long_, short = case["long_xs"][1], case["xs"][4][:40]
    assert 2 * len(short) < len(long_) and len(short) >= 12
    window = 60

    def serve(on, k, x, step):
        out = []
        for t in range(0, len(x), step):
            on.push([k], [x[t:t + step]])
            on.commit([k])
            out.append((on.settled([k])[0][0], int(on.settled([k])[1][0])))
        return out
    used = dec.online(n_streams=3, window=window, settle=True)
    serve(used, 1, long_, 7)
    assert used.settled([1])[1][0] > window                               # the ring has wrapped, an anchor is set
    assert used.finish([1])[0] == dec.decode([long_])
    fresh = dec.online(n_streams=3, window=window, settle=True)
    assert serve(used, 1, short, 3) == serve(fresh, 1, short, 3)
    (wu, iu), (wf, i_f) = used.finish([1]), fresh.finish([1])
    assert wu == wf == dec.decode([short])
    np.testing.assert_array_equal(iu["end_cost"], i_f["end_cost"])
    np.testing.assert_array_equal(iu["best_end"], i_f["best_end"])
    used.close()
    fresh.close()


def test_refusals(R, hip, ctx):
    """Through the real library: the graph forms gh_online_create_wide_settle does not take (the message names the entry
    point that does), a push past the window, gh_online_result on a windowed session, paths, an id twice in a commit."""
    from sr.recognition.continuous_speech import packed_lattice, packed_loop_lattice, packed_bigram_lattice
    case = make_case(17, 3, False, 0.5)
    dec = decoder_of(R, ctx, case)
    wt, n = case["trans"], case["n"]
    rng = np.random.default_rng(3)
    beam = packed_loop_lattice(wt, n, 0.0)[0]
    for graphs, match, prepare in (([packed_loop_lattice(wt[:16], n, 0.0)[0]], "gh_online_create takes it", None),
                                   ([packed_lattice(wt, n, [list(range(17))] * 3)[0]], "K-layer", None),
                                   ([packed_bigram_lattice(wt[:4], n, rng.uniform(0.5, 3.0, size=(4, 4)), None)[0]], "gh_online_create_bigram takes it", None),
                                   ([beam], "beam", lambda lat: lat.set_beam(3)),
                                   ([packed_loop_lattice(wt, n, 0.0)[0], packed_loop_lattice(wt, n, 1.0)[0]], "several graphs", None)):
        lat = hip.Lattices(ctx, graphs)
        if prepare:
            prepare(lat)
        for kw in (dict(max_frames=10, settle=True), dict(window=10)):
            with pytest.raises(hip.Unsupported, match=match) as e:
                hip.OnlineWideSession(ctx, lat, 4, **kw)
            assert "gh_online_create_wide_settle" in str(e.value)
        lat.close()
    with pytest.raises(ValueError):
        hip.OnlineWideSession(ctx, dec.lat, 3)
    with pytest.raises(ValueError):
        hip.OnlineWideSession(ctx, dec.lat, 3, max_frames=10, window=10)
    for kw in (dict(settle=True), dict(max_frames=10, window=10, settle=True)):
        with pytest.raises(ValueError):
            dec.online(3, **kw)
    xs = case["long_xs"]
    window = 40
    on = dec.online(n_streams=3, window=window, settle=True)
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
    with pytest.raises(hip.Unsupported, match="tail"):                    # gh_online_result on a windowed session
        s.result([2])
    new = on.commit([2])                                                  # a commit moves the window on
    words, frames = on.settled([2])
    assert words == new and frames[0] > 0 and len(words[0]) >= 1
    on.push([2], [xs[2][window:window + int(frames[0])]])
    assert on.frames[2] == window + frames[0]
    on.reset([2])
    assert on.settled([2])[0] == [[]] and on.settled([2])[1].tolist() == [0] and on.frames[2] == 0
    on.close()
    b.close()


W20, N20, M20, D20 = 20, 3, 2, 39


def test_push_recording_through_a_windowed_wide_decoder(R, hip, ctx):
    """A 20-word model (39 features) behind a StreamingFrontend and a StreamingEndpointer with `window=, settle=True`:
    a commit after every tick, and the utterances equal offline trim_ranges + decode_batch -- ranges, words, begins."""
    import sr.audio_capture as AC
    import stream_endpoints_ref as S
    from sr.feature import StreamingFrontend, feature_stats, features_from_signals
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(2003)
    means = rng.normal(size=(W20, N20, M20, D20)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W20, N20, M20, D20))
    w = rng.dirichlet(np.ones(M20), size=(W20, N20))
    hmms = [make_hmm(R, means[i], vars_[i], w[i], word_trans(rng, N20)) for i in range(W20)]
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=0.5, ctx=ctx)
    rate, tick = 16000, 3200
    sigs = [S.burst_signal(rng, 42000, 40, [(4000, 10000), (24000, 30000)], freq=300.0, rate=rate),
            S.burst_signal(rng, 36000, 40, [(4000, 10000), (24000, 36000)], rate=rate)]           # speech up to the end
    norm = feature_stats(sigs, rate)
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
    ep = AC.StreamingEndpointer(2, cfg, max_chunk=tick)
    fe = StreamingFrontend(2, rate, normalize=norm, max_chunk=ep.max_piece)
    on = dec.online(2, window=longest, frontend=fe, endpointer=ep, times=True, settle=True)
    assert isinstance(on.session, hip.OnlineWideSession) and on.session.window == longest
    got = [[], []]
    for t in range(max(-(-len(s) // tick) for s in sigs)):
        live = [k for k, s in enumerate(sigs) if t * tick < len(s)]
        for u in on.push_recording(live, [sigs[k][t * tick:(t + 1) * tick] for k in live], [(t + 1) * tick >= len(sigs[k]) for k in live]):
            got[u["stream"]].append(u)
    for r in range(2):
        assert [(u["begin"], u["stop"], u["open"], u["words"], u["begins"]) for u in got[r]] == offline[r], r
        assert len(got[r]) >= 1 and all(len(u["words"]) >= 1 for u in got[r])
    assert on.frames.tolist() == [0, 0]
    on.close(); fe.close(); ep.close()
