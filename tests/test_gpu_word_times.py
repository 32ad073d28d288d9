# -*- coding: utf-8 -*-
"""Word begin times on the device: the timed label mode of every kernel that emits labels (MODE 2 of the back-trace
kernels of gh_viterbi_layers.hip, gh_viterbi_layers_wide.hip and gh_viterbi_bigram.hip, the timed walks of
gh_online_settle.hip and gh_decode.hip) through gh_viterbi_labels_timed, gh_viterbi_labels_packed_timed,
gh_online_result_timed, gh_online_commit_timed and gh_online_tail_timed.

THE ORACLE of every offline case is `path_to_word_times` -- the host statement of the rule, itself pinned to the reference's
paths in test_word_times_host.py -- of the `want_path=True` path of the SAME decode; those paths are pinned to the reference
elsewhere (test_gpu_layers.py, test_gpu_bigram.py, test_gpu_seq.py).  Labels and begins are integers: `assert_array_equal`.

Offline batches have 70 utterances (more than one 64-lane back-trace block, rows of a wave ending at different columns):
0, 1 and 2 frames, one below / at / one above one and two multiples of the form's columns per decision word, random lengths
up to 60.  A 1-frame utterance sends the WHOLE batch to the row-per-lane kernels (the reference's column wrap at T == 1), so
every case decodes the batch twice: as it is, and with the 1-frame utterance left out -- the second run is the one that takes
the form's own back-trace, which `Lattices.forms()` and the bitwise-equal end costs of the two routes tie down.

Online: at every tick `result` with times equals `decode_batch(prefix, want_times=True)`; the commits are a prefix of the final
result and equal `settled_times`; a windowed session whose ring has been overwritten many times gives the begins of a
full-history session, absolute columns larger than the ring."""
import numpy as np
import pytest

from conftest import load_golden
from online_ref import CarriedDecode
from online_settle_ref import SettledDecode
from oracle import ref_numpy as O
from test_gpu_layers import word_trans
from test_gpu_seq import forced

pytestmark = pytest.mark.gpu

U70, M, D = 70, 2, 6
TODAY_LABEL_KEYS = ["best_end", "end_cost_flat", "end_off", "label_off", "labels", "labels_flat", "n_labels"]


@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


def loop_cpw(n, skip):
    return 32 // (n + 2 + (n - 2 if skip else 0))


def bigram_cpw(n, skip):
    return 32 // (n + 5 + (n - 2 if skip else 0))


def layer_cpw(n, skip, sets=2):
    bits = sets * (n + 1 + (n - 2 if skip else 0))
    return (64 if bits > 32 else 32) // bits


def make_model(rng, W, n):
    means = rng.normal(size=(W, n, M, D)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M, D))
    w = rng.dirichlet(np.ones(M), size=(W, n))
    return means, vars_, w


def utterance(rng, means, vars_, T):
    """T frames of random words of the model, the last one cut off."""
    W, n = means.shape[:2]
    segs, have = [np.zeros((0, D))], 0
    while have < T:
        wd, Tw = int(rng.integers(0, W)), int(rng.integers(n, 3 * n + 4))
        st = np.minimum(np.arange(Tw) * n // Tw, n - 1)
        comp = rng.integers(0, M, size=Tw)
        segs.append(means[wd, st, comp] + np.sqrt(vars_[wd, st, comp]) * rng.normal(size=(Tw, D)))
        have += Tw
    return np.concatenate(segs)[:T]


def lengths70(rng, cpw):
    T = [0, 1, 2] + [k * cpw + d for k in (1, 2) for d in (-1, 0, 1)]
    T += [int(v) for v in rng.integers(3, 61, size=U70 - len(T))]
    T = np.array(T)
    assert len(T) == U70 and T.min() == 0 and T.max() <= max(60, 2 * cpw + 1)
    return T[rng.permutation(U70)]


def check_labels_with_times(hip, ctx, lat, gmm, xs, row_states, n, dtype, utt_lattice=None, max_labels=None, n_words=1):
    """One batch: labels and begins of the slot route and of the packed route against `path_to_word_times` of the
    want_path=True path of the same decode; the untimed call returns today's keys and the same labels and ends."""
    from sr.recognition.batch import path_to_word_times
    b = hip.Batch(ctx, xs, dtype=dtype)
    b.loglik(gmm, fetch=False)
    U = b.U
    gi = np.zeros(U, dtype=np.int64) if utt_lattice is None else np.asarray(utt_lattice, dtype=np.int64)
    row_label = [np.where(rs >= 0, rs // n, -1).astype(np.int32) for rs in row_states]
    ref = lat.viterbi(b, utt_lattice=utt_lattice, want_path=True)
    want = [path_to_word_times(ref["paths"][u], row_states[gi[u]], n) for u in range(U)]
    timed = lat.viterbi_labels(b, row_label, utt_lattice=utt_lattice, max_labels=max_labels, want_begin=True)
    assert sorted(timed) == sorted(TODAY_LABEL_KEYS + ["begins", "begins_flat"])
    for u in range(U):
        np.testing.assert_array_equal(timed["labels"][u], want[u][0], err_msg="labels of utterance %d (%d frames)" % (u, len(xs[u])))
        np.testing.assert_array_equal(timed["begins"][u], want[u][1], err_msg="begins of utterance %d (%d frames)" % (u, len(xs[u])))
        assert timed["begins"][u].dtype == np.int32
    np.testing.assert_array_equal(timed["best_end"], ref["best_end"])
    np.testing.assert_array_equal(timed["end_cost_flat"], ref["end_cost_flat"])
    packed = lat.viterbi_labels(b, row_label, utt_lattice=utt_lattice, max_labels=max_labels, as_lists=False, want_begin=True)
    assert len(packed["begins_flat"]) == len(packed["labels_flat"]) == sum(len(w[0]) for w in want)
    for u in range(U):
        sl = slice(packed["label_off"][u], packed["label_off"][u] + packed["n_labels"][u])
        np.testing.assert_array_equal(packed["labels_flat"][sl], want[u][0])
        np.testing.assert_array_equal(packed["begins_flat"][sl], want[u][1])
    plain = lat.viterbi_labels(b, row_label, utt_lattice=utt_lattice, max_labels=max_labels)
    assert sorted(plain) == TODAY_LABEL_KEYS                              # want_begin=False: exactly today's keys
    plain_packed = lat.viterbi_labels(b, row_label, utt_lattice=utt_lattice, max_labels=max_labels, as_lists=False)
    assert sorted(plain_packed) == [k for k in TODAY_LABEL_KEYS if k != "labels"]
    np.testing.assert_array_equal(plain["n_labels"], timed["n_labels"])
    for u in range(U):                                      # (the slots of labels_flat are filled up to n_labels only)
        np.testing.assert_array_equal(plain["labels"][u], timed["labels"][u])
    np.testing.assert_array_equal(plain_packed["labels_flat"], packed["labels_flat"])
    np.testing.assert_array_equal(plain["best_end"], timed["best_end"])
    b.close()
    return sum(len(w[0]) >= n_words for w in want), ref


def both_batches(xs):
    """The batch as it is (a 1-frame utterance: the row-per-lane kernels take all of it) and without its 1-frame utterances (the
    form's own kernels); both keep the 0- and 2-frame utterances."""
    lens = [len(x) for x in xs]
    assert 1 in lens and 0 in lens and 2 in lens
    keep = [u for u, T in enumerate(lens) if T != 1]
    return [(xs, None), ([xs[u] for u in keep], keep)]


# ------------------------------------------------------------------------------------------------- offline, every label route
#        name            kind     W   n  skip  K
ROUTES = [("layers",     "layers", 4,  3, False, 3),
          ("layers-K9",  "layers", 3,  3, False, 9),       # more than 8 layers: four register sets (H = 4)
          ("loop-n3",    "loop",   5,  3, False, 0),
          ("loop-n5",    "loop",   4,  5, False, 0),
          ("loop-n5-skip", "loop", 4,  5, True,  0),
          ("loop-n12",   "loop",   3, 12, False, 0),
          ("wide-layers", "layers", 17, 3, False, 2),
          ("wide-loop",  "loop",  17,  3, False, 0),
          ("bigram-n3",  "bigram", 5,  3, False, 0),
          ("bigram-n5",  "bigram", 4,  5, False, 0)]


def route_graph(rng, kind, W, n, skip, K):
    from sr.recognition.continuous_speech import packed_lattice, packed_loop_lattice, packed_bigram_lattice
    wt = [word_trans(rng, n, skip, last_self=rng.uniform(0.0, 0.3)) for _ in range(W)]
    if kind == "layers":
        return packed_lattice(wt, n, [list(range(W))] * K)[0], layer_cpw(n, skip, 4 if K > 8 else 2) if W <= 16 else 1
    if kind == "loop":
        return packed_loop_lattice(wt, n, 0.5)[0], loop_cpw(n, skip) if W <= 16 else 1
    B = rng.uniform(0.0, 4.0, size=(W, W))
    B[1, 2] = np.inf                                                      # one forbidden pair
    return packed_bigram_lattice(wt, n, B, None)[0], bigram_cpw(n, skip)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_offline_labels_with_times_on_every_form(hip, ctx, route, dtype):
    name, kind, W, n, skip, K = route
    rng = np.random.default_rng(4000 + 31 * W + n + K)
    means, vars_, w = make_model(rng, W, n)
    graph, cpw = route_graph(rng, kind, W, n, skip, K)
    gmm = hip.PackedGMM(ctx, means.reshape(W * n, M, D), vars_.reshape(W * n, M, D), w.reshape(W * n, M))
    lat = hip.Lattices(ctx, [graph])
    assert {"layers": "layers", "loop": "loop", "bigram": "bigram"}[kind] in lat.forms()
    xs = [utterance(rng, means, vars_, int(T)) for T in lengths70(rng, cpw)]
    with_words = 0
    for batch, _ in both_batches(xs):
        got, _ = check_labels_with_times(hip, ctx, lat, gmm, batch, [np.asarray(graph["row_state"])], n, dtype, n_words=2)
        with_words += got
    assert with_words >= 20                 # not vacuous: of 2 x 61 random lengths up to 60, those that hold two 12-state words
    lat.close()
    gmm.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("how", ["lean", "generic", "beam"])
def test_offline_labels_with_times_on_the_path_route(hip, ctx, how, dtype):
    """The families that materialise a path on the device and read the labels off it (path_labels_timed_kernel): the lean and
    the generic kernel forced by GMMHMM_VITERBI, and a graph with a rank beam (generic kernel)."""
    from sr.recognition.continuous_speech import packed_loop_lattice
    rng = np.random.default_rng(4100)
    W, n = 5, 3
    means, vars_, w = make_model(rng, W, n)
    graph = packed_loop_lattice([word_trans(rng, n, False, last_self=rng.uniform(0.0, 0.3)) for _ in range(W)], n, 0.5)[0]
    gmm = hip.PackedGMM(ctx, means.reshape(W * n, M, D), vars_.reshape(W * n, M, D), w.reshape(W * n, M))
    lat = hip.Lattices(ctx, [graph])
    xs = [utterance(rng, means, vars_, int(T)) for T in lengths70(rng, loop_cpw(n, False))]
    with_words = 0
    if how == "beam":
        lat.set_beam(9)
    for batch, _ in both_batches(xs):
        if how == "beam":
            got, _ = check_labels_with_times(hip, ctx, lat, gmm, batch, [np.asarray(graph["row_state"])], n, dtype, n_words=2)
        else:
            with forced(GMMHMM_VITERBI=how):
                got, _ = check_labels_with_times(hip, ctx, lat, gmm, batch, [np.asarray(graph["row_state"])], n, dtype, n_words=2)
        with_words += got
    assert with_words >= 20
    lat.set_beam(None)
    lat.close()
    gmm.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_offline_labels_with_times_on_a_transcripts_handle(hip, ctx, dtype):
    """Sequence form: one forced-alignment graph per distinct transcript, built on the library's side.  Two-state words, so
    that the 2-frame utterance holds its one-word transcript (an utterance too short for its transcript has a back-trace
    without predecessor, which the path call refuses just as the label call does)."""
    from sr.recognition.continuous_speech import packed_lattice
    rng = np.random.default_rng(4200)
    W, n = 4, 2
    means, vars_, w = make_model(rng, W, n)
    wt = [word_trans(rng, n, False, last_self=rng.uniform(0.0, 0.3)) for _ in range(W)]
    gmm = hip.PackedGMM(ctx, means.reshape(W * n, M, D), vars_.reshape(W * n, M, D), w.reshape(W * n, M))
    T = lengths70(rng, 32 // n)                                           # gh_seq_cpw: n bits per column
    xs = [utterance(rng, means, vars_, int(t)) for t in T]
    keys, transcripts, utt_graph = {}, [], np.empty(U70, dtype=np.int32)
    for u, t in enumerate(T):
        words = tuple(int(v) for v in rng.integers(0, W, size=min(4, max(1, int(t) // 6))))
        if words not in keys:
            keys[words] = len(transcripts)
            transcripts.append(list(words))
        utt_graph[u] = keys[words]
    lat = hip.Lattices.from_transcripts(ctx, wt, n, transcripts)
    assert lat.forms() == {"sequence"}
    row_states = [np.asarray(packed_lattice(wt, n, [[x] for x in l])[0]["row_state"]) for l in transcripts]
    with_words = 0
    for batch, keep in both_batches(xs):
        ug = utt_graph if keep is None else utt_graph[keep]
        got, ref = check_labels_with_times(hip, ctx, lat, gmm, batch, row_states, n, dtype, utt_lattice=ug, max_labels=5)
        with_words += got
    assert with_words >= 100 and len(transcripts) >= 10
    lat.close()
    gmm.close()


def test_max_labels_too_small_still_raises(hip, ctx):
    from sr.recognition.continuous_speech import packed_loop_lattice
    rng = np.random.default_rng(4300)
    W, n = 5, 3
    means, vars_, w = make_model(rng, W, n)
    graph = packed_loop_lattice([word_trans(rng, n) for _ in range(W)], n, 0.0)[0]
    gmm = hip.PackedGMM(ctx, means.reshape(W * n, M, D), vars_.reshape(W * n, M, D), w.reshape(W * n, M))
    lat = hip.Lattices(ctx, [graph])
    xs = [utterance(rng, means, vars_, 50) for _ in range(5)]
    row_word = np.where(graph["row_state"] >= 0, graph["row_state"] // n, -1).astype(np.int32)
    b = hip.Batch(ctx, xs)
    b.loglik(gmm, fetch=False)
    assert min(lat.viterbi_labels(b, row_word, want_begin=True)["n_labels"]) >= 3
    for kw in (dict(), dict(utt_lattice=np.zeros(5, dtype=np.int32))):    # the direct route and the path route
        for want_begin in (False, True):
            with pytest.raises(hip.BackendError, match="label capacity"):
                lat.viterbi_labels(b, row_word, max_labels=2, want_begin=want_begin, **kw)
    b.close()
    lat.close()
    gmm.close()


def test_device_begins_on_the_reference_goldens(hip, ctx):
    """G4 / G14 / G20: the device's begins equal `path_to_word_times` of the golden's own reference path."""
    from sr.recognition.batch import path_to_word_times
    from sr.recognition.continuous_speech import packed_loop_lattice, packed_bigram_lattice
    cases = []
    g = load_golden("G4_lattice_decode")
    W, n = g["means"].shape[:2]
    for K in (1, 2, 3):
        p = "K%d_" % K
        rw, rs = g[p + "row_word"], g[p + "row_state"]
        graph = dict(row_state=np.where(rw < 0, -1, rw * n + rs), arc_to=g[p + "arc_to"], arc_from=g[p + "arc_from"],
                     arc_cost=g[p + "arc_cost"], start_rows=[0], end_rows=g[p + "ends"])
        cases.append(("G4 " + p, (g["means"], g["vars"], g["w"]), "layers", graph, [g[p + "x"]], [g[p + "path"]], [g[p + "digits"]]))
    g = load_golden("G14_loop_grammar")
    W, n = g["means"].shape[:2]
    for pen in (0, 1):
        pp = "p%d_" % pen
        graph = packed_loop_lattice([g["word_trans"]] * W, n, float(g[pp + "penalty"]))[0]
        us = range(int(g["n_utts"]))
        cases.append(("G14 " + pp, (g["means"], g["vars"], g["w"]), "loop", graph, [g[pp + "x%d" % u] for u in us],
                      [g[pp + "path%d" % u] for u in us], [g[pp + "digits%d" % u] for u in us]))
    g = load_golden("G20_bigram_grammar")
    for c in range(int(g["n_cases"])):
        pp = "c%d_" % c
        W, n = g[pp + "means"].shape[:2]
        graph = packed_bigram_lattice([g["word_trans"]] * W, n, g[pp + "B"], g[pp + "init"])[0]
        us = range(int(g["n_utts"]))
        cases.append(("G20 " + pp, (g[pp + "means"], g[pp + "vars"], g[pp + "w"]), "bigram", graph, [g[pp + "x%d" % u] for u in us],
                      [g[pp + "path%d" % u] for u in us], [g[pp + "digits%d" % u] for u in us]))
    literal = {}
    for name, (means, vars_, w), form, graph, xs, paths, digits in cases:
        W, n, Mg, Dg = means.shape
        gmm = hip.PackedGMM(ctx, means.reshape(W * n, Mg, Dg), vars_.reshape(W * n, Mg, Dg), w.reshape(W * n, Mg))
        lat = hip.Lattices(ctx, [graph])
        assert form in lat.forms()
        rs = np.asarray(graph["row_state"])
        b = hip.Batch(ctx, xs)
        b.loglik(gmm, fetch=False)
        r = lat.viterbi_labels(b, np.where(rs >= 0, rs // n, -1).astype(np.int32), want_begin=True)
        for u in range(len(xs)):
            words, begins = path_to_word_times(paths[u], rs, n)
            assert words == [int(d) for d in digits[u]]
            np.testing.assert_array_equal(r["labels"][u], words)
            np.testing.assert_array_equal(r["begins"][u], begins)
            literal[name + "path%d" % u if form != "layers" else name + "path"] = begins
        b.close()
        lat.close()
        gmm.close()
    assert literal["G14 p0_path2"] == [0, 11, 19, 29, 40] and literal["G20 c1_path2"] == [0, 8, 13, 25, 36] and literal["G4 K3_path"] == [0, 17, 36]


# ------------------------------------------------------------------------------------------------------------------- online
N_STREAMS = 9          # three waves of four streams, the last one partly filled


def online_case(seed, W, n, skip, penalty, T_of):
    rng = np.random.default_rng(seed)
    means, vars_, w = make_model(rng, W, n)
    trans = [word_trans(rng, n, skip, last_self=rng.uniform(0.0, 0.3)) for _ in range(W)]
    xs = [utterance(rng, means, vars_, int(T_of(rng, u))) for u in range(N_STREAMS)]
    nes, rw, rs, dense, ends = O.loop_grammar(trans, n, penalty)
    return dict(W=W, n=n, skip=skip, penalty=penalty, means=means, vars=vars_, w=w, trans=trans, xs=xs, nes=nes, rw=rw, rs=rs,
                dense=dense, ends=ends, rng=rng)


def decoder_of(ctx, case, dtype=np.float64):
    import sr.recognition as R
    from sr.recognition.batch import ContinuousDecoder
    from test_gpu_online_settle import make_hmm
    hmms = [make_hmm(R, case["means"][i], case["vars"][i], case["w"][i], case["trans"][i]) for i in range(case["W"])]
    dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=case["penalty"], dtype=dtype, ctx=ctx)
    assert "loop" in dec.lat.forms()
    return dec


def finite_end(info):
    return np.array([b >= 0 and np.isfinite(info["end_cost"][i, b]) for i, b in enumerate(info["best_end"])])


@pytest.mark.parametrize("chunk", ["1", "7", "cpw-1", "cpw+1"])
def test_online_result_with_times_equals_the_one_shot_decode_at_every_tick(hip, ctx, chunk):
    """Full history (max_frames): words, begins and end costs of `result` are those of `decode_batch(prefix,
    want_times=True)` at every tick, and every commit(want_times=True) extends a prefix of the final result."""
    W, n, skip = 6, 3, True
    case = online_case(5000, W, n, skip, 0.7, lambda rng, u: 2 if u == 4 else rng.integers(18, 34))
    dec = decoder_of(ctx, case)
    c = {"1": 1, "7": 7, "cpw-1": loop_cpw(n, skip) - 1, "cpw+1": loop_cpw(n, skip) + 1}[chunk]
    xs = case["xs"]
    T = np.array([len(x) for x in xs])
    ids = np.random.default_rng(3).permutation(N_STREAMS + 3)[:N_STREAMS]
    on = dec.online(n_streams=N_STREAMS + 3, max_frames=int(T.max()), times=True)
    b = hip.Batch(ctx, xs)
    b.loglik(dec.gmm, fetch=False)
    pos = np.zeros(N_STREAMS, dtype=np.int64)
    acc_w, acc_b = [[] for _ in xs], [[] for _ in xs]
    compared = 0
    while np.any(pos < T):
        cnt = np.minimum(c, T - pos)
        on.push_batch(ids, b, first=pos, count=cnt)
        pos = pos + cnt
        new_w, new_b = on.commit(ids, want_times=True)
        for u in range(N_STREAMS):
            assert len(new_w[u]) == len(new_b[u])
            acc_w[u] += new_w[u]
            acc_b[u] += new_b[u]
        assert on.settled_times(ids) == acc_b and on.settled(ids)[0] == acc_w
        words, info = on.result(ids)
        pb = hip.Batch(ctx, [x[:p] for x, p in zip(xs, pos)])
        ref_words, ref = dec.decode_batch(pb, want_times=True)
        pb.close()
        assert sorted(info) == ["begins", "best_end", "end_cost", "frames"]
        np.testing.assert_array_equal(info["end_cost"].reshape(-1), ref["end_cost_flat"])             # bitwise
        np.testing.assert_array_equal(info["best_end"], ref["best_end"])
        live = finite_end(info)
        for u in range(N_STREAMS):
            assert words[u] == ref_words[u], (int(pos[u]), u)
            np.testing.assert_array_equal(info["begins"][u], ref["begins"][u], err_msg="stream %d after %d frames" % (u, pos[u]))
            if live[u]:                                     # (a +inf end is outside the stability contract)
                assert ref_words[u][:len(acc_w[u])] == acc_w[u] and ref["begins"][u][:len(acc_b[u])].tolist() == acc_b[u]
                compared += len(acc_b[u]) > 0
    assert compared > 0 and sum(len(x) for x in acc_b) >= N_STREAMS
    final_w, final = on.finish(ids)
    for u in range(N_STREAMS):
        if live[u]:
            assert final_w[u][:len(acc_w[u])] == acc_w[u] and final["begins"][u][:len(acc_b[u])].tolist() == acc_b[u]
    assert on.settled_times(ids) == [[]] * N_STREAMS
    # with paths as well, the begins come from the host rule on the session's path
    on.push_batch(ids, b)
    wp, ip = on.result(ids, want_path=True)
    assert wp == final_w and [x.tolist() for x in ip["begins"]] == [x.tolist() for x in final["begins"]]
    on.close()
    b.close()


def restate_tails(case, E, chunks):
    """The restatement's unsettled frames before every commit of a stream fed E [R, T] in `chunks`."""
    cd = CarriedDecode(case["nes"], case["dense"], case["ends"])
    sd = SettledDecode(cd, case["rw"])
    t, out = 0, []
    for c in chunks:
        cd.push(E[:, t:t + c])
        t += int(c)
        out.append(t - sd.settled_frames)
        sd.commit()
    return out


def test_windowed_session_gives_the_begins_of_a_full_history_session(hip, ctx):
    """`window=`: the smallest value for which these seeded streams are never refused -- the largest unsettled tail the CPU
    restatement (tests/online_settle_ref.py) sees before a commit on the batch's own likelihood matrix, rounded up to a
    decision word -- with streams at least eight times the ring long: every ring position is overwritten several times, and
    the begins are absolute columns far larger than the ring."""
    W, n, skip, TICK = 6, 3, False, 7
    case = online_case(5100, W, n, skip, 0.5, lambda rng, u: 330 + 3 * u)
    dec = decoder_of(ctx, case)
    cpw = loop_cpw(n, skip)
    xs = case["xs"]
    T = np.array([len(x) for x in xs])
    b = hip.Batch(ctx, xs)
    nll = b.loglik(dec.gmm, fetch=True)
    off = np.concatenate([[0], np.cumsum(T)])
    col = np.where(case["nes"], 0, case["rw"] * n + case["rs"])
    n_ticks = int(-(-T.max() // TICK))
    tails = []
    for u in range(N_STREAMS):
        E = np.where(case["nes"][:, None], 0.0, np.asarray(nll[off[u]:off[u + 1]], dtype=np.float64)[:, col].T)
        tails += restate_tails(case, E, [len(xs[u][k * TICK:(k + 1) * TICK]) for k in range(n_ticks)])
    window = -(-max(tails) // cpw) * cpw
    ring = window + cpw                                    # whole decision words plus one for the anchor's own
    assert T.min() >= 8 * ring, (int(T.min()), ring)
    ids = np.arange(N_STREAMS)
    full = dec.online(N_STREAMS, max_frames=int(T.max()), times=True)
    win = dec.online(N_STREAMS, window=window, times=True)
    pos = np.zeros(N_STREAMS, dtype=np.int64)
    for k in range(n_ticks):
        cnt = np.minimum(TICK, T - pos)
        for on in (full, win):
            on.push_batch(ids, b, first=pos, count=cnt)
        pos = pos + cnt
        (fw, fb), (ww, wb) = full.commit(ids, want_times=True), win.commit(ids, want_times=True)
        assert fw == ww and fb == wb
        assert full.settled_times(ids) == win.settled_times(ids)
        rf, info_f = full.result(ids)
        rw_, info_w = win.result(ids)
        np.testing.assert_array_equal(info_w["end_cost"], info_f["end_cost"])
        assert sorted(info_w) == sorted(info_f) == ["begins", "best_end", "end_cost", "frames"]
        live = finite_end(info_f)
        assert live.all()
        for u in range(N_STREAMS):
            assert rw_[u] == rf[u]
            np.testing.assert_array_equal(info_w["begins"][u], info_f["begins"][u])
    pb_words, pr = dec.decode_batch(b, want_times=True)
    assert rw_ == pb_words
    for u in range(N_STREAMS):
        np.testing.assert_array_equal(info_w["begins"][u], pr["begins"][u])
        assert info_w["begins"][u].max() > 4 * ring and len(win.settled_times([u])[0]) >= 10
    full.close()
    win.close()
    b.close()


def test_tail_with_times_without_anchor_short_and_idle_streams(hip, ctx):
    """gh_online_tail_timed through a windowed decoder's `result`: a stream that never committed (no anchor: its whole label
    list with begins from column 0), streams of 0 and 1 frames, and a stream that sat ticks out behind its anchor."""
    W, n, skip = 5, 3, False
    case = online_case(5200, W, n, skip, 0.3, lambda rng, u: 60)
    dec = decoder_of(ctx, case)
    xs = case["xs"]
    on = dec.online(N_STREAMS, window=120, times=True)
    # stream 0: never committed; 1: one frame; 2: no frame; 3: committed, then idle; 4: committed every tick
    on.push([0, 1, 3, 4], [xs[0][:40], xs[1][:1], xs[3][:40], xs[4][:20]])
    assert len(on.commit([3, 4], want_times=True)[1][0]) >= 1
    on.push([4, 0], [xs[4][20:45], xs[0][40:50]])           # stream 3 sits this tick out
    on.commit([4])
    on.push([4], [xs[4][45:60]])                             # ... and this one
    given = {0: 50, 1: 1, 2: 0, 3: 40, 4: 60}
    ids = [3, 0, 2, 4, 1]
    words, info = on.result(ids)
    raw = on.session.tail(np.array(ids), row_label=on._row_word, max_labels=62, want_begin=True)
    plain = on.session.tail(np.array(ids), row_label=on._row_word, max_labels=62)
    assert sorted(plain) == ["best_end", "end_cost", "frames", "labels"] and sorted(raw) == sorted(list(plain) + ["begins"])
    pb = hip.Batch(ctx, [xs[k][:given[k]] for k in ids])
    ref_words, ref = dec.decode_batch(pb, want_times=True)
    pb.close()
    for i, k in enumerate(ids):
        assert words[i] == ref_words[i], k
        np.testing.assert_array_equal(info["begins"][i], ref["begins"][i])
        settled = len(on.settled_times([k])[0])
        np.testing.assert_array_equal(raw["begins"][i], ref["begins"][i][settled:])      # the tail's own begins: behind the anchor
        np.testing.assert_array_equal(raw["labels"][i], plain["labels"][i])
    assert on.settled_times([0]) == [[]] and len(ref["begins"][1]) >= 2 and ref["begins"][1][0] == 0   # stream 0: no anchor
    assert len(on.settled_times([3])[0]) >= 1 and len(on.settled_times([4])[0]) >= 2
    assert info["begins"][2].tolist() == [] and info["begins"][4].tolist() == []
    on.close()


def test_untimed_online_calls_keep_their_keys_and_types(hip, ctx):
    case = online_case(5300, 4, 3, False, 0.0, lambda rng, u: 30)
    dec = decoder_of(ctx, case)
    for kw in (dict(max_frames=30), dict(window=60)):
        on = dec.online(N_STREAMS, **kw)
        on.push([2, 5], [case["xs"][2], case["xs"][5][:17]])
        new = on.commit([2, 5])
        assert isinstance(new, list) and all(isinstance(w, list) for w in new)
        words, info = on.result([2, 5])
        assert sorted(info) == ["best_end", "end_cost", "frames"]
        with pytest.raises(ValueError):
            on.commit([2], want_times=True)
        with pytest.raises(ValueError):
            on.settled_times()
        s = on.session
        assert sorted(s.commit(np.array([2]), row_label=on._row_word, max_labels=32)) == ["labels", "settled_frames"]
        assert sorted(s.tail(np.array([2]), row_label=on._row_word, max_labels=32)) == ["best_end", "end_cost", "frames", "labels"]
        if "max_frames" in kw:
            assert sorted(s.result(np.array([2]), row_label=on._row_word)) == ["best_end", "end_cost", "frames", "labels"]
        on.close()


# ---------------------------------------------------------------------------------------------- push_recording with times=True
def test_push_recording_reports_word_begins_in_recording_samples(hip):
    """`word_begin` == offline `trim_ranges(detect_endpoints(...))` begin + `decode_batch(..., want_times=True)` begins x the
    front-end's step, on seeded burst signals of the streaming-endpoint tests (three 16 kHz recordings with two bursts each,
    the last one ending while speech is open), with full history and with a window."""
    import sr.audio_capture as AC
    import sr.recognition as R
    import stream_endpoints_ref as S
    from sr.feature import StreamingFrontend, feature_stats, features_from_signals
    from sr.recognition.batch import ContinuousDecoder
    from test_gpu_api import make_hmm
    ctx = hip.default_context()
    rng = np.random.default_rng(17)
    rate, TICK = 16000, 3200
    sigs = [S.burst_signal(rng, ln, 40, [(4000, 10000), (24000, 30000)], freq=300.0 + 150 * i, rate=rate) for i, ln in enumerate([42000, 43333])]
    sigs.append(S.burst_signal(rng, 36000, 40, [(4000, 10000), (24000, 36000)], rate=rate))
    norm = feature_stats(sigs, rate)
    W, n, Mm, Dd = 3, 4, 2, 39
    trans = np.full((n, n), np.inf)
    for i in range(n):
        trans[i, i] = -np.log(0.8) if i < n - 1 else 0.0
        if i < n - 1:
            trans[i + 1, i] = -np.log(0.2)
    hmms = [make_hmm(R, rng.normal(size=(n, Mm, Dd)), rng.uniform(0.5, 1.5, size=(n, Mm, Dd)), rng.dirichlet(np.ones(Mm), size=n), trans)
            for _ in range(W)]
    dec = ContinuousDecoder(hmms, grammar="loop", ctx=ctx)
    cfg = AC.default_config(rate)
    det = AC.detect_endpoints(sigs, dict(cfg), max_segments=8)
    assert det["n_segments"].tolist() == [2, 2, 2]
    begin, stop = AC.trim_ranges(det, [len(x) for x in sigs], dict(cfg))
    rec = np.repeat(np.arange(3), det["n_segments"])
    offline = [[] for _ in sigs]
    longest = 0
    for r, b0, e0 in zip(rec, begin, stop):
        batch = features_from_signals([sigs[r][b0:e0]], rate, normalize=norm)
        words, info = dec.decode_batch(batch, want_times=True)
        offline[r].append((int(b0), int(e0), words[0], info["begins"][0].tolist()))
        longest = max(longest, int(batch.lengths[0]))
        batch.close()
    for mode in ("max_frames", "window"):
        ep = AC.StreamingEndpointer(3, dict(cfg), max_chunk=TICK)
        fe = StreamingFrontend(3, rate, normalize=norm, max_chunk=ep.max_piece)
        on = dec.online(3, frontend=fe, endpointer=ep, times=True, **({"max_frames": longest} if mode == "max_frames" else {"window": longest + 8}))
        got = [[] for _ in sigs]
        for t in range(max(-(-len(s) // TICK) for s in sigs)):
            live = [k for k, s in enumerate(sigs) if t * TICK < len(s)]
            for u in on.push_recording(live, [sigs[k][t * TICK:(t + 1) * TICK] for k in live], [(t + 1) * TICK >= len(sigs[k]) for k in live]):
                got[u["stream"]].append(u)
        for r, per in enumerate(offline):
            assert [(u["begin"], u["stop"], u["words"], u["begins"]) for u in got[r]] == per, (mode, r)
            for u, (b0, _, words, begins) in zip(got[r], per):
                assert sorted(u) == ["begin", "begins", "open", "stop", "stream", "word_begin", "words"]
                assert u["word_begin"] == [b0 + f * fe.step for f in begins] and len(words) >= 1 and begins[0] == 0
        on.close()
        fe.close()
        ep.close()
