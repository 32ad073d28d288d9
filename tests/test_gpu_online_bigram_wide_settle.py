# -*- coding: utf-8 -*-
"""The settled prefix and the windowed history of an online decode with a BIGRAM grammar of 17 to 64 words on the device
(gh_online_create_bigram_wide_settle; online_bigram_wide_settle_kernel / online_bigram_wide_segment_kernel in
csrc/gh_online_bigram_wide_settle.hip; the ring store of viterbi_bigram_online_wide_kernel), through
`ContinuousDecoder.online_bigram(window=, wide="settle")` and `(max_frames=, settle=True, wide="settle")`.

C: the settled words after a commit; B: their begin frames (times=True).
  1. anchors are exact and maximal: at every tick settled_frames, C and B of a full-history and of a windowed session equal
     the restatement's (tests/online_settle_ref.py on tests/online_ref.py) on the batch's own fp64 likelihood matrix;
  2. prefix stability, device against device: C and B only ever extend, are a prefix of the session's own `result` now and
     at the end, and -- where the chosen end is finite -- of the result of a plain `online_bigram(max_frames, wide=True)`
     session fed the same frames, whose words, begins, end costs and chosen ends the windowed `result` equals as well;
  3. windowed == full history after the ring has wrapped eight times, window = the restatement's largest tail;
  4. the hop, constructed with integer costs; 5. edges; 6. refusals through the real library; 7. recordings.
Shapes: W = 17 with every N = 2 .. 8 x skip arcs, W = 33, 49 and 64 at N = 5; D = 5, 5 streams on 7 ids, utterances of 1 to
7 synthetic words, two of them shorter than a word.  A stream is named in a tick while it still has frames to take.
THE INPUT CONDITIONS -- an anchor that advances at three ticks or more, a settled path through an entry row, 3/4 of the
(stream, tick) pairs with >= 2 frames with a finite chosen end, a column in which live first states hop to two different
words, a hop that crosses a 16-lane group -- are asserted from the restatement BEFORE the device is compared."""
import numpy as np
import pytest

from online_bigram_wide_settle_ref import BigramWideSettle, BigramWideSweep, HopLog
from online_ref import CarriedDecode
from test_gpu_online_bigram import M, make_hmm, make_model, random_costs, ticks_of, word_trans, TICK
from test_gpu_online_bigram_settle import dense_of, emissions, live_schedule, per_stream_chunks
from test_gpu_online_settle import finite_end

pytestmark = pytest.mark.gpu


def write_emissions(hip, ctx, batch, nll):
    """Replace the resident [N, S] likelihood matrix of `batch` (the library has no call for it).  hipMemcpy is looked up
    THROUGH THE LIBRARY'S OWN HANDLE, so it is the one of the HIP runtime the library is linked against and the pointer
    belongs to: a process may hold a second runtime (the one an imported torch brings along), which knows neither."""
    import ctypes
    ctx.sync()
    lib = hip.load_library()
    dev = lib.gh_loglik_dev_ptr(batch.h)
    assert dev
    copy, sync = lib.hipMemcpy, lib.hipDeviceSynchronize
    copy.restype, copy.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    sync.restype, sync.argtypes = ctypes.c_int, []
    nll = np.ascontiguousarray(nll)
    assert copy(dev, nll.ctypes.data, nll.nbytes, 1) == 0                 # hipMemcpyHostToDevice
    assert sync() == 0

U, N_IDS, D = 5, 7, 5
#          W   n  skip
SHAPES = ([(17, 2, False)] + [(17, n, s) for n in range(3, 9) for s in (False, True)] +
          [(33, 5, False), (49, 5, True), (64, 5, False)])
LONG = [(17, 2, False), (64, 5, False), (64, 8, True)]
shape_id = lambda s: "W%d-n%d-%s" % (s[0], s[1], "skip" if s[2] else "plain")


def make_case(W, n, skip, seed=0):
    """Model, bigram costs with +inf pairs and starts, 5 utterances of 1 - 7 synthetic words (utterances 0 and 3 shorter than a
    word) and the stream ids, scattered over 7.  No GPU."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(4100 + 77 * W + 2 * n + skip + 1000 * seed)
    means, vars_, w = make_model(rng, W, n, d=D)
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
        if u % 3 == 0:
            xs.append(rng.normal(size=(min(n - 1, 2), D)) * 2.0)         # shorter than any word (n = 2: one frame)
        else:
            xs.append(synth(rng.integers(0, W, size=rng.integers(1, 8) if u != 1 else 7)))
    ids = rng.permutation(N_IDS)[:U]
    graph, _ = packed_bigram_lattice(trans, n, B, init)
    nes = graph["row_state"] < 0
    return dict(W=W, n=n, skip=skip, means=means, vars=vars_, w=w, trans=trans, B=B, init=init, xs=xs, ids=ids, synth=synth,
                graph=graph, nes=nes, rw=np.where(nes, -1, graph["row_state"] // n), rng=rng,
                dense=dense_of(graph), ends=[int(e) for e in graph["end_rows"]])


def restate(case, E, chunks, ties=False):
    """The row-level restatement on the emission matrix E [R, T] of one stream fed in `chunks`: (its HopLog, per tick
    dict(settled, words, begins, tail: unsettled frames the history held before the commit, frames, entry: the settled path
    passes an entry row, finite: the chosen end is a live cell))."""
    from sr.recognition.batch import path_to_word_times
    cd = CarriedDecode(case["nes"], case["dense"], case["ends"])
    cols = [] if ties else None
    sd = HopLog(cd, case["rw"], case["W"], case["n"], cols=cols)
    t, out = 0, []
    for c in chunks:
        new_cols = cd.push(E[:, t:t + c])
        if ties:
            cols.extend(new_cols.T)
        t += int(c)
        tail = t - sd.settled_frames
        sd.commit()
        ec, bi, _ = cd.result()
        entry, begins = False, []
        if sd.anchor is not None:
            path = sd.path_from(sd.anchor[1], sd.anchor[0])
            entry = bool(np.any(case["nes"][path[:, 0]] & (path[:, 0] > 0)))
            words, begins = path_to_word_times(path, np.where(case["nes"], -1, case["rw"]), 1)
            assert words == sd.words
        out.append(dict(settled=sd.settled_frames, words=list(sd.words), begins=[int(v) for v in begins], tail=tail, frames=t,
                        entry=entry, finite=bool(bi >= 0 and np.isfinite(ec[bi]))))
    return sd, out


def assert_input_conditions(logs, refs):
    """What the issue asks of the inputs, from the restatement alone.  Conditions, not tolerances."""
    adv = max(sum(a["settled"] != b["settled"] for a, b in zip(r[1:], r[:-1])) + (r[0]["settled"] > 0) for r in refs)
    pairs = [tk for r in refs for tk in r if tk["frames"] >= 2]
    fin = sum(tk["finite"] for tk in pairs)
    entry = any(tk["entry"] for r in refs for tk in r)
    two, cross = sum(sd.two_word_columns() for sd in logs), sum(sd.crossing_hops() for sd in logs)
    assert adv >= 3 and entry and 4 * fin >= 3 * len(pairs) and two >= 1 and cross >= 1, (adv, entry, fin, len(pairs), two, cross)


def restate_bits(case, E, chunks):
    """The BIT-LEVEL restatement (tests/online_bigram_wide_settle_ref.py, held against the row-level one by
    tests/test_online_bigram_wide_settle_host.py) of one stream, for the long streams: per tick dict(settled, words, tail,
    frames, finite); and (anchor advances, entry rows passed, two-word hop columns, crossing hops)."""
    sw = BigramWideSweep(case["dense"], case["W"], case["n"])
    ws = BigramWideSettle(sw)
    end_cell = [(int(np.argwhere(sw.row == e)[0][0]), int(np.argwhere(sw.row == e)[0][1])) for e in case["ends"]]
    t, out, adv = 0, [], 0
    for c in chunks:
        sw.push(E[:, t:t + c])
        t += int(c)
        tail, before = t - ws.settled_frames, ws.anchor
        ws.commit()
        assert ws.flag == 0
        adv += ws.anchor != before
        ec = [sw.prev[s, w] for s, w in end_cell]
        out.append(dict(settled=ws.settled_frames, words=list(ws.words), tail=tail, frames=t, finite=bool(t > 0 and np.isfinite(min(ec)))))
    two = sum(len({v for _, v in h}) >= 2 for _, h in ws.passed)
    cross = sum(l // 16 != v // 16 for _, h in ws.passed for l, v in h)
    return out, (adv, ws.entries, two, cross)


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
    assert "bigram_wide" in dec.lat.forms() and "bigram" not in dec.lat.forms()
    np.testing.assert_array_equal(dec.row_state, case["graph"]["row_state"])
    assert list(dec.lat.end_rows[0]) == list(case["ends"])
    return dec


@pytest.fixture(scope="module", params=SHAPES, ids=shape_id)
def committed(request, R, hip, ctx):
    """Per shape: a full-history session that settles, a windowed one (window: the longest utterance, so nothing is ever
    refused) and a plain one, fed the 5 utterances in random column ranges with a commit after every push.  What the device
    said at every tick, and the restatement on the same likelihood matrix.  Computed once, shared by (1) and (2)."""
    case = make_case(*request.param)
    dec = decoder_of(R, ctx, case)
    rng = case["rng"]
    xs, ids = case["xs"], case["ids"]
    b = hip.Batch(ctx, xs, dtype=np.float64)
    nll = b.loglik(dec.gmm, fetch=True)                                  # the matrix both sides decode
    T = np.asarray(b.lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(T)])
    sched = live_schedule(rng, T, [0, 1, 1, 2, 3, 5, 8, 13, 21])
    assert any(0 in cnt for _, cnt in sched) and any(1 in cnt for _, cnt in sched)
    both = [restate(case, emissions(case, nll[off[u]:off[u + 1]]), per_stream_chunks(sched, u)) for u in range(U)]
    logs, ref = [sd for sd, _ in both], [r for _, r in both]
    assert_input_conditions(logs, ref)                                   # before the device is looked at
    full = dec.online_bigram(N_IDS, max_frames=int(T.max()), settle=True, times=True, wide="settle")
    win = dec.online_bigram(N_IDS, window=int(T.max()), times=True, wide="settle")
    plain = dec.online_bigram(N_IDS, max_frames=int(T.max()), times=True, wide=True)
    for on in (full, win, plain):
        assert isinstance(on.session, hip.OnlineBigramWideSession) and on.wide
    assert full.settles and win.settles and not plain.settles and win.session.window == T.max() and full.session.window is None
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
    paths = full.result(ids, want_path=True)[1]["paths"]                 # full history: the paths are still there
    ref_paths = dec.lat.viterbi(b, want_path=True)["paths"]
    for u in range(U):
        np.testing.assert_array_equal(paths[u], ref_paths[u])
    out = dict(case=case, ticks=ticks, ref=ref, sched=sched, T=T, final=final[0], final_begins=[x.tolist() for x in final[1]["begins"]])
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
                got = (int(tk[name]["frames"][i]), tk[name]["words"][i], tk[name]["times"][i])
                assert got == (want["settled"], want["words"], want["begins"]), (name, u, k_of[u])
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


# ----------------------------------------------------------------------------------------------------------------------
LONG_FRAMES = 640


def run_pair(hip, ctx, dec, case, dtype):
    """(3): a window= and a max_frames=, settle=True session on the same pushes of long streams; the window is the
    restatement's largest unsettled tail on the device's own matrix (one column per record word: nothing to round)."""
    rng = np.random.default_rng(5 + case["W"] + case["n"])
    xs = [case["synth"](rng.integers(0, case["W"], size=200))[:LONG_FRAMES + 3 * u] for u in range(U)]
    ids = case["ids"]
    b = hip.Batch(ctx, xs, dtype=dtype)
    nll = b.loglik(dec.gmm, fetch=True)
    T = np.asarray(b.lengths, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(T)])
    sched = live_schedule(rng, T, [0, 1, 1, 2, 3, 5, 8, 13, 21])
    both = [restate_bits(case, emissions(case, nll[off[u]:off[u + 1]]), per_stream_chunks(sched, u)) for u in range(U)]
    ref, seen = [r for r, _ in both], np.sum([s for _, s in both], axis=0)
    pairs = [tk for r in ref for tk in r if tk["frames"] >= 2]
    assert max(s[0] for _, s in both) >= 3 and np.all(seen[1:] >= 1) and 4 * sum(tk["finite"] for tk in pairs) >= 3 * len(pairs), seen
    window = max(tk["tail"] for r in ref for tk in r)
    assert T.min() >= 8 * (window + 1), "the streams must be long enough for the ring to wrap eight times: %d, %d" % (T.min(), window)
    full = dec.online_bigram(N_IDS, max_frames=int(T.max()), settle=True, times=True, wide="settle")
    win = dec.online_bigram(N_IDS, window=window, times=True, wide="settle")
    assert win.session.window == window and win.session.settles
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


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("shape", LONG, ids=shape_id)
def test_windowed_equals_full_history(R, hip, ctx, shape, dtype):
    case = make_case(*shape, seed=1)
    run_pair(hip, ctx, decoder_of(R, ctx, case, dtype=dtype), case, dtype)


# ----------------------------------------------------------------------------------------------------------------------
def integer_case(W, n, seqs, twins, seed):
    """(4): a bigram graph with small-integer costs and an INTEGER likelihood matrix written over the batch's own: the
    states of the words of `seqs` cost 0 in their frames, every other state 2 .. 5.  twins: (a, b) pairs of words with equal
    transitions, equal rows and columns of B and equal likelihoods: as predecessors they tie at every entry row, exactly.
    The unit of the likelihoods is 2^-30, not 1: every state adds its own 20-bit multiple of it to its integers (twins
    share theirs), so all arithmetic stays exact and the ties are those between twins.  Without that, whole-number costs tie
    INSIDE the words as well, and there the records and the reference go different ways: on "stay in state 1" against "come
    from state 0" at equal cost the sweeps take state 0 (the lower state), decode_hmm_states the lower ROW, which is state 1
    -- first states have the highest rows of a loop or bigram graph.  The caller asserts that no such tie is met."""
    from sr.recognition.continuous_speech import packed_bigram_lattice
    rng = np.random.default_rng(seed)
    means, vars_, w = make_model(rng, W, n, d=D)
    trans = [word_trans(rng, n, integer=True, last_self=0.0) for _ in range(W)]
    B = rng.integers(1, 4, size=(W, W)).astype(np.float64)
    B[rng.random((W, W)) < 0.1] = np.inf
    init = rng.integers(0, 3, size=W).astype(np.float64)
    for sq in seqs:                                                       # the spoken pairs are allowed and cheap
        init[sq[0]] = 0.0
        for a, c in zip(sq[:-1], sq[1:]):
            B[a, c] = 1.0
    for a, c in twins:                                                    # (a twin of a spoken word is spoken: the cheaper cost is both's)
        trans[c] = trans[a]
        B[a] = B[c] = np.minimum(B[a], B[c])
        init[a] = init[c] = min(init[a], init[c])
    for a, c in twins:
        B[:, a] = B[:, c] = np.minimum(B[:, a], B[:, c])
    frac = rng.integers(1, 1 << 20, size=W * n) * 2.0 ** -30
    lens, nlls = [], []
    for sq in seqs:
        cols = []
        for wd in sq:
            Tw = int(rng.integers(n, 2 * n + 2))
            for k in range(Tw):
                e = rng.integers(2, 6, size=W * n).astype(np.float64)
                e[wd * n + min(k * n // Tw, n - 1)] = 0.0
                cols.append(e)
        x = np.array(cols) + frac
        for a, c in twins:
            x[:, a * n:(a + 1) * n] = x[:, c * n:(c + 1) * n] = np.minimum(x[:, a * n:(a + 1) * n], x[:, c * n:(c + 1) * n])
        nlls.append(x)
        lens.append(len(x))
    graph, _ = packed_bigram_lattice(trans, n, B, init)
    nes = graph["row_state"] < 0
    return dict(W=W, n=n, skip=False, means=means, vars=vars_, w=w, trans=trans, B=B, init=init, lens=lens, nll=np.concatenate(nlls),
                graph=graph, nes=nes, rw=np.where(nes, -1, graph["row_state"] // n), dense=dense_of(graph),
                ends=[int(e) for e in graph["end_rows"]])


HOPS = {64: dict(n=3, seed=640,
                 # low -> high -> low words, a repeated word, words whose twins sit 32 lanes up
                 seqs=[[3, 50, 7, 60, 60, 2, 55], [48, 5, 5, 63, 9, 49], [12, 12, 58, 1, 52, 52], [20, 40, 10, 33], [6, 61, 14]],
                 twins=[(k, k + 32) for k in (4, 5, 8, 9, 11, 13, 21, 26)]),
        17: dict(n=3, seed=170,
                 # the one lane of the second 16-lane group: word 16 after itself and between the others
                 seqs=[[16, 16, 3, 16, 16, 9], [5, 16, 16, 16, 2], [16, 0, 16, 16, 15], [7, 16, 16], [16, 16, 16, 16]],
                 twins=[])}


@pytest.mark.parametrize("W", [64, 17])
def test_the_hop_constructed(R, hip, ctx, W):
    """Integer costs (`integer_case`), one frame per push, a commit after every push.  From the restatement, before the device
    is compared: a column in which two live first states name different predecessors; two hoppers that name the same word; a hopper that
    names itself; at W = 64 a hop from a word below 16 to a word at 48 or above and one the other way, and a hop whose
    predecessors tied (the lowest word wins); at W = 17 a column in which lane 16, the one lane of the second group, is
    hopper and target.  Then anchors, words and begins of a full-history and of a windowed session equal the restatement's."""
    spec = HOPS[W]
    case = integer_case(W, spec["n"], spec["seqs"], spec["twins"], spec["seed"])
    S = len(spec["seqs"])
    T = np.asarray(case["lens"], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(T)])
    both = [restate(case, emissions(case, case["nll"][off[u]:off[u + 1]]), [1] * int(T[u]), ties=True) for u in range(S)]
    logs, ref = [sd for sd, _ in both], [r for _, r in both]
    assert_input_conditions(logs, ref)
    for u in range(S):                                                    # no tie inside a word (integer_case): records == rows
        bits = restate_bits(case, emissions(case, case["nll"][off[u]:off[u + 1]]), [1] * int(T[u]))[0]
        assert [(tk["settled"], tk["words"]) for tk in bits] == [(tk["settled"], tk["words"]) for tk in ref[u]], u
    hops = [h for sd in logs for h in sd.hops.values()]
    assert any(len({v for _, v in h}) >= 2 for h in hops)                 # two live first states, different predecessors
    assert any(len(h) > len({v for _, v in h}) for h in hops)             # two hoppers name the same word
    assert any(w == v for h in hops for w, v in h)                        # a hopper names itself
    if W == 64:
        assert any(w < 16 and v >= 48 for h in hops for w, v in h) and any(w >= 48 and v < 16 for h in hops for w, v in h)
        assert sum(len(sd.tied) for sd in logs) >= 3                      # predecessor ties on the walks: the lowest word
    else:
        assert any(any(w == 16 for w, _ in h) and any(v == 16 for _, v in h) for h in hops)
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, [np.zeros((int(t), D)) for t in T], dtype=np.float64)
    own = b.loglik(dec.gmm, fetch=True)
    assert own.shape == case["nll"].shape and own.dtype == np.float64
    write_emissions(hip, ctx, b, case["nll"])                             # the integer matrix, over the batch's own
    ids = np.arange(S)[::-1].copy()
    window = max(tk["tail"] for r in ref for tk in r)
    full = dec.online_bigram(S, max_frames=int(T.max()), settle=True, times=True, wide="settle")
    win = dec.online_bigram(S, window=window, times=True, wide="settle")
    for t in range(int(T.max())):
        live = np.flatnonzero(t < T)
        count = (t < T).astype(np.int64)
        for on in (full, win):
            on.push_batch(ids, b, first=np.minimum(t, T), count=count)
            on.commit(ids[live])
            words, frames = on.settled(ids[live])
            times = on.settled_times(ids[live])
            for i, u in enumerate(live):
                want = ref[u][t]
                assert (int(frames[i]), words[i], times[i]) == (want["settled"], want["words"], want["begins"]), (t, u)
    rf, info_f = full.result(ids)
    rw_, info_w = win.result(ids)
    assert rf == rw_ and all(len(x) >= 2 for x in rf)
    np.testing.assert_array_equal(info_w["end_cost"], info_f["end_cost"])
    for u in range(S):
        C = ref[u][-1]["words"]
        assert len(C) >= 1 and C == rf[u][:len(C)]
    full.close(); win.close(); b.close()


# ----------------------------------------------------------------------------------------------------------------------
def test_edges(R, hip, ctx):
    """Streams with 0 and 1 frames in a commit; a commit with no new frames; a stream whose newest column is all +inf; an id
    named twice; a reused stream id against a fresh session."""
    case = make_case(17, 3, False, seed=2)
    dec = decoder_of(R, ctx, case)
    rng = case["rng"]
    long_, short, dead = (case["synth"](rng.integers(0, 17, size=k)) for k in (24, 4, 6))
    K = 20                                                                # the frame of `dead` that no state can emit
    assert len(dead) > K + 2 and len(short) >= 12 and len(long_) > 2 * 60
    b = hip.Batch(ctx, [long_, short, dead], dtype=np.float64)
    nll = b.loglik(dec.gmm, fetch=True)
    off = np.concatenate([[0], np.cumsum(b.lengths)])
    nll[off[2] + K, :] = np.inf
    write_emissions(hip, ctx, b, nll)
    E = [emissions(case, nll[off[u]:off[u + 1]]) for u in range(3)]
    window = 60
    for on in (dec.online_bigram(4, window=window, times=True, wide="settle"),
               dec.online_bigram(4, max_frames=len(long_), settle=True, times=True, wide="settle")):
        # streams 3 / 1 / 0 / 2 hold 0, 1, 30 and K + 1 frames: the newest column of stream 2 is all +inf
        on.push_batch([0, 1, 2], b, first=[0, 0, 0], count=[30, 1, K + 1])
        want = [restate(case, E[0], [30])[1][-1], restate(case, E[1], [1])[1][-1], restate(case, E[2], [K, 1])[1]]
        assert want[2][0]["settled"] > 0 and want[2][1]["settled"] == want[2][0]["settled"] and not want[2][1]["finite"]
        new = on.commit([3, 1, 0])
        assert new[0] == [] and new[1] == [] and new[2] == want[0]["words"] and len(new[2]) >= 1
        assert on.settled([3, 1, 0])[1].tolist() == [0, 0, want[0]["settled"]]
        assert on.commit([3, 1, 0]) == [[], [], []]                       # no new frames: nothing moves
        assert on.settled([3, 1, 0])[1].tolist() == [0, 0, want[0]["settled"]] and on.settled([0])[0] == [want[0]["words"]]
        # a dead newest column has no live cell to trace from: nothing is settled, nothing is flagged
        assert on.commit([2]) == [[]] and on.settled([2])[1].tolist() == [0]
        for bad in ([1, 1], [0, 2, 0]):
            with pytest.raises(ValueError):
                on.commit(bad)
            with pytest.raises(hip.BackendError, match="named twice"):
                on.session.commit(bad)
        assert on.settled([0])[1].tolist() == [want[0]["settled"]]
        on.close()
    # a stream that settled BEFORE its column died keeps its anchor
    on = dec.online_bigram(4, window=window, times=True, wide="settle")
    on.push_batch([0, 1, 2], b, first=[0, 0, 0], count=[0, 0, K])
    assert on.commit([2]) == [want[2][0]["words"]] and len(want[2][0]["words"]) >= 1
    on.push_batch([0, 1, 2], b, first=[0, 0, K], count=[0, 0, 1])
    assert on.commit([2]) == [[]] and on.settled([2])[1].tolist() == [want[2][1]["settled"]]
    on.close()
    b.close()

    # a windowed stream is finished and its id takes a SHORTER utterance: no stale anchor, no stale ring
    def serve(on, k, x, step):
        out = []
        for t in range(0, len(x), step):
            on.push([k], [x[t:t + step]])
            on.commit([k])
            out.append((on.settled([k])[0][0], int(on.settled([k])[1][0]), on.settled_times([k])[0]))
        return out
    used = dec.online_bigram(3, window=window, times=True, wide="settle")
    serve(used, 1, long_, 7)
    assert used.settled([1])[1][0] > window                               # the ring has wrapped, an anchor is set
    assert used.finish([1])[0] == dec.decode([long_])
    fresh = dec.online_bigram(3, window=window, times=True, wide="settle")
    assert serve(used, 1, short, 3) == serve(fresh, 1, short, 3)
    (wu, iu), (wf, i_f) = used.finish([1]), fresh.finish([1])
    assert wu == wf == dec.decode([short])
    np.testing.assert_array_equal(iu["end_cost"], i_f["end_cost"])
    np.testing.assert_array_equal(iu["best_end"], i_f["best_end"])
    used.close()
    fresh.close()


def test_refusals(R, hip, ctx):
    """Through the real library: the graph forms gh_online_create_bigram_wide_settle does not take (the reasons of
    gh_online_create_bigram_wide under its own name), a push past the window, gh_online_result on a windowed session, paths,
    and `wide=True`, which still refuses a window."""
    from sr.recognition.continuous_speech import packed_lattice, packed_loop_lattice, packed_bigram_lattice
    case = make_case(17, 3, False, seed=3)
    dec = decoder_of(R, ctx, case)
    wt, n, Bw, initw = case["trans"], case["n"], case["B"], case["init"]
    wide_graph = lambda: packed_bigram_lattice(wt, n, Bw, initw)[0]
    for graphs, match, prepare in (([packed_bigram_lattice(wt[:16], n, Bw[:16, :16], initw[:16])[0]], "gh_online_create_bigram takes it", None),
                                   ([packed_loop_lattice(wt, n, 0.0)[0]], "gh_online_create_wide takes it", None),
                                   ([packed_loop_lattice(wt[:16], n, 0.0)[0]], "gh_online_create takes it", None),
                                   ([packed_lattice(wt, n, [list(range(17))] * 2)[0]], "K-layer", None),
                                   ([wide_graph()], "beam", lambda lat: lat.set_beam(3)),
                                   ([wide_graph(), packed_bigram_lattice(wt, n, Bw + 1.0, initw)[0]], "several graphs", None)):
        lat = hip.Lattices(ctx, graphs)
        if prepare:
            prepare(lat)
        for kw in (dict(max_frames=10, settle=True), dict(window=10)):
            with pytest.raises(hip.Unsupported, match=match) as e:
                hip.OnlineBigramWideSession(ctx, lat, 4, **kw)
            assert "gh_online_create_bigram_wide_settle" in str(e.value)
        lat.close()
    with pytest.raises(ValueError):
        hip.OnlineBigramWideSession(ctx, dec.lat, 3)
    with pytest.raises(ValueError):
        hip.OnlineBigramWideSession(ctx, dec.lat, 3, max_frames=10, window=10)
    for kw in (dict(window=10), dict(max_frames=10, settle=True)):        # the older keyword keeps its refusal
        with pytest.raises(hip.Unsupported, match="not built yet"):
            dec.online_bigram(4, wide=True, **kw)
    with pytest.raises(ValueError, match="wide"):
        dec.online_bigram(4, max_frames=10, wide="window")
    with pytest.raises(hip.Unsupported, match="not in bigram form"):      # ... and without the permission: as before
        dec.online_bigram(4, window=10)
    x = [case["synth"](case["rng"].integers(0, 17, size=20)) for _ in range(3)]
    window = 40
    on = dec.online_bigram(n_streams=3, window=window, times=True, wide="settle")
    on.push([2, 0], [x[2][:window], x[0][:4]])                            # exactly the window is fine
    before = on.result()
    b = hip.Batch(ctx, [x[1][:3], x[2][window:window + 1]])
    b.loglik(dec.gmm, fetch=False)
    s = on.session
    with pytest.raises(ValueError, match="stream 2"):                     # through the decoder: before the GPU is touched
        on.push([1, 2], [x[1][:3], x[2][window:window + 1]])
    with pytest.raises(hip.BackendError, match="stream 2"):               # the binding itself: stream 1 must not move either
        s.push(b, [1, 2])
    for bad in ([3], [-1]):
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
        on.result([2], want_path=True)                                    # a windowed decoder offers no paths
    with pytest.raises(ValueError):
        on.finish([2], want_path=True)
    with pytest.raises(hip.Unsupported, match="tail"):                    # gh_online_result on a windowed session
        s.result([2])
    new = on.commit([2])                                                  # a commit moves the window on
    words, frames = on.settled([2])
    assert words == new and frames[0] > 0 and len(words[0]) >= 1 and len(on.settled_times([2])[0]) == len(words[0])
    on.push([2], [x[2][window:window + int(frames[0])]])
    assert on.frames[2] == window + frames[0]
    on.reset([2])
    assert on.settled([2])[0] == [[]] and on.settled([2])[1].tolist() == [0] and on.frames[2] == 0
    on.close()
    b.close()
    # a full-history session that settles still gives paths; the plain one still refuses commit and tail
    row_word = np.where(dec.row_state >= 0, dec.row_state // n, -1).astype(np.int32)
    st = hip.OnlineBigramWideSession(ctx, dec.lat, 2, 40, settle=True)
    assert st.settles and st.window is None and st.max_frames == 40
    st.close()
    plain = hip.OnlineBigramWideSession(ctx, dec.lat, 2, 40)
    assert not plain.settles
    for call in (plain.commit, plain.tail):
        with pytest.raises(hip.Unsupported, match="does not settle"):
            call([0], row_label=row_word)
    plain.close()


W17, N17, M17, D17 = 17, 3, 2, 39


def test_push_recording_through_a_windowed_wide_bigram_decoder(R, hip, ctx):
    """A 17-word model (39 features) under a bigram grammar behind a StreamingFrontend and a StreamingEndpointer with
    `window=, wide="settle"`: a commit after every tick, and the utterances equal offline trim_ranges + decode_batch --
    ranges, words and word begins."""
    import sr.audio_capture as AC
    import stream_endpoints_ref as S
    from sr.feature import StreamingFrontend, feature_stats, features_from_signals
    from sr.recognition.batch import ContinuousDecoder
    rng = np.random.default_rng(1703)
    means, vars_, w = make_model(rng, W17, N17, m=M17, d=D17)
    hmms = [make_hmm(R, means[i], vars_[i], w[i], word_trans(rng, N17)) for i in range(W17)]
    Bw, initw = random_costs(rng, W17, 0.1)
    dec = ContinuousDecoder(hmms, grammar="bigram", bigram=Bw, initial=initw, ctx=ctx)
    assert "bigram_wide" in dec.lat.forms()
    rate = 16000
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
    ep = AC.StreamingEndpointer(2, cfg, max_chunk=TICK)
    fe = StreamingFrontend(2, rate, normalize=norm, max_chunk=ep.max_piece)
    on = dec.online_bigram(2, window=longest, frontend=fe, endpointer=ep, times=True, wide="settle")
    assert isinstance(on.session, hip.OnlineBigramWideSession) and on.session.window == longest and on.settles
    got = [[], []]
    for ids, chunks, end in ticks_of(sigs):
        for u in on.push_recording(ids, chunks, end):
            got[u["stream"]].append(u)
    for r in range(2):
        assert [(u["begin"], u["stop"], u["open"], u["words"], u["begins"]) for u in got[r]] == offline[r], r
        assert len(got[r]) >= 1 and all(len(u["words"]) >= 1 for u in got[r])
    assert on.frames.tolist() == [0, 0]
    on.close(); fe.close(); ep.close()
