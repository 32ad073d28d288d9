# -*- coding: utf-8 -*-
"""The end costs and the chosen end of an online session (online_end_kernel<LANES, BIGRAM_ROWS> in csrc/gh_online.hip, behind
gh_online_result and gh_online_tail) in all four session forms, at EXACT TIES across word lanes.

Graph: N = 2 states per word; W = 3 (narrow loop, narrow bigram) or W = 17 (wide loop, wide bigram); words 0 and W - 1 are
the SAME model -- the same transitions and emission states, and in the bigram forms the same word-to-word and start costs --
so their cells cost exactly the same in every column and their end costs are equal bit for bit.  They sit in different lanes,
at W = 17 in different 16-lane rows.  Every stream hears word 0, so the two are the best ends.
Streams: five in one session (a narrow form launches a second block with one live row) that have taken 0, 1, 2, 5 and 5
frames; the last two take the same five frames as `5` and as `2 + 0 + 3`.
Asserted, for fp64 and fp32 likelihoods:
  * `result()`: end_cost and best_end are bitwise those of the one-shot `viterbi` on the same likelihood matrix;
  * both equal oracle.ref_numpy.decode_states on that matrix -- best_end equal, end_cost bitwise (fp32 likelihoods: 1e-5, the
    tolerance of tests/test_gpu_online.py);
  * the stream without frames gives +inf everywhere and -1;
  * `tail()` of the session that settles gives the same end_cost and best_end;
  * NOT VACUOUS, from the oracle's numbers alone: in a stream of every form the minimum end cost is finite and attained by two
    end slots, and the chosen end is the larger slot."""
import numpy as np
import pytest

from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu

N, M, D = 2, 2, 5
FORMS = {"loop": ("loop", 3), "bigram": ("bigram", 3), "wide": ("loop", 17), "bigram_wide": ("bigram", 17)}
LENGTHS = [1, 2, 5, 5]                                    # the batch's utterances: streams 1 .. 4 (stream 0 takes nothing)


def make_case(form):
    """Model, graph and frames.  No GPU."""
    from sr.recognition.continuous_speech import packed_bigram_lattice, packed_loop_lattice
    grammar, W = FORMS[form]
    rng = np.random.default_rng(9100 + W + 100 * (grammar == "bigram"))
    means = rng.normal(size=(W, N, M, D)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, N, M, D))
    w = rng.dirichlet(np.ones(M), size=(W, N))
    trans = []
    for _ in range(W):
        t = np.full((N, N), np.inf)
        t[0, 0], t[1, 0], t[1, 1] = rng.uniform(0.05, 0.6), rng.uniform(0.8, 2.5), rng.uniform(0.0, 0.3)
        trans.append(t)
    means[W - 1], vars_[W - 1], w[W - 1], trans[W - 1] = means[0], vars_[0], w[0], trans[0].copy()
    B = init = None
    if grammar == "bigram":
        B, init = rng.uniform(0.0, 4.0, size=(W, W)), rng.uniform(0.0, 2.0, size=W)
        B[:, W - 1] = B[:, 0]
        B[W - 1, :] = B[0, :]
        init[W - 1] = init[0]
        graph = packed_bigram_lattice(trans, N, B, init)[0]
    else:
        graph = packed_loop_lattice(trans, N, 0.7)[0]
    five = means[0, [0, 0, 1, 1, 1], rng.integers(0, M, size=5)] + 0.3 * rng.normal(size=(5, D))
    xs = [five[:1].copy(), five[[0, 2]].copy(), five, five.copy()]
    assert [len(x) for x in xs] == LENGTHS
    R_ = len(graph["row_state"])
    dense = np.full((R_, R_), np.inf)
    dense[graph["arc_to"], graph["arc_from"]] = graph["arc_cost"]
    return dict(form=form, grammar=grammar, W=W, means=means, vars=vars_, w=w, trans=trans, B=B, init=init, graph=graph, xs=xs,
                dense=dense, nes=graph["row_state"] < 0, ends=[int(e) for e in graph["end_rows"]])


def oracle_ends(case, nll):
    """(end_cost [n_end], best_end) of decode_states on the rows [T, S] of a likelihood matrix."""
    col = np.where(case["nes"], 0, case["graph"]["row_state"])
    E = np.where(case["nes"][:, None], 0.0, np.asarray(nll, dtype=np.float64)[:, col].T)
    T = E.shape[1]
    costs, _, end, _ = O.decode_states(E, case["nes"], case["dense"], end_points=[[e, T - 1] for e in case["ends"]], return_bp=True)
    return costs[case["ends"], T - 1], case["ends"].index(end[0])


def assert_tied(case, ref):
    """The input condition: some stream's minimum end cost is finite, two end slots attain it, the larger one is chosen."""
    slots = [case["ends"].index(r) for r in case["ends"]]
    assert slots == sorted(slots)
    tied = []
    for ec, be in ref:
        at_min = np.flatnonzero(ec == ec.min())
        if np.isfinite(ec.min()) and len(at_min) == 2:
            assert be == at_min.max() and be != at_min.min()
            tied.append(at_min)
    assert tied, [ec for ec, _ in ref]
    assert any(a[0] // 16 != a[1] // 16 for a in tied) or case["W"] <= 16      # W = 17: the two lanes lie in different 16-lane rows


@pytest.mark.parametrize("form", list(FORMS))
def test_the_oracle_ties_two_end_slots(form):
    """The oracle half of the input condition on the oracle's own fp64 likelihoods: it needs no device (it carries the
    module's mark and runs with the GPU suite; the device tests below assert the same on the device's matrix)."""
    case = make_case(form)
    S = case["W"] * N
    ref = [oracle_ends(case, O.gmm_neg_loglik_batch(x, case["means"].reshape(S, M, D), case["vars"].reshape(S, M, D),
                                                    case["w"].reshape(S, M))) for x in case["xs"]]
    assert_tied(case, ref)


@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


def sessions_of(hip, ctx, lat, form):
    """(a session with full history that does not settle where the form offers one, one that settles)."""
    cls = dict(loop=hip.OnlineSession, bigram=hip.OnlineBigramSession, wide=hip.OnlineWideSession,
               bigram_wide=hip.OnlineBigramWideSession)[form]
    if form == "loop":
        return cls(ctx, lat, 5, max_frames=5), cls(ctx, lat, 5, max_frames=5)
    return cls(ctx, lat, 5, max_frames=5), cls(ctx, lat, 5, max_frames=5, settle=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("form", list(FORMS))
def test_end_costs_and_chosen_end_at_exact_ties(hip, form, dtype):
    import sr.recognition as R
    from sr.recognition.batch import ContinuousDecoder
    from test_gpu_online import make_hmm
    ctx = hip.default_context()
    case = make_case(form)
    W = case["W"]
    hmms = [make_hmm(R, case["means"][i], case["vars"][i], case["w"][i], case["trans"][i]) for i in range(W)]
    if case["grammar"] == "bigram":
        dec = ContinuousDecoder(hmms, grammar="bigram", bigram=case["B"], initial=case["init"], dtype=dtype, ctx=ctx)
    else:
        dec = ContinuousDecoder(hmms, grammar="loop", word_penalty=0.7, dtype=dtype, ctx=ctx)
    assert {"loop": "loop", "bigram": "bigram", "wide": "loop", "bigram_wide": "bigram_wide"}[form] in dec.lat.forms()
    np.testing.assert_array_equal(dec.row_state, case["graph"]["row_state"])
    assert list(dec.lat.end_rows[0]) == case["ends"]
    n_end = len(case["ends"])
    b = hip.Batch(ctx, case["xs"], dtype=dtype)
    nll = np.asarray(b.loglik(dec.gmm, fetch=True), dtype=np.float64)    # the matrix all three sides decode
    off = np.concatenate([[0], np.cumsum(LENGTHS)])
    ref = [oracle_ends(case, nll[off[u]:off[u + 1]]) for u in range(4)]
    assert_tied(case, ref)                                                # before the device is looked at
    one = dec.lat.viterbi(b, want_path=False)
    one_cost, one_best = np.asarray(one["end_cost_flat"]).reshape(4, n_end), np.asarray(one["best_end"])
    ids = np.arange(1, 5)
    for on in sessions_of(hip, ctx, dec.lat, form):
        # streams 1 .. 3 whole; stream 4 as 2 + 0 + 3
        on.push(b, ids, first=[0, 0, 0, 0], count=[1, 2, 5, 2])
        on.push(b, ids, first=[1, 2, 5, 2], count=[0, 0, 0, 0])
        on.push(b, ids, first=[1, 2, 5, 2], count=[0, 0, 0, 3])
        np.testing.assert_array_equal(on.frames(), [0] + LENGTHS)
        outs = [on.result()]
        if getattr(on, "settles", True):
            outs.append(on.tail())
        for out in outs:
            print(form, dtype.__name__, "best_end", out["best_end"], "oracle", [be for _, be in ref])
            assert np.all(np.isposinf(out["end_cost"][0])) and out["best_end"][0] == -1      # no frames
            np.testing.assert_array_equal(out["end_cost"][1:], one_cost)                       # bitwise the one-shot decode
            np.testing.assert_array_equal(out["best_end"][1:], one_best)
            np.testing.assert_array_equal(out["end_cost"][3], out["end_cost"][4])              # 5 == 2 + 0 + 3
            for u, (ec, be) in enumerate(ref):
                assert out["best_end"][1 + u] == be
                if dtype == np.float64:
                    np.testing.assert_array_equal(out["end_cost"][1 + u], ec)
                else:
                    np.testing.assert_allclose(out["end_cost"][1 + u], ec, rtol=1e-5)
        on.close()
    b.close()
