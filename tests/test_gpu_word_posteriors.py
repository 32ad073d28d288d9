# -*- coding: utf-8 -*-
"""Word posteriors and per-word confidence on the device: gh_word_posteriors (csrc/gh_fb_loop.hip),
`Lattices.word_posteriors`, `ContinuousDecoder.word_posteriors` and `decode_batch(..., want_confidence=True)`.

Every case feeds tiny models (D = 3, 2 mixtures) and at most 60 frames per utterance.  Both sides of a comparison work on
the device's own likelihood matrix (`b.loglik(gmm, fetch=True)`; an fp32 batch: the fp32 values widened), so likelihood
error never enters.  Tolerances: posteriors and confidences rtol 1e-8 with atol 1e-10, log P rtol 1e-10 -- the project's
bounds for gamma-derived sums and log P against `O.forward_backward` (`_close` in tests/test_gpu_em_strings.py); "sums to
one" follows from them: |sum_w post[t] - 1| <= W 1e-10 + 2e-8.

  1. every N = 2 .. 8 with and without skip arcs, both dtypes, W over {1, 3, 16, 17, 33, 64} in a rotating table, 9 ragged
     utterances, word_penalty = 0: post, logp and the confidences of the decode's own words against the restatement
     (tests/word_posteriors_ref.py);
  2. against the generic kernel: q from `forward_backward(want_matrices=True)`'s alpha, beta and log P;
  3. T = 1, T = 2 and T < N beside long utterances;
  4. not vacuous: the per-word sum of gamma exceeds 1.05 where post sums to one; word_penalty = 50;
  5. frames scaled by 1e3 (costs of order 1e6);
  6. chunking (>= 3 launches) and 7. batch position: bitwise the same;
  8. `decode_batch(b, want_confidence=True)` and `decode(xs, want_confidence=True)`;
  9. refusals through the real library."""
import numpy as np
import pytest

from oracle import ref_numpy as O
from word_posteriors_ref import confidence, word_posteriors

pytestmark = pytest.mark.gpu

M_, D_ = 2, 3
RTOL, ATOL, RTOL_LOGP = 1e-8, 1e-10, 1e-10
#         W   n  skip
CASES = [(64, 2, False),
         (1, 2, False),
         (33, 3, False),
         (17, 3, True),
         (33, 4, False),
         (16, 4, True),
         (17, 5, False),
         (3, 5, True),
         (16, 6, False),
         (1, 6, True),
         (17, 7, False),
         (3, 7, True),
         (16, 8, False),
         (17, 8, True)]
CASE_IDS = ["W%d-n%d-%s" % (c[0], c[1], "skip" if c[2] else "plain") for c in CASES]
RAGGED = tuple(60 - 7 * u for u in range(9))                              # 60, 53, ... 4


def word_trans(rng, n, skip):
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = rng.uniform(0.1, 2.0)
        if i < n - 1:
            t[i + 1, i] = rng.uniform(0.1, 2.0)
        if skip and i < n - 2:
            t[i + 2, i] = rng.uniform(0.1, 2.0)
    return t


def make_case(W, n, skip, penalty=0.0, T=RAGGED, seed=0, scale=1.0):
    rng = np.random.default_rng(9000 + 100 * W + 10 * n + skip + seed)
    means = rng.normal(size=(W, n, M_, D_)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M_, D_))
    w = rng.dirichlet(np.ones(M_), size=(W, n))
    trans = [word_trans(rng, n, skip) for _ in range(W)]
    xs = [rng.normal(size=(t, D_)) * 2.0 * scale for t in T]
    nes, rw, rs, dense, ends = O.loop_grammar(trans, n, penalty)
    return dict(W=W, n=n, skip=skip, penalty=penalty, means=means, vars=vars_, w=w, trans=trans, xs=xs, T=np.array(T),
                nes=nes, rw=rw, rs=rs, dense=dense, ends=ends)


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


def decoder_of(R, ctx, case, dtype=np.float64, **kw):
    from sr.recognition.batch import ContinuousDecoder
    hmms = [make_hmm(R, case["means"][i], case["vars"][i], case["w"][i], case["trans"][i]) for i in range(case["W"])]
    kw.setdefault("grammar", "loop")
    if kw["grammar"] == "loop":
        kw.setdefault("word_penalty", case["penalty"])
    dec = ContinuousDecoder(hmms, dtype=dtype, ctx=ctx, **kw)
    if kw["grammar"] == "loop":
        np.testing.assert_array_equal(dec.row_state, np.where(case["nes"], -1, case["rw"] * case["n"] + case["rs"]))
        assert list(dec.lat.end_rows[0]) == list(case["ends"])
    return dec


def emissions(case, nll):
    col = np.where(case["nes"], 0, case["rw"] * case["n"] + case["rs"])
    return np.where(case["nes"][:, None], 0.0, np.asarray(nll, dtype=np.float64)[:, col].T)


def restate(case, nll):
    """[(post [T, W], logp)] of every utterance from the device's own likelihood matrix."""
    off = np.concatenate([[0], np.cumsum(case["T"])])
    return [word_posteriors(emissions(case, nll[off[u]:off[u + 1]]), case["nes"], case["rw"], case["dense"], case["ends"],
                            case["W"], case["n"]) for u in range(len(case["T"]))]


def close_logp(got, want):
    got, want = np.asarray(got), np.asarray(want)
    inf = np.isinf(want)
    np.testing.assert_array_equal(got[inf], want[inf])
    np.testing.assert_allclose(got[~inf], want[~inf], rtol=RTOL_LOGP, atol=0)


def check_against(case, ref, post, logp, conf=None, words=None, begins=None, sums_to_one=True):
    off = np.concatenate([[0], np.cumsum(case["T"])])
    W = case["W"]
    assert post.shape == (off[-1], W) and np.isfinite(post).all()
    close_logp(logp, [r[1] for r in ref])
    worst = 0.0
    for u, (p, lp) in enumerate(ref):
        got = post[off[u]:off[u + 1]]
        worst = max(worst, float(np.max(np.abs(got - p) / (ATOL + RTOL * np.abs(p)), initial=0.0)))
        if np.isinf(lp):
            assert not got.any()
        elif sums_to_one:
            assert np.max(np.abs(got.sum(axis=1) - 1.0)) <= W * 1e-10 + 2e-8
        if conf is not None:
            want = confidence(p, words[u], begins[u], case["T"][u])
            assert conf[u].shape == want.shape and conf[u].dtype == np.float64
            worst = max(worst, float(np.max(np.abs(conf[u] - want) / (ATOL + RTOL * np.abs(want)), initial=0.0)))
            if np.isinf(lp):
                assert not conf[u].any()
    print("worst error / tolerance: %.3g" % worst)
    for u, (p, lp) in enumerate(ref):
        np.testing.assert_allclose(post[off[u]:off[u + 1]], p, rtol=RTOL, atol=ATOL)
        if conf is not None:
            np.testing.assert_allclose(conf[u], confidence(p, words[u], begins[u], case["T"][u]), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", CASES, ids=CASE_IDS)
def test_every_instantiation_against_the_restatement(R, hip, ctx, shape, dtype):
    case = make_case(*shape)
    dec = decoder_of(R, ctx, case, dtype)
    assert "loop" in dec.lat.forms()
    b = hip.Batch(ctx, case["xs"], dtype=dtype)
    nll = b.loglik(dec.gmm, fetch=True)
    ref = restate(case, nll)
    words, r = dec.decode_batch(b, want_confidence=True)
    post, logp = dec.word_posteriors(b)
    assert ctx.last_chunks == 1
    np.testing.assert_array_equal(logp, r["logp"])
    assert sum(len(w) for w in words) >= len(words) - 2                   # the confidences are not checked on nothing
    assert sum(np.isfinite(lp) for _, lp in ref) >= 7
    check_against(case, ref, post, logp, r["confidence"], words, r["begins"])
    for u, c in enumerate(r["confidence"]):
        assert np.all(c >= 0.0) and np.all(c <= 1.0 + 1e-9)
    b.close()


def q_from_matrices(case, alpha, beta, logp):
    W, n = case["W"], case["n"]
    Lr = 1 + W * (n - 1)
    T = alpha.shape[1]
    post = np.zeros((T, W))
    if np.isinf(logp):
        return post
    with np.errstate(invalid="ignore"):
        gamma = np.exp(alpha + beta - logp)
    gamma[np.isnan(gamma)] = 0.0
    for w in range(W):
        last = 1 + w * (n - 1) + (n - 2)
        leave = np.exp(alpha[last] - case["dense"][Lr, last] + beta[Lr] - logp)
        leave[np.isnan(leave)] = 0.0
        post[:, w] = gamma[case["rw"] == w].sum(axis=0) - leave
    return np.maximum(post, 0.0)


@pytest.mark.parametrize("shape", [(3, 3, False), (16, 5, True), (17, 2, False)], ids=["3x3", "16x5-skip", "17x2"])
def test_against_the_generic_kernel(R, hip, ctx, shape):
    case = make_case(*shape, seed=1)
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, case["xs"])
    b.loglik(dec.gmm, fetch=False)
    fb = dec.lat.forward_backward(b, want_matrices=True)
    post, logp = dec.word_posteriors(b)
    close_logp(logp, fb["logp"])
    off = np.concatenate([[0], np.cumsum(case["T"])])
    for u in range(len(case["T"])):
        want = q_from_matrices(case, fb["alpha"][u], fb["beta"][u], fb["logp"][u])
        np.testing.assert_allclose(post[off[u]:off[u + 1]], want, rtol=RTOL, atol=ATOL)
    b.close()


@pytest.mark.parametrize("shape", [(3, 2, False), (17, 4, True), (5, 8, False)], ids=["3x2", "17x4-skip", "5x8"])
def test_short_utterances_beside_long_ones(R, hip, ctx, shape):
    n = shape[1]
    T = (40, 1, 2, n - 1, 33, 1, n, 2)
    case = make_case(*shape, T=T, seed=2)
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, case["xs"])
    nll = b.loglik(dec.gmm, fetch=True)
    ref = restate(case, nll)
    assert np.isinf(ref[1][1]) and np.isinf(ref[5][1]) and np.isfinite(ref[0][1]) and np.isfinite(ref[4][1])
    # a span table of our own: one word from frame 0 in every utterance, also where there is no path
    labels = [[u % case["W"]] for u in range(len(T))]
    begins = [[0]] * len(T)
    r = dec.lat.word_posteriors(b, labels=labels, begins=begins)
    assert np.isfinite(r["post"]).all()
    check_against(case, ref, r["post"], r["logp"], r["confidence"], labels, begins)
    for u, (p, lp) in enumerate(ref):
        if np.isinf(lp):
            assert r["logp"][u] == -np.inf and r["confidence"][u].tolist() == [0.0]
    # ... and the decode's own words
    words, rd = dec.decode_batch(b, want_confidence=True)
    check_against(case, ref, r["post"], rd["logp"], rd["confidence"], words, rd["begins"])
    b.close()


def test_not_vacuous_and_a_word_penalty(R, hip, ctx):
    case = make_case(5, 3, True, penalty=0.0, seed=3)
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, case["xs"])
    nll = b.loglik(dec.gmm, fetch=True)
    fb = dec.lat.forward_backward(b, want_matrices=True)
    post, logp = dec.word_posteriors(b)
    off = np.concatenate([[0], np.cumsum(case["T"])])
    most = 0.0
    for u in range(len(case["T"])):
        if np.isfinite(logp[u]):
            per_frame = fb["gamma"][u][~case["nes"]].sum(axis=0)         # what `occ` summed over the states gives
            most = max(most, float(per_frame.max()))
            assert np.max(np.abs(post[off[u]:off[u + 1]].sum(axis=1) - 1.0)) <= case["W"] * 1e-10 + 2e-8
    assert most > 1.05
    check_against(case, restate(case, nll), post, logp)
    b.close()
    case = make_case(5, 3, True, penalty=50.0, seed=3)
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, case["xs"])
    nll = b.loglik(dec.gmm, fetch=True)
    words, r = dec.decode_batch(b, want_confidence=True)
    post, logp = dec.word_posteriors(b)
    check_against(case, restate(case, nll), post, logp, r["confidence"], words, r["begins"])
    b.close()


def test_costs_of_order_a_million(R, hip, ctx):
    """Under the reference's linear-domain underflow rule (a context's default) a cost above 745 is +inf and such frames have
    no path at all; set_compat(underflow=False) keeps the likelihoods in the log domain, where these costs are finite.
    What is asked here is agreement with the restatement.  "Sums to one" is not: log P is of order -1e8 here, one unit in its
    last place 1.5e-8 to 3e-8, and gamma = exp(la + lb - logP) of a certain cell comes out as 1 + 1.5e-7 in the restatement
    as on the device (both deviations are printed; on an MI355X: 1.49e-07 and 1.49e-07) -- the rounding of the definition,
    not of one side."""
    case = make_case(4, 4, True, T=(60, 31, 17), seed=4, scale=1e3)
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, case["xs"])
    ctx.set_compat(underflow=False)
    try:
        nll = b.loglik(dec.gmm, fetch=True)
        assert np.isfinite(nll).all() and np.median(nll) > 1e5
        words, r = dec.decode_batch(b, want_confidence=True)
        post, logp = dec.word_posteriors(b)
    finally:
        ctx.set_compat(underflow=True)
    assert np.isfinite(logp).all() and not np.isnan(post).any() and all(len(w) >= 1 for w in words)
    ref = restate(case, nll)
    print("restatement, max |sum_w q - 1|: %.3g; device: %.3g" % (max(np.max(np.abs(p.sum(axis=1) - 1.0)) for p, _ in ref),
                                                                   np.max(np.abs(post.sum(axis=1) - 1.0))))
    check_against(case, ref, post, logp, r["confidence"], words, r["begins"], sums_to_one=False)
    b.close()


def test_chunked_launches_give_the_same_bits(R, hip, ctx, monkeypatch):
    case = make_case(17, 3, True, seed=5)
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, case["xs"])
    monkeypatch.delenv("GMMHMM_SCRATCH_BUDGET", raising=False)
    words, r = dec.decode_batch(b, want_confidence=True)
    one = dec.lat.word_posteriors(b, labels=r["labels"], begins=r["begins"])
    assert ctx.last_chunks == 1
    # alpha scratch: 8 T n W bytes per utterance -- 24 KB for the longest; the batch takes 118 KB
    monkeypatch.setenv("GMMHMM_SCRATCH_BUDGET", "40K")
    cut = dec.lat.word_posteriors(b, labels=r["labels"], begins=r["begins"])
    assert ctx.last_chunks >= 3, ctx.last_chunks
    monkeypatch.delenv("GMMHMM_SCRATCH_BUDGET")
    np.testing.assert_array_equal(cut["post"], one["post"])
    np.testing.assert_array_equal(cut["logp"], one["logp"])
    for a, c, d in zip(one["confidence"], cut["confidence"], r["confidence"]):
        np.testing.assert_array_equal(c, a)
        np.testing.assert_array_equal(d, a)
    b.close()


def test_batch_position_does_not_matter(R, hip, ctx):
    case = make_case(17, 4, False, seed=6)
    dec = decoder_of(R, ctx, case)
    xs = case["xs"]
    x = xs[2]

    def run(batch_xs, u):
        b = hip.Batch(ctx, batch_xs)
        words, r = dec.decode_batch(b, want_confidence=True)
        post, logp = dec.word_posteriors(b)
        o = int(b.offsets[u])
        out = (post[o:o + len(x)].copy(), logp[u], r["confidence"][u].copy(), words[u])
        b.close()
        return out
    alone, first, last = run([x], 0), run([x] + xs[:2] + xs[3:], 0), run(xs[:2] + xs[3:] + [x], len(xs) - 1)
    assert len(alone[3]) >= 1
    for other in (first, last):
        np.testing.assert_array_equal(other[0], alone[0])
        assert other[1] == alone[1] and other[3] == alone[3]
        np.testing.assert_array_equal(other[2], alone[2])


def test_decode_batch_with_confidence(R, hip, ctx):
    case = make_case(16, 5, False, seed=7)
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, case["xs"])
    plain_words, plain = dec.decode_batch(b)
    timed_words, timed = dec.decode_batch(b, want_times=True)
    words, r = dec.decode_batch(b, want_confidence=True)
    assert words == timed_words == plain_words
    for key in ("end_cost_flat", "best_end", "n_labels", "label_off"):
        np.testing.assert_array_equal(r[key], timed[key])
    for u in range(len(case["T"])):                                       # (the slots behind n_labels are not written)
        np.testing.assert_array_equal(r["labels"][u], timed["labels"][u])
    post, logp = dec.word_posteriors(b)
    np.testing.assert_array_equal(r["logp"], logp)
    off = np.concatenate([[0], np.cumsum(case["T"])])
    for u in range(len(case["T"])):
        np.testing.assert_array_equal(r["begins"][u], timed["begins"][u])
        want = confidence(post[off[u]:off[u + 1]], words[u], r["begins"][u], case["T"][u])
        np.testing.assert_allclose(r["confidence"][u], want, rtol=1e-13, atol=1e-15)   # the same q, summed in the other order
    w2, b2, c2 = dec.decode(case["xs"], want_confidence=True)
    assert w2 == words
    for u in range(len(case["T"])):
        np.testing.assert_array_equal(b2[u], r["begins"][u])
        np.testing.assert_array_equal(c2[u], r["confidence"][u])
    again_words, again = dec.decode_batch(b)
    assert again_words == plain_words and sorted(again) == sorted(plain) and "confidence" not in again
    for key in ("end_cost_flat", "best_end", "n_labels"):
        np.testing.assert_array_equal(again[key], plain[key])
    for u in range(len(case["T"])):
        np.testing.assert_array_equal(again["labels"][u], plain["labels"][u])
    b.close()


def test_refusals_through_the_library(R, hip, ctx):
    rng = np.random.default_rng(8)
    small = make_case(3, 3, False, seed=8)
    wide = make_case(17, 2, False, seed=8)
    xs = small["xs"][:2]

    def refused(dec, hint):
        b = hip.Batch(ctx, xs)
        b.loglik(dec.gmm, fetch=False)
        with pytest.raises(hip.Unsupported, match=hint) as e:
            dec.lat.word_posteriors(b)
        b.close()
        return str(e.value)
    sentences = [refused(decoder_of(R, ctx, small, grammar="bigram", bigram=rng.uniform(0.0, 3.0, size=(3, 3))), "in bigram form"),
                 refused(decoder_of(R, ctx, wide, grammar="bigram", bigram=rng.uniform(0.0, 3.0, size=(17, 17))), "wide bigram form"),
                 refused(decoder_of(R, ctx, small, grammar="layers", n_layers=2), "K-layer lattice"),
                 refused(decoder_of(R, ctx, make_case(2, 12, False, seed=8)), "12 states")]
    beamed = decoder_of(R, ctx, small)
    beamed.lat.set_beam(3)
    sentences.append(refused(beamed, "rank beam"))
    assert len(set(sentences)) == 5
    # argument errors: nothing is written
    dec = decoder_of(R, ctx, small)
    b = hip.Batch(ctx, xs)
    with pytest.raises(hip.BackendError, match="gh_loglik has not been run") as e:
        dec.lat.word_posteriors(b)
    assert not isinstance(e.value, hip.Unsupported)
    b.loglik(dec.gmm, fetch=False)
    T0 = len(xs[0])
    import ctypes as C
    lib = ctx.lib
    f64p, i32p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    p = lambda a, t: a.ctypes.data_as(t)
    good = dict(labels=np.array([0, 2, 1, 0], dtype=np.int32), begins=np.array([0, 5, 0, 9], dtype=np.int32),
                off=np.array([0, 2, 4], dtype=np.int64), nl=np.array([2, 2], dtype=np.int32))
    bad = [("outside \\[0, 3\\)", dict(labels=np.array([0, 3, 1, 0], dtype=np.int32))),
           ("begin %d outside" % T0, dict(begins=np.array([0, T0, 0, 9], dtype=np.int32))),
           ("do not strictly increase", dict(begins=np.array([0, 5, 9, 9], dtype=np.int32))),
           ("beyond the slot", dict(nl=np.array([2, 3], dtype=np.int32)))]
    for hint, change in bad:
        a = dict(good, **change)
        logp, post, conf = np.full(2, 7.0), np.full((b.N, 3), 7.0), np.full(4, 7.0)
        rc = lib.gh_word_posteriors(ctx.h, dec.lat.h, b.h, p(logp, f64p), p(post, f64p), p(a["labels"], i32p), p(a["begins"], i32p),
                                    p(a["off"], i64p), p(a["nl"], i32p), p(conf, f64p))
        assert rc == -1, hint
        import re
        assert re.search(hint, lib.gh_last_error().decode()), lib.gh_last_error()
        assert np.all(logp == 7.0) and np.all(post == 7.0) and np.all(conf == 7.0)
    logp, post, conf = np.full(2, 7.0), np.full((b.N, 3), 7.0), np.full(4, 7.0)
    rc = lib.gh_word_posteriors(ctx.h, dec.lat.h, b.h, p(logp, f64p), p(post, f64p), p(good["labels"], i32p), p(good["begins"], i32p),
                                p(good["off"], i64p), p(good["nl"], i32p), p(conf, f64p))
    assert rc == 0 and np.all(logp != 7.0) and np.all(post != 7.0) and np.all(conf != 7.0)
    b.close()
