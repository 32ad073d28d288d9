# -*- coding: utf-8 -*-
"""Word posteriors and per-word confidence under the bigram grammar on the device: gh_word_posteriors_bigram
(csrc/gh_fb_bigram.hip), `Lattices.word_posteriors_bigram` and the `lm=True` permission of `ContinuousDecoder`.

Every case feeds tiny models (D = 3, 2 mixtures) and at most 60 frames per utterance, 9 ragged utterances of 60 - 7u
frames.  Both sides of a comparison work on the device's own likelihood matrix (`b.loglik(gmm, fetch=True)`; an fp32
batch: the fp32 values widened), so likelihood error never enters.  The restatement is `sweep` of
tests/word_posteriors_bigram_ref.py (the recursion of `O.forward_backward` written per column; the host tests hold it to
the row-by-row formula and to brute-force enumeration at 1e-12).  Tolerances: the project's own for these quantities
(tests/test_gpu_word_posteriors.py) -- posteriors and confidences rtol 1e-8 with atol 1e-10, log P rtol 1e-10; log P is
-inf exactly where the restatement's is.

  1. every N = 2 .. 8 with and without skip arcs, both dtypes, W over {2, 3, 16, 17, 33, 64} in a rotating table, dense
     random B and initial: the decode's own words, post, logp and confidences;
  2. sparse language models at 17 and 64 words: forbidden pairs, a word that can only start, one that can only end, a
     word whose only predecessor lies 800 below the wave's maximum in another quarter of the wave, and a graph with every
     pair and all but one start forbidden;
  3. constant costs against the loop-form kernel; 4. against the generic kernel; 5. short utterances;
  6. frames scaled by 1e3, the bound from the restatement's own rounding (fp64 against np.longdouble);
  7. batches of 1, 4, 5 and 9 utterances (blocks hold four), batch position and chunked launches: bitwise the same;
  8. `decode_batch(b, want_confidence=True, lm=True)` and `decode(xs, want_confidence=True, lm=True)`;
  9. refusals through the real library."""
import re

import numpy as np
import pytest

from word_posteriors_bigram_ref import bigram_graph, confidence, q_from_matrices, sweep

pytestmark = pytest.mark.gpu

M_, D_ = 2, 3
RTOL, ATOL, RTOL_LOGP = 1e-8, 1e-10, 1e-10
#         W   n  skip
CASES = [(64, 2, False),
         (2, 3, False),
         (17, 3, True),
         (33, 4, False),
         (16, 4, True),
         (17, 5, False),
         (3, 5, True),
         (16, 6, False),
         (2, 6, True),
         (33, 7, False),
         (3, 7, True),
         (64, 8, False),
         (17, 8, True)]
CASE_IDS = ["W%d-n%d-%s" % (c[0], c[1], "skip" if c[2] else "plain") for c in CASES]
RAGGED = tuple(60 - 7 * u for u in range(9))                              # 60, 53, ... 4


def word_trans(rng, n, skip, self_loops=True):
    t = np.full((n, n), np.inf)
    for i in range(n):
        if self_loops:
            t[i, i] = rng.uniform(0.1, 2.0)
        if i < n - 1:
            t[i + 1, i] = rng.uniform(0.1, 2.0)
        if skip and i < n - 2:
            t[i + 2, i] = rng.uniform(0.1, 2.0)
    return t


def make_case(W, n, skip, T=RAGGED, seed=0, scale=1.0, B=None, init=None, no_self_loops=()):
    rng = np.random.default_rng(12000 + 100 * W + 10 * n + skip + seed)
    means = rng.normal(size=(W, n, M_, D_)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M_, D_))
    w = rng.dirichlet(np.ones(M_), size=(W, n))
    trans = [word_trans(rng, n, skip, self_loops=i not in no_self_loops) for i in range(W)]
    xs = [rng.normal(size=(t, D_)) * 2.0 * scale for t in T]
    B = rng.uniform(0.0, 3.0, size=(W, W)) if B is None else np.asarray(B, dtype=np.float64)
    init = rng.uniform(0.0, 3.0, size=W) if init is None else np.asarray(init, dtype=np.float64)
    return dict(W=W, n=n, skip=skip, means=means, vars=vars_, w=w, trans=trans, xs=xs, T=np.array(T), B=B, init=init)


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


def hmms_of(R, case):
    return [make_hmm(R, case["means"][i], case["vars"][i], case["w"][i], case["trans"][i]) for i in range(case["W"])]


def decoder_of(R, ctx, case, dtype=np.float64, **kw):
    from sr.recognition.batch import ContinuousDecoder
    kw.setdefault("grammar", "bigram")
    if kw["grammar"] == "bigram":
        kw.setdefault("bigram", case["B"])
        if not hasattr(kw["bigram"], "costs"):
            kw.setdefault("initial", case["init"])
    dec = ContinuousDecoder(hmms_of(R, case), dtype=dtype, ctx=ctx, **kw)
    if kw["grammar"] == "bigram" and case["W"] >= 2:
        trans, nes, rw, ends, entry, row_of = bigram_graph(case["trans"], case["n"], case["B"], case["init"])
        want = np.full(len(nes), -1)
        want[row_of] = np.arange(case["W"] * case["n"]).reshape(case["W"], case["n"])
        np.testing.assert_array_equal(dec.row_state, want)
        assert list(dec.lat.end_rows[0]) == list(ends)
    return dec


def restate(case, nll, T=None, B=None, init=None, dtype=np.float64):
    """[(post [T, W], logp)] of every utterance from the device's own likelihood matrix."""
    T = case["T"] if T is None else np.asarray(T)
    off = np.concatenate([[0], np.cumsum(T)])
    W, n = case["W"], case["n"]
    nll = np.asarray(nll, dtype=np.float64)
    B = case["B"] if B is None else B
    init = case["init"] if init is None else init
    out = []
    for u in range(len(T)):
        post, logp, _ = sweep(case["trans"], B, init, nll[off[u]:off[u + 1]].reshape(-1, W, n), dtype=dtype)
        out.append((post, logp))
    return out


def close_logp(got, want, rtol=RTOL_LOGP):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    inf = np.isinf(want)
    np.testing.assert_array_equal(got[inf], want[inf])
    np.testing.assert_allclose(got[~inf], want[~inf], rtol=rtol, atol=0)


def check_against(case, ref, post, logp, conf=None, words=None, begins=None, sums_to_one=True, T=None, atol=ATOL, rtol_logp=RTOL_LOGP):
    T = case["T"] if T is None else np.asarray(T)
    off = np.concatenate([[0], np.cumsum(T)])
    W = case["W"]
    assert post.shape == (off[-1], W) and np.isfinite(post).all()
    worst = 0.0
    for u, (p, lp) in enumerate(ref):
        got = post[off[u]:off[u + 1]]
        worst = max(worst, float(np.max(np.abs(got - p) / (atol + RTOL * np.abs(p)), initial=0.0)))
        if conf is not None:
            want = confidence(p, words[u], begins[u], T[u])
            assert conf[u].shape == want.shape and conf[u].dtype == np.float64
            worst = max(worst, float(np.max(np.abs(conf[u] - want) / (atol + RTOL * np.abs(want)), initial=0.0)))
    fin = np.isfinite(np.asarray([float(lp) for _, lp in ref]))
    print("worst error / tolerance: %.3g; worst log P error / tolerance: %.3g" % (worst, float(np.max(
        np.abs(np.asarray(logp)[fin] - np.asarray([float(lp) for _, lp in ref])[fin]) /
        (rtol_logp * np.abs(np.asarray([float(lp) for _, lp in ref])[fin])), initial=0.0))))
    close_logp(logp, [float(lp) for _, lp in ref], rtol_logp)
    for u, (p, lp) in enumerate(ref):
        got = post[off[u]:off[u + 1]]
        if np.isinf(lp):
            assert not got.any()
        elif sums_to_one:
            assert np.max(np.abs(got.sum(axis=1) - 1.0)) <= W * 1e-10 + 2e-8
        np.testing.assert_allclose(got, np.asarray(p, dtype=np.float64), rtol=RTOL, atol=atol)
        if conf is not None:
            np.testing.assert_allclose(conf[u], confidence(p, words[u], begins[u], T[u]), rtol=RTOL, atol=atol)
            if np.isinf(lp):
                assert not conf[u].any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", CASES, ids=CASE_IDS)
def test_every_instantiation_against_the_restatement(R, hip, ctx, shape, dtype):
    case = make_case(*shape)
    dec = decoder_of(R, ctx, case, dtype)
    assert ("bigram_wide" if shape[0] > 16 else "bigram") in dec.lat.forms()
    b = hip.Batch(ctx, case["xs"], dtype=dtype)
    nll = b.loglik(dec.gmm, fetch=True)
    ref = restate(case, nll)
    words, r = dec.decode_batch(b, want_confidence=True, lm=True)
    post, logp = dec.word_posteriors(b, lm=True)
    assert ctx.last_chunks == 1
    np.testing.assert_array_equal(logp, r["logp"])
    assert sum(len(w) for w in words) >= len(words) - 2                   # the confidences are not checked on nothing
    assert sum(np.isfinite(lp) for _, lp in ref) >= 7
    check_against(case, ref, post, logp, r["confidence"], words, r["begins"])
    for c in r["confidence"]:
        assert np.all(c >= 0.0) and np.all(c <= 1.0 + 1e-9)
    b.close()


# ------------------------------------------------------------------------------------------------ sparse language models
def sparse_costs(W, kind, rng):
    """(B, init, words without self loops, the words the case is about)."""
    B = rng.uniform(0.0, 3.0, size=(W, W))
    init = rng.uniform(0.0, 3.0, size=W)
    B[rng.random((W, W)) < 0.35] = np.inf
    if kind == "forbidden":
        init[0] = np.inf
        B[:, 1] = np.inf                                                  # word 1 can only start an utterance
        B[2, :] = np.inf                                                  # word 2 can only end one
        return B, init, (), dict(only_starts=1, only_ends=2)
    if kind == "far-below-the-maximum":
        # j runs through its states without a self loop, from frame 0 and only there, and leads nowhere: in column n - 1
        # its last state holds the wave's maximum, above -400.  p is the only other start, at a cost of 1200, and leads
        # to c alone; c, in another quarter of the wave, is entered from p alone.  Every path of an utterance longer than
        # n frames begins with p, so the 1200 cancels in every posterior -- and c can be entered in column n - 1 only
        # if exp(a_p - max) is not what the sum is made of: a_p lies 800 below the maximum there, beyond exp's range.
        j, p, c = 4, 3, W - 1
        init[:] = np.inf
        init[j], init[p] = 0.0, 1200.0
        B[j, :] = np.inf
        B[:, j] = np.inf
        B[:, c] = np.inf
        B[p, :] = np.inf
        B[p, c] = 0.5
        B[c, 0] = B[c, 5] = 1.0                                           # (c leads on)
        return B, init, (j,), dict(j=j, p=p, c=c)
    assert kind == "one-start-only"
    B[:] = np.inf
    init[:] = np.inf
    init[6] = 0.7
    return B, init, (6,), dict(k=6)


@pytest.mark.parametrize("kind", ["forbidden", "far-below-the-maximum", "one-start-only"])
@pytest.mark.parametrize("W", [17, 64])
def test_sparse_language_models(R, hip, ctx, W, kind):
    n = 3
    rng = np.random.default_rng(77 + W)
    B, init, chains, who = sparse_costs(W, kind, rng)
    T = (60, 53, 46, n, 32, 25, 18, 11, 4) if kind == "one-start-only" else RAGGED
    case = make_case(W, n, kind == "forbidden", T=T, seed=9, B=B, init=init, no_self_loops=chains)
    dec = decoder_of(R, ctx, case)
    assert "bigram_wide" in dec.lat.forms()
    b = hip.Batch(ctx, case["xs"])
    nll = b.loglik(dec.gmm, fetch=True)
    ref = restate(case, nll)
    if kind == "one-start-only":
        # (most utterances have no path at all, which the Viterbi decode reports as an error of its own: a span table of
        #  our own, the one word from frame 0)
        words, begins = [[who["k"]]] * len(T), [[0]] * len(T)
        r = dec.lat.word_posteriors_bigram(b, labels=words, begins=begins)
        post, logp = r["post"], r["logp"]
    else:
        words, r = dec.decode_batch(b, want_confidence=True, lm=True)
        begins = r["begins"]
        post, logp = dec.word_posteriors(b, lm=True)
    check_against(case, ref, post, logp, r["confidence"], words, begins)
    if kind == "forbidden":
        assert np.isinf(B[:, who["only_starts"]]).all() and np.isinf(B[who["only_ends"]]).all()
        for p, lp in ref:
            assert np.isfinite(lp) and p[0, 0] == 0.0                     # word 0 never starts
    elif kind == "far-below-the-maximum":
        j, p_, c = who["j"], who["p"], who["c"]
        assert j // 16 == p_ // 16 and c // 16 != p_ // 16
        off = np.concatenate([[0], np.cumsum(case["T"])])
        weights = []
        for u, (p, lp) in enumerate(ref):
            assert np.isfinite(lp) and lp < -1200.0
            e = np.asarray(nll, dtype=np.float64)[off[u]:off[u] + n].reshape(n, W, n)
            a_j = -sum(e[t, j, t] + (case["trans"][j][t, t - 1] if t else 0.0) for t in range(n))
            assert a_j > -400.0                                           # the wave's maximum in column n - 1: 800 above a_p
            weights.append(float(p[n - 1, c]))                            # c entered in that very column
        print("q_{n-1}(c) per utterance:", " ".join("%.3g" % x for x in weights))
        assert max(weights) > 1e-3 and sum(x > 1e-7 for x in weights) >= 5
    else:
        fin = [np.isfinite(lp) for _, lp in ref]
        assert fin == [t == n for t in T]
        for u, (p, lp) in enumerate(ref):
            if np.isinf(lp):
                assert logp[u] == -np.inf and not r["confidence"][u].any()
            else:
                np.testing.assert_allclose(post[sum(T[:u]):sum(T[:u + 1]), who["k"]], 1.0, rtol=0, atol=1e-9)
    b.close()


# ------------------------------------------------------------------------------------------------ other kernels
@pytest.mark.parametrize("shape,p", [((3, 3, False), 0.7), ((17, 4, True), 0.0), ((64, 2, False), 2.5)], ids=["3x3", "17x4-skip", "64x2"])
def test_constant_costs_against_the_loop_form_kernel(R, hip, ctx, shape, p):
    W = shape[0]
    case = make_case(*shape, seed=1, B=np.full((W, W), p), init=np.zeros(W))
    bg = decoder_of(R, ctx, case)
    loop = decoder_of(R, ctx, case, grammar="loop", word_penalty=p)
    assert "loop" in loop.lat.forms() and not loop.lat.forms() & {"bigram", "bigram_wide"}
    b = hip.Batch(ctx, case["xs"])
    words, r = loop.decode_batch(b, want_confidence=True)
    want = loop.lat.word_posteriors(b, labels=r["labels"], begins=r["begins"])
    b.loglik(bg.gmm, fetch=False)
    got = bg.lat.word_posteriors_bigram(b, labels=r["labels"], begins=r["begins"])
    close_logp(got["logp"], want["logp"])
    assert np.isfinite(want["logp"]).sum() >= 7
    np.testing.assert_allclose(got["post"], want["post"], rtol=RTOL, atol=ATOL)
    for g, w_ in zip(got["confidence"], want["confidence"]):
        np.testing.assert_allclose(g, w_, rtol=RTOL, atol=ATOL)
    b.close()


@pytest.mark.parametrize("shape", [(3, 3, False), (16, 5, True), (17, 2, False)], ids=["3x3", "16x5-skip", "17x2"])
def test_against_the_generic_kernel(R, hip, ctx, shape):
    case = make_case(*shape, seed=2)
    case["B"][np.random.default_rng(3).random(case["B"].shape) < 0.2] = np.inf
    dec = decoder_of(R, ctx, case)
    trans, nes, rw, ends, entry, row_of = bigram_graph(case["trans"], case["n"], case["B"], case["init"])
    b = hip.Batch(ctx, case["xs"])
    b.loglik(dec.gmm, fetch=False)
    fb = dec.lat.forward_backward(b, want_matrices=True)
    post, logp = dec.word_posteriors(b, lm=True)
    close_logp(logp, fb["logp"])
    off = np.concatenate([[0], np.cumsum(case["T"])])
    for u in range(len(case["T"])):
        want = q_from_matrices(fb["alpha"][u], fb["beta"][u], fb["logp"][u], trans, rw, entry, row_of)
        np.testing.assert_allclose(post[off[u]:off[u + 1]], want, rtol=RTOL, atol=ATOL)
    b.close()


@pytest.mark.parametrize("shape", [(3, 2, False), (17, 4, True), (5, 8, False)], ids=["3x2", "17x4-skip", "5x8"])
def test_short_utterances_beside_long_ones(R, hip, ctx, shape):
    n = shape[1]
    T = (40, 1, 2, n - 1, 33, 1, n, 2)
    case = make_case(*shape, T=T, seed=3)
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, case["xs"])
    nll = b.loglik(dec.gmm, fetch=True)
    ref = restate(case, nll)
    assert np.isinf(ref[1][1]) and np.isinf(ref[5][1]) and np.isfinite(ref[0][1]) and np.isfinite(ref[4][1])
    # a span table of our own: one word from frame 0 in every utterance, also where there is no path
    labels = [[u % case["W"]] for u in range(len(T))]
    begins = [[0]] * len(T)
    r = dec.lat.word_posteriors_bigram(b, labels=labels, begins=begins)
    assert np.isfinite(r["post"]).all()
    check_against(case, ref, r["post"], r["logp"], r["confidence"], labels, begins)
    for u, (p, lp) in enumerate(ref):
        if np.isinf(lp):
            assert r["logp"][u] == -np.inf and r["confidence"][u].tolist() == [0.0]
    # ... and the decode's own words
    words, rd = dec.decode_batch(b, want_confidence=True, lm=True)
    check_against(case, ref, r["post"], rd["logp"], rd["confidence"], words, rd["begins"])
    b.close()


def test_costs_of_order_a_million(R, hip, ctx):
    """set_compat(underflow=False) keeps the likelihoods in the log domain, where costs of order 1e6 are finite.  Both sides
    are fp64 recursions that round log-alphas of order 1e7 (one unit in the last place: 2e-9), so the bound is taken from
    the restatement's own rounding: the largest deviation of the fp64 restatement from the same recursion in np.longdouble
    on these inputs, times 8 (the other order of the sums over the words, one or two units in the last place of the
    device's exp / log), and never less than the project's bound.  Both figures are printed."""
    case = make_case(4, 4, True, T=(60, 31, 17), seed=4, scale=1e3)
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, case["xs"])
    ctx.set_compat(underflow=False)
    try:
        nll = b.loglik(dec.gmm, fetch=True)
        assert np.isfinite(nll).all() and np.median(nll) > 1e5
        words, r = dec.decode_batch(b, want_confidence=True, lm=True)
        post, logp = dec.word_posteriors(b, lm=True)
    finally:
        ctx.set_compat(underflow=True)
    assert np.isfinite(logp).all() and not np.isnan(post).any() and all(len(w) >= 1 for w in words)
    ref = restate(case, nll)
    ext = restate(case, nll, dtype=np.longdouble)
    dev_q = max(float(np.max(np.abs(p - x))) for (p, _), (x, _) in zip(ref, ext))
    dev_logp = max(float(abs((lp - xl) / xl)) for (_, lp), (_, xl) in zip(ref, ext))
    atol, rtol_logp = max(ATOL, 8.0 * dev_q), max(RTOL_LOGP, 8.0 * dev_logp)
    print("fp64 restatement against np.longdouble: max |dq| = %.3g, max rel |dlogP| = %.3g -> atol %.3g, log P rtol %.3g"
          % (dev_q, dev_logp, atol, rtol_logp))
    print("restatement, max |sum_w q - 1|: %.3g; device: %.3g" % (max(np.max(np.abs(p.sum(axis=1) - 1.0)) for p, _ in ref),
                                                                   np.max(np.abs(post.sum(axis=1) - 1.0))))
    check_against(case, ref, post, logp, r["confidence"], words, r["begins"], sums_to_one=False, atol=atol, rtol_logp=rtol_logp)
    b.close()


# ------------------------------------------------------------------------------------------------ blocks, position, chunks
@pytest.mark.parametrize("U", [1, 4, 5, 9])
@pytest.mark.parametrize("shape", [(3, 3, False), (17, 3, True)], ids=["3x3", "17x3-skip"])
def test_full_and_partly_filled_blocks(R, hip, ctx, shape, U):
    """A block holds four utterances: 1 and 5 leave waves without one, 4 fills a block, 9 fills two and starts a third."""
    case = make_case(*shape, seed=5)
    xs = [x for x in case["xs"][:U]]
    T = [len(x) for x in xs]
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, xs)
    nll = b.loglik(dec.gmm, fetch=True)
    ref = restate(case, nll, T=T)
    words, r = dec.decode_batch(b, want_confidence=True, lm=True)
    post, logp = dec.word_posteriors(b, lm=True)
    check_against(case, ref, post, logp, r["confidence"], words, r["begins"], T=T)
    b.close()


def test_batch_position_does_not_matter(R, hip, ctx):
    case = make_case(17, 4, False, seed=6)
    dec = decoder_of(R, ctx, case)
    xs = case["xs"]
    x = xs[2]

    def run(batch_xs, u):
        b = hip.Batch(ctx, batch_xs)
        words, r = dec.decode_batch(b, want_confidence=True, lm=True)
        post, logp = dec.word_posteriors(b, lm=True)
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


def test_chunked_launches_give_the_same_bits(R, hip, ctx, monkeypatch):
    case = make_case(17, 3, True, seed=7)
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, case["xs"])
    monkeypatch.delenv("GMMHMM_SCRATCH_BUDGET", raising=False)
    words, r = dec.decode_batch(b, want_confidence=True, lm=True)
    one = dec.lat.word_posteriors_bigram(b, labels=r["labels"], begins=r["begins"])
    assert ctx.last_chunks == 1
    # alpha scratch: 8 T n W bytes per utterance -- 24 KB for the longest; the batch takes 118 KB
    monkeypatch.setenv("GMMHMM_SCRATCH_BUDGET", "40K")
    cut = dec.lat.word_posteriors_bigram(b, labels=r["labels"], begins=r["begins"])
    assert ctx.last_chunks >= 3, ctx.last_chunks
    monkeypatch.delenv("GMMHMM_SCRATCH_BUDGET")
    np.testing.assert_array_equal(cut["post"], one["post"])
    np.testing.assert_array_equal(cut["logp"], one["logp"])
    for a, c, d in zip(one["confidence"], cut["confidence"], r["confidence"]):
        np.testing.assert_array_equal(c, a)
        np.testing.assert_array_equal(d, a)
    b.close()


# ------------------------------------------------------------------------------------------------ the decoder keyword
@pytest.mark.parametrize("W", [3, 17])
def test_decode_with_confidence_under_a_language_model(R, hip, ctx, W):
    from sr.langmodel import BigramModel
    case = make_case(W, 4, False, seed=8)
    rng = np.random.default_rng(80 + W)
    lm = BigramModel(W, smoothing=0.5).fit([list(rng.integers(0, W, size=6)) for _ in range(30)])
    init, B = lm.costs(2.0)
    case["B"], case["init"] = np.asarray(B, dtype=np.float64), np.asarray(init, dtype=np.float64)
    dec = decoder_of(R, ctx, case, bigram=lm, lm_scale=2.0)
    b = hip.Batch(ctx, case["xs"])
    with pytest.raises(hip.Unsupported, match="bigram grammar"):
        dec.decode_batch(b, want_confidence=True)
    plain_words, plain = dec.decode_batch(b, lm=True)
    timed_words, timed = dec.decode_batch(b, want_times=True)
    words, r = dec.decode_batch(b, want_confidence=True, lm=True)
    assert words == timed_words == plain_words and "confidence" not in plain and "confidence" not in timed
    for key in ("end_cost_flat", "best_end", "n_labels", "label_off"):
        np.testing.assert_array_equal(r[key], timed[key])
    nll = b.loglik(dec.gmm, fetch=True)
    ref = restate(case, nll)
    post, logp = dec.word_posteriors(b, lm=True)
    np.testing.assert_array_equal(r["logp"], logp)
    off = np.concatenate([[0], np.cumsum(case["T"])])
    for u in range(len(case["T"])):
        np.testing.assert_array_equal(r["labels"][u], timed["labels"][u])
        np.testing.assert_array_equal(r["begins"][u], timed["begins"][u])
        assert np.all(r["confidence"][u] >= 0.0) and np.all(r["confidence"][u] <= 1.0 + 1e-9)
        want = confidence(post[off[u]:off[u + 1]], words[u], r["begins"][u], case["T"][u])
        np.testing.assert_allclose(r["confidence"][u], want, rtol=1e-13, atol=1e-15)   # the same q, summed in the other order
    check_against(case, ref, post, logp, r["confidence"], words, r["begins"])
    w2, b2, c2 = dec.decode(case["xs"], want_confidence=True, lm=True)
    assert w2 == words
    for u in range(len(case["T"])):
        np.testing.assert_array_equal(b2[u], r["begins"][u])
        np.testing.assert_array_equal(c2[u], r["confidence"][u])
    b.close()


def test_a_one_word_bigram_decoder_goes_by_its_form(R, hip, ctx):
    case = make_case(1, 3, False, seed=9, B=np.zeros((1, 1)), init=np.zeros(1))
    dec = decoder_of(R, ctx, case)
    assert "loop" in dec.lat.forms()                                      # one entry row: the rows of the loop form
    loop = decoder_of(R, ctx, case, grammar="loop", word_penalty=0.0)
    b = hip.Batch(ctx, case["xs"])
    words, r = dec.decode_batch(b, want_confidence=True, lm=True)
    lwords, lr = loop.decode_batch(b, want_confidence=True)
    assert words == lwords
    np.testing.assert_array_equal(r["logp"], lr["logp"])
    for a, c in zip(r["confidence"], lr["confidence"]):
        np.testing.assert_array_equal(a, c)
    b.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_through_the_library(R, hip, ctx):
    rng = np.random.default_rng(8)
    small = make_case(3, 3, False, seed=10)
    wide = make_case(17, 2, False, seed=10)
    xs = small["xs"][:2]

    def refused(dec, hint, method="word_posteriors_bigram"):
        b = hip.Batch(ctx, xs)
        b.loglik(dec.gmm, fetch=False)
        with pytest.raises(hip.Unsupported, match=hint) as e:
            getattr(dec.lat, method)(b)
        b.close()
        return str(e.value)
    twelve = make_case(2, 12, False, seed=10)
    sentences = [refused(decoder_of(R, ctx, small, grammar="loop"), "loop form.*gh_word_posteriors takes it"),
                 refused(decoder_of(R, ctx, small, grammar="layers", n_layers=2), "K-layer lattice"),
                 refused(decoder_of(R, ctx, twelve), "12 states")]
    beamed = decoder_of(R, ctx, small)
    beamed.lat.set_beam(3)
    sentences.append(refused(beamed, "rank beam"))
    assert len(set(sentences)) == 4 and all(s.startswith("gh_word_posteriors_bigram:") for s in sentences)
    # gh_word_posteriors on a bigram handle is refused as it always was
    assert "in bigram form" in refused(decoder_of(R, ctx, small), "in bigram form", "word_posteriors")
    assert "wide bigram form" in refused(decoder_of(R, ctx, wide), "wide bigram form", "word_posteriors")
    # argument errors: nothing is written
    dec = decoder_of(R, ctx, small)
    b = hip.Batch(ctx, xs)
    with pytest.raises(hip.BackendError, match="gh_word_posteriors_bigram: gh_loglik has not been run") as e:
        dec.lat.word_posteriors_bigram(b)
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
        rc = lib.gh_word_posteriors_bigram(ctx.h, dec.lat.h, b.h, p(logp, f64p), p(post, f64p), p(a["labels"], i32p),
                                           p(a["begins"], i32p), p(a["off"], i64p), p(a["nl"], i32p), p(conf, f64p))
        assert rc == -1, hint
        assert re.search("gh_word_posteriors_bigram: .*" + hint, lib.gh_last_error().decode()), lib.gh_last_error()
        assert np.all(logp == 7.0) and np.all(post == 7.0) and np.all(conf == 7.0)
    logp, post, conf = np.full(2, 7.0), np.full((b.N, 3), 7.0), np.full(4, 7.0)
    rc = lib.gh_word_posteriors_bigram(ctx.h, dec.lat.h, b.h, p(logp, f64p), p(post, f64p), p(good["labels"], i32p),
                                       p(good["begins"], i32p), p(good["off"], i64p), p(good["nl"], i32p), p(conf, f64p))
    assert rc == 0 and np.all(logp != 7.0) and np.all(post != 7.0) and np.all(conf != 7.0)
    b.close()
