# -*- coding: utf-8 -*-
"""Word posteriors and per-word confidence on the K-layer lattice, on the device: gh_word_posteriors_layers
(csrc/gh_fb_layers.hip), `Lattices.word_posteriors_layers`, `ContinuousDecoder.word_posteriors(..., layers=True)` and
`decode_batch(..., want_confidence=True, layers=True)`.

Every case feeds tiny models (D = 3, 2 mixtures) and at most 40 frames per utterance.  Both sides of a comparison work on
the device's own likelihood matrix (`b.loglik(gmm, fetch=True)`; an fp32 batch: the fp32 values widened), so likelihood
error never enters.  Tolerances are those of tests/test_gpu_word_posteriors.py: posteriors and confidences rtol 1e-8 with
atol 1e-10, log P rtol 1e-10, -inf and zero rows exact; "sums to one" follows from them: |sum_w post[t] - 1| <= W 1e-10 +
2e-8.  The restatement is `sweep` of tests/word_posteriors_layers_ref.py (held to the formula on `O.forward_backward` and to
enumeration by the host tests); the generic kernel's matrices are a second, independent reference.

  1. every N = 2 .. 8 with and without skip arcs, both dtypes, K = 5, W = 3 (two register sets, partly filled rows);
  2. K in {1, 2, 4, 5, 8} x W in {1, 3, 16} at N = 3 (row-to-row hand-over, the set boundary 3 -> 4, full rows, one word,
     one layer);
  3. against q from the generic kernel's alpha, beta and log P;
  4. T = 1, 2, K (N-1) (no path) and K (N-1) + 1 beside long utterances;
  5. the mixture identity against gh_word_posteriors of a loop decoder, K = 1 .. 8 on the same matrix;
  6. frames scaled by 1e3 (costs of order 1e6);
  7. batches of 1 / 4 / 5, batch position and chunked launches: bitwise the same;
  8. `decode_batch(b, want_confidence=True, layers=True)` and `decode(...)`, one utterance at the reference's 11 x 5 x 7;
  9. refusals and bad span tables through the real library."""
import re

import numpy as np
import pytest

from word_posteriors_layers_ref import confidence, layers_graph, q_from_matrices, sweep

pytestmark = pytest.mark.gpu

M_, D_ = 2, 3
RTOL, ATOL, RTOL_LOGP = 1e-8, 1e-10, 1e-10
RAGGED = (40, 38, 37, 30, 21, 9)


def word_trans(rng, n, skip):
    t = np.full((n, n), np.inf)
    for i in range(n):
        t[i, i] = rng.uniform(0.1, 2.0)
        if i < n - 1:
            t[i + 1, i] = rng.uniform(0.1, 2.0)
        if skip and i < n - 2:
            t[i + 2, i] = rng.uniform(0.1, 2.0)
    return t


def make_case(W, n, K, skip, T=RAGGED, seed=0, scale=1.0):
    rng = np.random.default_rng(31000 + 1000 * K + 100 * W + 10 * n + skip + seed)
    means = rng.normal(size=(W, n, M_, D_)) * 2.0
    vars_ = rng.uniform(0.5, 1.5, size=(W, n, M_, D_))
    w = rng.dirichlet(np.ones(M_), size=(W, n))
    trans = [word_trans(rng, n, skip) for _ in range(W)]
    xs = [rng.normal(size=(t, D_)) * 2.0 * scale for t in T]
    return dict(W=W, n=n, K=K, skip=skip, means=means, vars=vars_, w=w, trans=trans, xs=xs, T=np.array(T))


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
    kw.setdefault("grammar", "layers")
    if kw["grammar"] == "layers":
        kw.setdefault("n_layers", case["K"])
    dec = ContinuousDecoder(hmms, dtype=dtype, ctx=ctx, **kw)
    if kw["grammar"] == "layers":
        P = case["W"] * case["n"]
        np.testing.assert_array_equal(dec.row_state[1:1 + P], np.arange(P))     # row (w, s) of a layer scores state w n + s
    return dec


def restate(case, nll, K=None, dtype=np.float64, T=None):
    """[(post [T, W], logp)] of every utterance from the device's own likelihood matrix."""
    T = case["T"] if T is None else np.asarray(T)
    off = np.concatenate([[0], np.cumsum(T)])
    nll = np.asarray(nll, dtype=np.float64)
    return [sweep(case["trans"], nll[off[u]:off[u + 1], :case["W"] * case["n"]].reshape(-1, case["W"], case["n"]),
                  case["K"] if K is None else K, dtype)[:2] for u in range(len(T))]


def close_logp(got, want, rtol=RTOL_LOGP):
    got, want = np.asarray(got), np.asarray(want, dtype=np.float64)
    inf = np.isinf(want)
    np.testing.assert_array_equal(got[inf], want[inf])
    np.testing.assert_allclose(got[~inf], want[~inf], rtol=rtol, atol=0)


def check_against(case, ref, post, logp, conf=None, words=None, begins=None, sums_to_one=True, T=None, atol=ATOL, rtol_logp=RTOL_LOGP):
    T = case["T"] if T is None else np.asarray(T)
    off = np.concatenate([[0], np.cumsum(T)])
    W = case["W"]
    assert post.shape == (off[-1], W) and np.isfinite(post).all()
    close_logp(logp, [r[1] for r in ref], rtol_logp)
    worst = 0.0
    for u, (p, lp) in enumerate(ref):
        p = np.asarray(p, dtype=np.float64)
        got = post[off[u]:off[u + 1]]
        worst = max(worst, float(np.max(np.abs(got - p) / (atol + RTOL * np.abs(p)), initial=0.0)))
        if np.isinf(lp):
            assert not got.any()
        elif sums_to_one:
            assert np.max(np.abs(got.sum(axis=1) - 1.0)) <= W * 1e-10 + 2e-8
        if conf is not None:
            want = confidence(p, words[u], begins[u], T[u])
            assert conf[u].shape == want.shape and conf[u].dtype == np.float64
            worst = max(worst, float(np.max(np.abs(conf[u] - want) / (atol + RTOL * np.abs(want)), initial=0.0)))
            if np.isinf(lp):
                assert not conf[u].any()
    print("worst error / tolerance: %.3g" % worst)
    for u, (p, lp) in enumerate(ref):
        p = np.asarray(p, dtype=np.float64)
        np.testing.assert_allclose(post[off[u]:off[u + 1]], p, rtol=RTOL, atol=atol)
        if conf is not None:
            np.testing.assert_allclose(conf[u], confidence(p, words[u], begins[u], T[u]), rtol=RTOL, atol=atol)


def run_case(R, hip, ctx, case, dtype=np.float64, min_paths=2):
    dec = decoder_of(R, ctx, case, dtype)
    assert "layers" in dec.lat.forms()
    b = hip.Batch(ctx, case["xs"], dtype=dtype)
    nll = b.loglik(dec.gmm, fetch=True)
    ref = restate(case, nll)
    words, r = dec.decode_batch(b, want_confidence=True, layers=True)
    post, logp = dec.word_posteriors(b, layers=True)
    assert ctx.last_chunks == 1
    np.testing.assert_array_equal(logp, r["logp"])
    assert sum(np.isfinite(lp) for _, lp in ref) >= min_paths
    assert sum(len(w) == case["K"] for w in words) >= min_paths            # the confidences are not checked on nothing
    check_against(case, ref, post, logp, r["confidence"], words, r["begins"])
    for c in r["confidence"]:
        assert np.all(c >= 0.0) and np.all(c <= 1.0 + 1e-9)
    b.close()


N_CASES = [(2, False)] + [(n, s) for n in range(3, 9) for s in (False, True)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,skip", N_CASES, ids=["n%d-%s" % (n, "skip" if s else "plain") for n, s in N_CASES])
def test_every_instantiation_against_the_restatement(R, hip, ctx, n, skip, dtype):
    run_case(R, hip, ctx, make_case(3, n, 5, skip), dtype)


@pytest.mark.parametrize("W", [1, 3, 16])
@pytest.mark.parametrize("K", [1, 2, 4, 5, 8])
def test_layer_and_word_counts(R, hip, ctx, K, W):
    run_case(R, hip, ctx, make_case(W, 3, K, (K + W) % 2 == 1, seed=1))


@pytest.mark.parametrize("shape", [(3, 3, 5, False), (16, 2, 8, False), (2, 5, 4, True), (1, 4, 1, True)],
                         ids=["3x3x5", "16x2x8", "2x5x4-skip", "1x4x1-skip"])
def test_against_the_generic_kernel(R, hip, ctx, shape):
    case = make_case(*shape, seed=2)
    W, n, K = shape[:3]
    dec = decoder_of(R, ctx, case)
    rw, rs, nes, dense, ends = layers_graph(case["trans"], n, K)
    np.testing.assert_array_equal(dec.row_state, np.where(nes, -1, rw * n + rs))
    assert list(dec.lat.end_rows[0]) == list(ends)
    b = hip.Batch(ctx, case["xs"])
    b.loglik(dec.gmm, fetch=False)
    fb = dec.lat.forward_backward(b, want_matrices=True)
    post, logp = dec.word_posteriors(b, layers=True)
    close_logp(logp, fb["logp"])
    assert np.isfinite(logp).sum() >= 2
    off = np.concatenate([[0], np.cumsum(case["T"])])
    for u in range(len(case["T"])):
        want, _ = q_from_matrices(fb["alpha"][u], fb["beta"][u], fb["logp"][u], dense, W, n, K)
        np.testing.assert_allclose(post[off[u]:off[u + 1]], want, rtol=RTOL, atol=ATOL)
    b.close()


@pytest.mark.parametrize("shape", [(3, 2, 5, False), (16, 4, 3, False), (2, 8, 4, False), (3, 3, 8, False)],
                         ids=["3x2x5", "16x4x3", "2x8x4", "3x3x8"])
def test_short_utterances_beside_long_ones(R, hip, ctx, shape):
    W, n, K = shape[:3]
    need = K * (n - 1) + 1                                                 # the shortest utterance with a path (no skip arcs)
    T = (40, 1, 2, need - 1, need, 33, 1, need + 1)
    case = make_case(*shape, T=T, seed=3)
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, case["xs"])
    nll = b.loglik(dec.gmm, fetch=True)
    ref = restate(case, nll)
    for u, t in enumerate(T):
        assert np.isfinite(ref[u][1]) == (t >= need), (u, t)
    # a span table of our own: one word from frame 0 in every utterance, also where there is no path
    labels = [[u % W] for u in range(len(T))]
    begins = [[0]] * len(T)
    r = dec.lat.word_posteriors_layers(b, labels=labels, begins=begins)
    assert np.isfinite(r["post"]).all()
    check_against(case, ref, r["post"], r["logp"], r["confidence"], labels, begins)
    for u, (p, lp) in enumerate(ref):
        if np.isinf(lp):
            assert r["logp"][u] == -np.inf and r["confidence"][u].tolist() == [0.0]
    # at the exact minimum length the posterior of a LAYER is 0 or 1; summed over the layers every row is 1
    o = int(np.sum(T[:4]))
    np.testing.assert_allclose(r["post"][o:o + need].sum(axis=1), 1.0, rtol=0, atol=W * 1e-10 + 2e-8)
    # ... and the decode's own words
    words, rd = dec.decode_batch(b, want_confidence=True, layers=True)
    check_against(case, ref, r["post"], rd["logp"], rd["confidence"], words, rd["begins"])
    b.close()


@pytest.mark.parametrize("n,skip", [(2, False), (3, True)], ids=["n2", "n3-skip"])
def test_mixture_identity_against_the_loop_kernel(R, hip, ctx, n, skip):
    """word_penalty = 0: q_loop_t(w) = sum_K exp(logP_K - logP_loop) q^K_t(w) and logP_loop = LSE_K logP_K.  A word takes at
    least one column step, so with T - 1 = 7 <= 8 no lattice of 9 or more layers has a path: K = 1 .. 8 is the whole sum.
    Both kernels and all eight handles read the same resident matrix."""
    W, T = 3, (8, 8, 7, 5)
    case = make_case(W, n, 1, skip, T=T, seed=4)
    loop = decoder_of(R, ctx, case, grammar="loop", word_penalty=0.0)
    b = hip.Batch(ctx, case["xs"])
    b.loglik(loop.gmm, fetch=False)
    lq, llogp = loop.word_posteriors(b)
    assert np.isfinite(llogp).all()
    qs, lps = [], []
    for K in range(1, 9):
        dec = decoder_of(R, ctx, case, n_layers=K)
        r = dec.lat.word_posteriors_layers(b)
        qs.append(r["post"])
        lps.append(r["logp"])
    lps = np.array(lps)                                                    # [K, U]
    assert np.isfinite(lps).sum(axis=0).min() >= 2
    m = lps.max(axis=0)
    tot = m + np.log(np.exp(lps - m).sum(axis=0))
    np.testing.assert_allclose(tot, llogp, rtol=RTOL_LOGP, atol=0)
    wgt = np.repeat(np.exp(lps - tot), np.array(T), axis=1)                # [K, N]
    mix = sum(wgt[k][:, None] * qs[k] for k in range(8))
    print("max |mixture - loop|: %.3g" % np.abs(mix - lq).max())
    np.testing.assert_allclose(mix, lq, rtol=RTOL, atol=ATOL)
    b.close()


def test_costs_of_order_a_million(R, hip, ctx):
    """set_compat(underflow=False) keeps the likelihoods in the log domain, where costs of order 1e6 are finite.  Both sides
    are fp64 recursions that round log-alphas of order 1e7 (one unit in the last place: 2e-9), so the bound is taken from
    the restatement's own rounding, as tests/test_gpu_word_posteriors_bigram.py does: the largest deviation of the fp64
    restatement from the same recursion in np.longdouble on these inputs, times 8 (the other order of the sums over the
    words, one or two units in the last place of the device's exp / log), and never less than the project's bound.  Both
    figures are printed."""
    case = make_case(4, 4, 5, True, T=(40, 31, 17), seed=5, scale=1e3)
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, case["xs"])
    ctx.set_compat(underflow=False)
    try:
        nll = b.loglik(dec.gmm, fetch=True)
        assert np.isfinite(nll).all() and np.median(nll) > 1e5
        words, r = dec.decode_batch(b, want_confidence=True, layers=True)
        post, logp = dec.word_posteriors(b, layers=True)
    finally:
        ctx.set_compat(underflow=True)
    assert np.isfinite(logp).all() and not np.isnan(post).any() and all(len(w) == 5 for w in words)
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


def test_batch_size_position_and_chunking_give_the_same_bits(R, hip, ctx, monkeypatch):
    case = make_case(3, 3, 5, True, T=(40, 36, 31, 27, 22), seed=6)
    dec = decoder_of(R, ctx, case)
    xs = case["xs"]
    monkeypatch.delenv("GMMHMM_SCRATCH_BUDGET", raising=False)

    def run(batch_xs):
        b = hip.Batch(ctx, batch_xs)
        words, r = dec.decode_batch(b, want_confidence=True, layers=True)
        wp = dec.lat.word_posteriors_layers(b, labels=r["labels"], begins=r["begins"])
        chunks = ctx.last_chunks
        off = np.asarray(b.offsets)
        out = [(wp["post"][off[u]:off[u + 1]].copy(), wp["logp"][u], wp["confidence"][u].copy(), r["confidence"][u].copy(), words[u])
               for u in range(len(batch_xs))]
        b.close()
        return out, chunks
    five, chunks = run(xs)
    assert chunks == 1 and all(len(o[4]) == 5 for o in five)

    def same(a, c):
        np.testing.assert_array_equal(a[0], c[0])
        assert a[1] == c[1] and a[4] == c[4]
        np.testing.assert_array_equal(a[2], c[2])
        np.testing.assert_array_equal(a[3], c[3])
        np.testing.assert_array_equal(a[2], a[3])
    # batches of 1 and 4; three positions of utterance 2: alone, first, last
    alone, _ = run([xs[2]])
    same(alone[0], five[2])
    four, _ = run(xs[:4])
    for u in range(4):
        same(four[u], five[u])
    first, _ = run([xs[2]] + xs[:2] + xs[3:])
    last, _ = run(xs[:2] + xs[3:] + [xs[2]])
    same(first[0], five[2])
    same(last[4], five[2])
    # three launches: alpha scratch is 8 T K n W bytes per utterance -- 14 400 B for the longest, 56 160 B for the batch
    monkeypatch.setenv("GMMHMM_SCRATCH_BUDGET", "24K")
    cut, chunks = run(xs)
    monkeypatch.delenv("GMMHMM_SCRATCH_BUDGET")
    assert chunks >= 3, chunks
    for u in range(5):
        same(cut[u], five[u])


def test_decode_batch_with_confidence(R, hip, ctx):
    """... with one utterance at the reference's shape: 11 words x 5 states x 7 layers."""
    case = make_case(11, 5, 7, False, T=(40, 33, 29, 12), seed=7)
    dec = decoder_of(R, ctx, case)
    b = hip.Batch(ctx, case["xs"])
    nll = b.loglik(dec.gmm, fetch=True)
    plain_words, plain = dec.decode_batch(b)
    timed_words, timed = dec.decode_batch(b, want_times=True)
    words, r = dec.decode_batch(b, want_confidence=True, layers=True)
    assert words == timed_words == plain_words and [len(w) for w in words[:3]] == [7, 7, 7]
    assert r["logp"][3] == -np.inf and not r["confidence"][3].any()       # 12 frames: no path, whatever the decode labels
    for key in ("end_cost_flat", "best_end", "n_labels", "label_off"):
        np.testing.assert_array_equal(r[key], timed[key])
    for u in range(len(case["T"])):                                       # (the slots behind n_labels are not written)
        np.testing.assert_array_equal(r["labels"][u], timed["labels"][u])
        np.testing.assert_array_equal(r["begins"][u], timed["begins"][u])
    ref = restate(case, nll)
    post, logp = dec.word_posteriors(b, layers=True)
    np.testing.assert_array_equal(r["logp"], logp)
    check_against(case, ref, post, logp, r["confidence"], words, r["begins"])
    off = np.concatenate([[0], np.cumsum(case["T"])])
    for u in range(len(case["T"])):
        want = confidence(post[off[u]:off[u + 1]], words[u], r["begins"][u], case["T"][u])
        np.testing.assert_allclose(r["confidence"][u], want, rtol=1e-13, atol=1e-15)   # the same q, summed in the other order
    w2, b2, c2 = dec.decode(case["xs"], want_confidence=True, layers=True)
    assert w2 == words
    for u in range(len(case["T"])):
        np.testing.assert_array_equal(b2[u], r["begins"][u])
        np.testing.assert_array_equal(c2[u], r["confidence"][u])
    # without the keyword the decoder is refused as before, and the plain decode is what it was
    with pytest.raises(hip.Unsupported, match="K-layer lattice"):
        dec.decode_batch(b, want_confidence=True)
    again_words, again = dec.decode_batch(b)
    assert again_words == plain_words and sorted(again) == sorted(plain) and "confidence" not in again
    for key in ("end_cost_flat", "best_end", "n_labels"):
        np.testing.assert_array_equal(again[key], plain[key])
    b.close()


def test_refusals_through_the_library(R, hip, ctx):
    from sr.recognition.continuous_speech import packed_lattice
    rng = np.random.default_rng(8)
    small = make_case(3, 3, 2, False, seed=8)
    xs = small["xs"][:2]

    def refused(lat, gmm, hint):
        b = hip.Batch(ctx, xs)
        b.loglik(gmm, fetch=False)
        with pytest.raises(hip.Unsupported, match=hint) as e:
            lat.word_posteriors_layers(b)
        b.close()
        assert str(e.value).startswith("gh_word_posteriors_layers: ")
        return str(e.value)
    of = lambda case, **kw: decoder_of(R, ctx, case, **kw)
    sentences = []
    for dec, hint in ((of(small, grammar="loop"), "in loop form"),
                      (of(small, grammar="bigram", bigram=rng.uniform(0.0, 3.0, size=(3, 3))), "in bigram form"),
                      (of(make_case(17, 2, 1, False, seed=8), grammar="bigram", bigram=rng.uniform(0.0, 3.0, size=(17, 17))), "wide bigram form"),
                      (of(make_case(17, 2, 2, False, seed=8)), "17 words per layer"),
                      (of(make_case(2, 2, 9, False, seed=8)), "9 layers"),
                      (of(make_case(2, 12, 2, False, seed=8)), "12 states")):
        sentences.append(refused(dec.lat, dec.gmm, hint))
    ok = of(small)
    sentences.append(refused(hip.Lattices.from_transcripts(ctx, small["trans"], 3, [[0, 1], [2]]), ok.gmm, "transcript graphs"))
    graph, _ = packed_lattice(small["trans"], 3, [[0, 1], [1, 0]])          # layers that differ: no special form
    sentences.append(refused(hip.Lattices(ctx, [graph]), ok.gmm, "generic graph"))
    beamed = of(small)
    beamed.lat.set_beam(3)
    sentences.append(refused(beamed.lat, beamed.gmm, "rank beam"))
    assert len(set(sentences)) == 9                                         # the eight cases; the two bigram forms differ too
    # the other two entry points keep refusing a K-layer handle with their own sentences
    b = hip.Batch(ctx, xs)
    b.loglik(ok.gmm, fetch=False)
    for call in (ok.lat.word_posteriors, ok.lat.word_posteriors_bigram):
        with pytest.raises(hip.Unsupported, match="K-layer lattice"):
            call(b)
    b.close()
    # argument errors: nothing is written
    dec = ok
    b = hip.Batch(ctx, xs)
    with pytest.raises(hip.BackendError, match="gh_loglik has not been run") as e:
        dec.lat.word_posteriors_layers(b)
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
        rc = lib.gh_word_posteriors_layers(ctx.h, dec.lat.h, b.h, p(logp, f64p), p(post, f64p), p(a["labels"], i32p), p(a["begins"], i32p),
                                           p(a["off"], i64p), p(a["nl"], i32p), p(conf, f64p))
        assert rc == -1, hint
        assert re.search(hint, lib.gh_last_error().decode()), lib.gh_last_error()
        assert lib.gh_last_error().decode().startswith("gh_word_posteriors_layers: ")
        assert np.all(logp == 7.0) and np.all(post == 7.0) and np.all(conf == 7.0)
    logp, post, conf = np.full(2, 7.0), np.full((b.N, 3), 7.0), np.full(4, 7.0)
    rc = lib.gh_word_posteriors_layers(ctx.h, dec.lat.h, b.h, p(logp, f64p), p(post, f64p), p(good["labels"], i32p), p(good["begins"], i32p),
                                       p(good["off"], i64p), p(good["nl"], i32p), p(conf, f64p))
    assert rc == 0 and np.all(logp != 7.0) and np.all(post != 7.0) and np.all(conf != 7.0)
    # no utterances: GH_OK and no launch
    empty = hip.Batch(ctx, [])
    r = dec.lat.word_posteriors_layers(empty)
    assert ctx.last_chunks == 0 and r["logp"].shape == (0,) and r["post"].shape == (0, 3)
    empty.close()
    b.close()
