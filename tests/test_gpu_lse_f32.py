# -*- coding: utf-8 -*-
"""The opt-in fp32-exponential epilogue of the fp64 likelihood kernel (gh_ctx_set_compat bit 1, GMMHMM_LSE=f32exp;
`tile_lse_fe` / `nll_of_fe` in csrc/gh_loglik_mfma.hip) against two references:

* the same kernel with the flag off (the default context): the MFMA accumulators and the fp64 maximum are identical in
  both modes, so the difference is the fp32 epilogue's error alone;
* the fp64 oracle (`O.gmm_neg_loglik_batch`), with the default path's own tolerance of 1e-11 relative on top.

Every tolerance comes from one bound, `lse_f32_bound(M_pad)`, derived in DESIGN.md section 4.1 from the epilogue's
operations.  The module has a context of its own with the flag on; the default context is never switched."""
import math

import numpy as np
import pytest

from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24         # fp32 unit roundoff
EPS_EXP = 2.0 ** -23     # relative error of v_exp_f32 taken by the bound (1 ulp)
EPS_LOG = 2.0 ** -23     # error of v_log_f32 taken by the bound: 1 ulp of its result, here relative to 1
FP64_REL = 2.0 ** -50    # fp64 rounding of max + log(sum) and the scaling, both modes together, relative to |nll|


def _lambert_w(z):
    w = math.log1p(z)
    for _ in range(30):
        w -= (w * math.exp(w) - z) / (math.exp(w) * (w + 1.0))
    return w


def m_pad_of(M):
    """gh_gmm_create's padded mixture size: a power of two up to 16, else a multiple of 16."""
    if M <= 16:
        return 1 << max(0, (M - 1).bit_length())
    return (M + 15) // 16 * 16


def lse_f32_bound(m_pad):
    """B(M_pad), absolute |delta nll| of the fp32 epilogue against the exact log-sum-exp of the same accumulators
    (DESIGN.md section 4.1): fp32 sum levels d (2, 3, 4 for M_pad = 4, 8, >= 16) and T - 1 running-sum fmas, T exponentials
    per term (T = M_pad / 16 tiles per state from 32 on), the fp64 -> fp32 conversion of the exponents (at most
    W((M_pad - 1)/e) u over the sum), v_log_f32 on a sum in [1, M_pad] (1 ulp of log2 M_pad), and 1e-12 for
    second-order terms and the fp64 epilogue's own error."""
    depth = 2 if m_pad == 4 else 3 if m_pad == 8 else 4
    tiles = max(1, m_pad // 16)
    rel = (depth + tiles - 1 + _lambert_w((m_pad - 1) / math.e)) * U32 + tiles * EPS_EXP
    ulp_log = EPS_LOG * 2.0 ** math.floor(math.log2(math.log2(m_pad)))
    return rel + math.log(2.0) * ulp_log + 1e-12


@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


@pytest.fixture(scope="module")
def ctx_ref(hip):
    return hip.default_context()


@pytest.fixture(scope="module")
def ctx_fe(hip):
    c = hip.Context(0)
    c.set_compat(underflow=True, lse_f32=True)
    yield c
    c.close()


def loglik_on(hip, ctx, means, vars_, w, X, offsets, dtype=np.float64, **kw):
    gmm = hip.PackedGMM(ctx, means, vars_, w)
    b = hip.Batch(ctx, feats=X, offsets=offsets, dtype=dtype)
    try:
        return b.loglik(gmm, **kw).copy()
    finally:
        b.close()
        gmm.close()


def oracle_chunked(X, means, vars_, w, rows=4096):
    return np.concatenate([O.gmm_neg_loglik_batch(X[i:i + rows], means, vars_, w) for i in range(0, len(X), rows)])


def assert_within(got, ref, bound, rel=FP64_REL):
    """|got - ref| <= bound + rel |ref| on the finite entries; +inf / NaN at the same entries."""
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(ref))
    fin = np.isfinite(ref)
    assert np.isfinite(got[fin]).all()
    err = np.abs(got[fin] - ref[fin])
    tol = bound + rel * np.abs(ref[fin])
    if err.size:
        i = int(np.argmax(err - tol))
        assert err[i] <= tol[i], "max excess: |delta| = %.3g > %.3g (ref %.6g)" % (err[i], tol[i], ref[fin][i])
    return float(err.max()) if err.size else 0.0


def random_model(rng, S, M, D):
    return (rng.normal(size=(S, M, D)), rng.uniform(0.5, 1.5, size=(S, M, D)), rng.dirichlet(np.ones(M), size=S))


# ---------------------------------------------------------------------------- (a) every instantiation of the mode
LENS = [1, 33, 64, 97, 31, 2]   # 228 frames: one-frame and 33-frame utterances, a block boundary inside an utterance


@pytest.mark.parametrize("M", [3, 8, 11, 32, 48])
@pytest.mark.parametrize("D", [3, 7, 13, 22, 39, 46, 64])
def test_every_instantiation_within_bound(hip, ctx_ref, ctx_fe, monkeypatch, D, M):
    """KS = 2 ... 32 x M_pad = 4, 8, 16, 32, 48 x one / several blocks per wave; S = 67 (two LDS chunks, not a multiple
    of the states per tile) or 29 (whole rows)."""
    S = 67 if (D + M) % 2 else 29
    rng = np.random.default_rng(1000 * D + M)
    means, vars_, w = random_model(rng, S, M, D)
    X = rng.normal(size=(sum(LENS), D)) * 1.3
    off = np.concatenate([[0], np.cumsum(LENS)])
    B = lse_f32_bound(m_pad_of(M))
    ref = oracle_chunked(X, means, vars_, w)
    got = {}
    for bpw in ("1", "8"):
        monkeypatch.setenv("GMMHMM_LOGLIK_BPW", bpw)
        off_ = loglik_on(hip, ctx_ref, means, vars_, w, X, off)
        fe = loglik_on(hip, ctx_fe, means, vars_, w, X, off)
        assert_within(fe, off_, B)
        assert_within(fe, ref, B, rel=1e-11)
        got[bpw] = fe
    # the per-tile arithmetic does not depend on how many blocks a wave walks
    np.testing.assert_array_equal(got["1"], got["8"])


# ---------------------------------------------------------------------------- (b) worst case: near-ties
@pytest.mark.parametrize("M", [4, 8, 16, 32, 48, 64])
def test_near_ties_within_bound(hip, ctx_ref, ctx_fe, M):
    """Every component of a state nearly equally likely on every frame (one mean, variances within 3 %, weights over
    e^-2 ... 1): every term of the sum counts, the sum is deepest.  1.2e5 frames against the flag-off kernel."""
    rng = np.random.default_rng(500 + M)
    S, D, N = 6, 13, 120_000
    mu = rng.normal(size=(S, 1, D))
    means = np.repeat(mu, M, axis=1)
    vars_ = rng.uniform(0.97, 1.03, size=(S, M, D))
    w = np.exp(-rng.uniform(0.0, 2.0, size=(S, M)))
    w /= w.sum(axis=1, keepdims=True)
    X = mu[rng.integers(0, S, size=N), 0] + 0.7 * rng.normal(size=(N, D))
    off = [0, N // 3, N // 3 + 1, N]
    off_ = loglik_on(hip, ctx_ref, means, vars_, w, X, off)
    fe = loglik_on(hip, ctx_fe, means, vars_, w, X, off)
    B = lse_f32_bound(m_pad_of(M))
    err = assert_within(fe, off_, B)
    print("near-ties M=%d M_pad=%d: max |delta nll| = %.3g (bound %.3g)" % (M, m_pad_of(M), err, B))
    assert err > 0.0      # the mode is on: the fp32 epilogue is not bit-identical to the fp64 one


# ---------------------------------------------------------------------------- (c) dynamic range
@pytest.mark.parametrize("M", [4, 8, 16, 48])
def test_components_far_below_the_maximum(hip, ctx_ref, ctx_fe, M):
    """One dominant component, the others 10 ... 300 octaves below it (fp32's denormal and underflow range): terms
    that vanish in fp32 leave every cost finite and within the bound."""
    rng = np.random.default_rng(40 + M)
    S, D, N = 5, 7, 300
    mu = rng.normal(size=(S, 1, D))
    means = np.repeat(mu, M, axis=1)
    vars_ = np.repeat(rng.uniform(0.5, 1.5, size=(S, 1, D)), M, axis=1)
    octaves = np.concatenate([np.zeros((S, 1)), rng.uniform(10.0, 300.0, size=(S, M - 1))], axis=1)
    octaves[:, 1:4] = [10.0, 126.5, 149.5]                      # fp32 normal, denormal and below-denormal range
    w = 2.0 ** -octaves
    X = mu[rng.integers(0, S, size=N), 0] + rng.normal(size=(N, D))
    off = [0, 33, N]
    off_ = loglik_on(hip, ctx_ref, means, vars_, w, X, off)
    fe = loglik_on(hip, ctx_fe, means, vars_, w, X, off)
    assert np.isfinite(fe).all()
    assert_within(fe, off_, lse_f32_bound(m_pad_of(M)))


@pytest.mark.parametrize("M", [4, 8, 32])
def test_zero_weights(hip, ctx_ref, ctx_fe, M):
    """Weight-0 components; a state whose weights are all 0 costs +inf in both modes."""
    rng = np.random.default_rng(60 + M)
    S, D, N = 7, 13, 140
    means, vars_, w = random_model(rng, S, M, D)
    w[1, : M // 2] = 0.0
    w[2, 1:] = 0.0
    w[4] = 0.0
    w[1] /= w[1].sum()
    w[2] /= w[2].sum()
    X = rng.normal(size=(N, D))
    off_ = loglik_on(hip, ctx_ref, means, vars_, w, X, [0, N])
    fe = loglik_on(hip, ctx_fe, means, vars_, w, X, [0, N])
    assert np.isposinf(fe[:, 4]).all() and np.isposinf(off_[:, 4]).all()
    assert np.isfinite(np.delete(fe, 4, axis=1)).all()
    assert_within(fe, off_, lse_f32_bound(m_pad_of(M)))


def extreme_problem():
    """test_gpu_kernels.test_loglik_extreme_parameter_ranges's data: tiny and huge variances, far offsets, weights over
    12 decades, far-away frames (costs ~1e6)."""
    rng = np.random.default_rng(77)
    S, M, D, N = 6, 8, 13, 200
    means = rng.normal(size=(S, M, D)) * np.array([1e-3, 1.0, 30.0, 1e3, 1.0, 1.0])[:, None, None]
    vars_ = 10.0 ** rng.uniform(-6, 6, size=(S, M, D))
    vars_[4] = 10.0 ** rng.uniform(-1, 1, size=(M, D))
    w = 10.0 ** rng.uniform(-12, 0, size=(S, M))
    X = rng.normal(size=(N, D)) * 3.0
    X[:50] += means[3, 0]
    X[50:60] *= 1e3
    return means, vars_, w, X


def test_extreme_parameter_ranges(hip, ctx_ref, ctx_fe):
    """With the reference's underflow rule (+inf at the same entries) and in the log domain, where costs reach ~1e6."""
    means, vars_, w, X = extreme_problem()
    off = [0, len(X)]
    B = lse_f32_bound(8)
    off_ = loglik_on(hip, ctx_ref, means, vars_, w, X, off)
    fe = loglik_on(hip, ctx_fe, means, vars_, w, X, off)
    assert np.isposinf(off_).any() and np.isfinite(off_).any()
    assert_within(fe, off_, B)
    c_fe, c_ref = hip.Context(0), hip.Context(0)
    try:
        c_fe.set_compat(underflow=False, lse_f32=True)
        c_ref.set_compat(underflow=False, lse_f32=False)
        fe_log = loglik_on(hip, c_fe, means, vars_, w, X, off)
        ref_log = loglik_on(hip, c_ref, means, vars_, w, X, off)
    finally:
        c_fe.close()
        c_ref.close()
    assert np.isfinite(fe_log).all() and (np.abs(ref_log) > 1e5).any()
    assert_within(fe_log, ref_log, B)


# ---------------------------------------------------------------------------- (d) where the flag changes nothing
@pytest.mark.parametrize("M,D,dtype", [(8, 39, np.float32), (32, 13, np.float32), (1, 13, np.float64), (2, 39, np.float64),
                                       (2, 7, np.float64), (8, 70, np.float64), (3, 70, np.float64)])
def test_flag_changes_nothing(hip, ctx_ref, ctx_fe, M, D, dtype):
    """fp32 batches, M_pad < 4 (M = 1, 2) and D = 70 (the vector kernel) never take the fp32 epilogue: bitwise equal."""
    rng = np.random.default_rng(7 * M + D)
    S, N = 9, 150
    means, vars_, w = random_model(rng, S, M, D)
    X = rng.normal(size=(N, D))
    off = [0, 1, 64, N]
    np.testing.assert_array_equal(loglik_on(hip, ctx_fe, means, vars_, w, X, off, dtype=dtype),
                                  loglik_on(hip, ctx_ref, means, vars_, w, X, off, dtype=dtype))


# ---------------------------------------------------------------------------- (e) non-finite results
@pytest.mark.parametrize("M", [4, 16, 48])
def test_nan_feature(hip, ctx_ref, ctx_fe, M):
    rng = np.random.default_rng(90 + M)
    S, D, N = 5, 13, 100
    means, vars_, w = random_model(rng, S, M, D)
    X = rng.normal(size=(N, D))
    X[3, 2] = np.nan
    X[40, 0] = np.nan
    off_ = loglik_on(hip, ctx_ref, means, vars_, w, X, [0, N])
    fe = loglik_on(hip, ctx_fe, means, vars_, w, X, [0, N])
    assert np.isnan(fe[[3, 40]]).all()
    assert_within(fe, off_, lse_f32_bound(m_pad_of(M)))


@pytest.mark.parametrize("M,D", [(4, 5), (8, 39), (32, 39)])
def test_underflow_rule_same_infinities(hip, ctx_ref, ctx_fe, M, D):
    """The +inf of the reference's linear-domain rule is decided on the fp64 maximum: the same entries in both modes,
    the finite ones within the bound.  With the rule off (a context pair of its own) every cost is finite."""
    rng = np.random.default_rng(M * 100 + D)
    S, N = 6, 96
    means, vars_, w = random_model(rng, S, M, D)
    X = rng.normal(size=(N, D))
    X[::3] += 30.0 * np.sign(rng.normal(size=(N // 3, D)))
    off = [0, 40, N]
    B = lse_f32_bound(m_pad_of(M))
    off_ = loglik_on(hip, ctx_ref, means, vars_, w, X, off)
    fe = loglik_on(hip, ctx_fe, means, vars_, w, X, off)
    assert np.isposinf(off_[::3]).all() and np.isfinite(off_[1::3]).all()
    assert_within(fe, off_, B)
    c_fe, c_ref = hip.Context(0), hip.Context(0)
    try:
        c_fe.set_compat(underflow=False, lse_f32=True)
        c_ref.set_compat(underflow=False, lse_f32=False)
        fe_log = loglik_on(hip, c_fe, means, vars_, w, X, off)
        ref_log = loglik_on(hip, c_ref, means, vars_, w, X, off)
    finally:
        c_fe.close()
        c_ref.close()
    assert np.isfinite(fe_log).all()
    assert_within(fe_log, ref_log, B)
    assert_within(fe_log, oracle_chunked(X, means, vars_, w), B, rel=1e-11)


@pytest.mark.parametrize("M,D", [(4, 13), (8, 39), (32, 13)])
def test_underflow_rule_with_normalisers_above_one(hip, ctx_ref, ctx_fe, M, D):
    """Variances of 0.01 (log(w norm) > 0): gh_loglik_underflow_fix re-tests the band per component -- the same +inf
    entries in both modes, here and through a subset launch."""
    rng = np.random.default_rng(7 * M + D)
    S, N = 5, 120
    means = rng.normal(size=(S, M, D)) * 0.002
    vars_ = np.full((S, M, D), 0.01) * rng.uniform(0.9, 1.1, size=(S, M, D))
    w = rng.dirichlet(np.ones(M), size=S)
    X = rng.normal(size=(N, D)) * 0.1
    for i in range(0, N, 2):
        d = rng.normal(size=D)
        X[i] = d / np.linalg.norm(d) * np.sqrt(2 * (700.0 + 90.0 * i / N) * 0.01)
    lognorm = -0.5 * (D * np.log(2 * np.pi) + np.sum(np.log(vars_), axis=2)) + np.log(w)
    assert (lognorm > 5).all()
    off = [0, 40, N]
    off_ = loglik_on(hip, ctx_ref, means, vars_, w, X, off)
    fe = loglik_on(hip, ctx_fe, means, vars_, w, X, off)
    assert np.isposinf(off_).sum() >= 20 and np.isfinite(off_).sum() >= N * S // 2
    assert_within(fe, off_, lse_f32_bound(m_pad_of(M)))
    lo, hi = np.zeros(2, dtype=np.int32), np.full(2, S, dtype=np.int32)
    sub = loglik_on(hip, ctx_fe, means, vars_, w, X, off, state_ranges=(lo, hi))
    np.testing.assert_array_equal(sub, fe)


# ---------------------------------------------------------------------------- (f) block-table launches
@pytest.mark.parametrize("S,M,D", [(70, 8, 39), (12, 3, 13), (9, 32, 7), (30, 16, 24), (11, 48, 22), (67, 11, 46)])
def test_subset_and_sets_equal_full_on_the_ranges(hip, ctx_fe, S, M, D):
    """gh_loglik_subset and gh_loglik_sets in this mode: bit-identical to the mode's full launch on their ranges."""
    rng = np.random.default_rng(S + M + D)
    means, vars_, w = random_model(rng, S, M, D)
    lens = [1, 31, 32, 33, 64, 100, 7, 150]
    off = np.concatenate([[0], np.cumsum(lens)])
    X = rng.normal(size=(int(off[-1]), D))
    U = len(lens)
    lo = rng.integers(0, S - 1, size=U).astype(np.int32)
    hi = np.minimum(S, lo + rng.integers(1, 7, size=U)).astype(np.int32)
    lo[0], hi[0] = 0, min(S, 5)
    lo[-1], hi[-1] = max(0, S - 5), S
    full = loglik_on(hip, ctx_fe, means, vars_, w, X, off)
    sub = loglik_on(hip, ctx_fe, means, vars_, w, X, off, state_ranges=(lo, hi))
    for u in range(U):
        np.testing.assert_array_equal(sub[off[u]:off[u + 1], lo[u]:hi[u]], full[off[u]:off[u + 1], lo[u]:hi[u]])
    # several ranges per utterance (the words of a transcript), some of them touching or overlapping
    r_off, r_lo, r_hi = [0], [], []
    for u in range(U):
        k = 1 + u % 3
        a = rng.integers(0, S - 1, size=k)
        r_lo += list(a)
        r_hi += list(np.minimum(S, a + rng.integers(1, 5, size=k)))
        r_off.append(r_off[-1] + k)
    sets = loglik_on(hip, ctx_fe, means, vars_, w, X, off, state_sets=(r_off, r_lo, r_hi))
    for u in range(U):
        for r in range(r_off[u], r_off[u + 1]):
            np.testing.assert_array_equal(sets[off[u]:off[u + 1], r_lo[r]:r_hi[r]], full[off[u]:off[u + 1], r_lo[r]:r_hi[r]])


# ---------------------------------------------------------------------------- (g) the environment switch
def test_environment_switch(hip, ctx_ref, ctx_fe, monkeypatch):
    """GMMHMM_LSE=f32exp before a context is created == set_compat(underflow=True, lse_f32=True)."""
    rng = np.random.default_rng(3)
    S, M, D, N = 20, 8, 39, 200
    means, vars_, w = random_model(rng, S, M, D)
    X = rng.normal(size=(N, D))
    monkeypatch.delenv("GMMHMM_COMPAT", raising=False)
    monkeypatch.setenv("GMMHMM_LSE", "f32exp")
    c = hip.Context(0)
    try:
        env = loglik_on(hip, c, means, vars_, w, X, [0, N])
    finally:
        c.close()
    fe = loglik_on(hip, ctx_fe, means, vars_, w, X, [0, N])
    np.testing.assert_array_equal(env, fe)
    assert not np.array_equal(fe, loglik_on(hip, ctx_ref, means, vars_, w, X, [0, N]))


# ---------------------------------------------------------------------------- (h) consumers
def test_viterbi_end_costs_within_frames_times_bound(hip, ctx_ref, ctx_fe):
    """A K = 3 word lattice over configs[2]-style words: every end cost moves by at most T_u B (plus fp64 rounding of
    the path sums); the unreachable ends (+inf: too few frames for K words) are the same."""
    import bench
    from sr.recognition.continuous_speech import packed_lattice
    K = 3
    wl = bench.synth_workload(11, 60, W=6, n=5, M=8, D=39, tmin=8, tmax=120)
    W, n, M, D = wl["W"], wl["n"], wl["M"], wl["D"]
    S = W * n
    off = np.asarray(wl["off"], dtype=np.int64)
    lens = np.diff(off)
    graph = packed_lattice([wl["trans"]] * W, n, [list(range(W))] * K)[0]
    ends = {}
    for name, c in (("off", ctx_ref), ("fe", ctx_fe)):
        gmm = hip.PackedGMM(c, wl["means"].reshape(S, M, D), wl["vars"].reshape(S, M, D), wl["w"].reshape(S, M))
        b = hip.Batch(c, feats=wl["X"], offsets=off)
        lat = hip.Lattices(c, [graph])
        b.loglik(gmm, fetch=False)
        r = lat.viterbi(b, utt_lattice=np.zeros(b.U, dtype=np.int32), want_path=False)
        ends[name] = [e.copy() for e in r["end_cost"]]
        lat.close(); b.close(); gmm.close()
    B = lse_f32_bound(8)
    n_inf = 0
    for u, (a, e) in enumerate(zip(ends["fe"], ends["off"])):
        np.testing.assert_array_equal(np.isposinf(a), np.isposinf(e))
        n_inf += int(np.isposinf(e).sum())
        fin = np.isfinite(e)
        assert np.isfinite(a[fin]).all()
        tol = lens[u] * B + FP64_REL * lens[u] * np.abs(e[fin])
        assert np.all(np.abs(a[fin] - e[fin]) <= tol), u
    assert n_inf > 0 and any(np.isfinite(e).any() for e in ends["off"])


@pytest.mark.parametrize("form", ["subset", "full"])
def test_em_session_log_probability_within_frames_times_bound(hip, ctx_ref, ctx_fe, monkeypatch, form):
    """The word-string EM session's first log P (before the update), flag on against flag off: |delta| <= N B, through
    the block-table likelihood launch (GMMHMM_EM_LL=subset) and the full matrix (=full)."""
    import bench
    U, K = 60, 3
    wl = bench.synth_workload(1003, U * K)
    W, n, M, D = wl["W"], wl["n"], wl["M"], wl["D"]
    S = W * n
    off = np.asarray(wl["off"])[::K]
    labels = [tuple(int(x) for x in wl["words"].reshape(U, K)[u]) for u in range(U)]
    distinct = sorted(set(labels))
    utt = np.array([distinct.index(l) for l in labels], dtype=np.int32)
    means = wl["means"].reshape(S, M, D) + 0.3 * np.random.default_rng(0).normal(size=(S, M, D))
    vars_, w = wl["vars"].reshape(S, M, D), wl["w"].reshape(S, M)
    trans = np.stack([wl["trans"]] * W)
    monkeypatch.setenv("GMMHMM_EM_LL", form)
    logp = {}
    for name, c in (("off", ctx_ref), ("fe", ctx_fe)):
        b = hip.Batch(c, feats=wl["X"][:off[-1]], offsets=off)
        sess = hip.EMSession(c, b, means, vars_, w, trans, utt, var_floor=1e-3, transcripts=[list(l) for l in distinct])
        try:
            logp[name] = sess.iteration()[0]
        finally:
            sess.close()
            b.close()
    N = int(off[-1])
    assert np.isfinite(logp["off"])
    # (the forward-backward's own fp64 rounding: 1e-12 of |log P|, far below N B)
    assert abs(logp["fe"] - logp["off"]) <= N * lse_f32_bound(8) + 1e-12 * abs(logp["off"])
