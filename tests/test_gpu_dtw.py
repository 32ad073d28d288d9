# -*- coding: utf-8 -*-
"""The template DP on the device (gh_dtw.hip: dtw_kernel through gh_dtw and gh_fit_dtw) against tests/dtw_ref.py.

Inputs come from the seeded builders of dtw_ref.py; tests/test_dtw_ref_host.py shows on the CPU that every one of them
keeps its decisions further apart than 1e-9 (paths can be compared exactly), that the walk ends, and that it reaches the
launch form / branch it is named for.  Paths are compared exactly.  Costs: the +inf / -inf pattern and the beam's -1 marks
equal; finite costs of the built-in distances within rtol 1e-11 of dtw_ref on the long-double distance matrix (variances
in [0.5, 2]: every term of a cost is positive, rounding is bounded by about (D + T) 2^-53 <= 2e-13 at the largest case:
50 x margin); costs from a caller's matrix bitwise (the DP itself is one addition per arc and one per cell, in the
oracle's order).
  1. every launch form x Euclidean / mahalanobis / dist=;  2. frame staging strides;  3. beam edges, -1 marks in both
  waves, finite ties at the cut;  4. NaN / -inf arcs;  5. back-traces that cross the LDS window;  6. ragged batches and
  batch position;  7. the distance-matrix route on an fp32 batch;  8. refusals;  9. the public routes;  10. gh_fit_dtw."""
import numpy as np
import pytest

import dtw_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-11
MAX_ERR = {"euclid": 0.0, "mahalanobis": 0.0}


@pytest.fixture(scope="module")
def SR():
    import sr.recognition as SR
    return SR


@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest relative cost error (bound %g): %s" % (RTOL, ", ".join("%s %.3g" % kv for kv in sorted(MAX_ERR.items()))))


def check(costs, path, ref, kind):
    """kind "euclid" / "mahalanobis": rtol 1e-11; anything else: bitwise."""
    rc, rp = ref[0], ref[1]
    np.testing.assert_array_equal(path, rp)
    assert costs.shape == rc.shape and not np.isnan(costs).any()
    for pattern in (np.isposinf, np.isneginf, lambda a: a == -1.0):
        np.testing.assert_array_equal(pattern(costs), pattern(rc))
    fin = np.isfinite(rc) & (rc != -1.0)
    if kind in MAX_ERR:
        if fin.any():
            err = float(np.max(np.abs(costs[fin] - rc[fin]) / np.abs(rc[fin])))
            MAX_ERR[kind] = max(MAX_ERR[kind], err)
            assert err <= RTOL, err
    else:
        np.testing.assert_array_equal(costs[fin], rc[fin])


def beam_arg(beam):
    return 0 if np.isinf(beam) else int(beam)


def run(batch, case, kind, beam=np.inf, want_costs=True, dist=None):
    if kind == "euclid":
        return batch.dtw(case["trans"], y=case["y"], beam=beam_arg(beam), want_costs=want_costs)
    if kind == "mahalanobis":
        return batch.dtw(case["trans"], y=case["y"], var=case["var"], beam=beam_arg(beam), want_costs=want_costs)
    return batch.dtw(case["trans"], dist=R.case_dists(case, "euclid") if dist is None else dist, beam=beam_arg(beam),
                     want_costs=want_costs)


def run_job(hip, ctx, name, kind, beam=np.inf):
    case = R.jobs()[name]["case"]
    b = hip.Batch(ctx, case["xs"])
    try:
        costs, paths = run(b, case, kind, beam)
    finally:
        b.close()
    ref = R.reference(name, kind, beam)
    for u in range(len(case["xs"])):
        check(costs[u], paths[u], ref[u], kind)
    return costs, paths


# ---------------------------------------------------------------------------------------- 1. instantiation x distance
# staged uint8 in one wave (n = 2, 5, 64) and in several (65, 100); unstaged uint8 by size (128, 255) and by D > 4 threads
# (n = 5, D = 257); unstaged uint16 (256, 300).  dtw_kernel<uint16_t, true> is never launched: from 256 rows on the arcs
# alone take 512 KB, and staging stops at 96 KB (test_dtw_ref_host.py::test_instantiation_cases_take_their_launch_form).
@pytest.mark.parametrize("kind", R.KINDS3)
@pytest.mark.parametrize("name", R.job_names("inst"))
def test_every_launch_form(hip, ctx, name, kind):
    run_job(hip, ctx, name, kind)


# ------------------------------------------------------------------------------------------- 2. frame staging strides
# one wave: thread i parks frame elements i, i + 64, i + 128, i + 192 (D up to 256 staged).  The two-wave cases run
# unstaged: 70 rows at D >= 127 do not fit the 96 KB (no staged launch of several waves has D above its thread count).
@pytest.mark.parametrize("kind", R.KINDS2)
@pytest.mark.parametrize("name", R.job_names("stride"))
def test_frame_staging_strides(hip, ctx, name, kind):
    run_job(hip, ctx, name, kind)


# -------------------------------------------------------------------------------------------------------------- 3. beam
@pytest.mark.parametrize("kind", R.KINDS2)
@pytest.mark.parametrize("name", R.job_names("beam"))
def test_beam_edges(hip, ctx, name, kind):
    job = R.jobs()[name]
    n = job["case"]["n"]
    assert job["beams"] == (1, 2, n - 1, n, n + 5)
    b = hip.Batch(ctx, job["case"]["xs"])
    try:
        c0, p0 = run(b, job["case"], kind)
        for beam in job["beams"]:
            costs, paths = run(b, job["case"], kind, beam)
            ref = R.reference(name, kind, beam)
            for u in range(len(costs)):
                check(costs[u], paths[u], ref[u], kind)       # (-1 exactly where dtw_ref has it, the second wave included)
                if beam >= n:                                 # nothing to prune: bitwise the unpruned run
                    np.testing.assert_array_equal(costs[u], c0[u])
                    np.testing.assert_array_equal(paths[u], p0[u])
    finally:
        b.close()


@pytest.mark.parametrize("n,beam", [(5, 3), (70, 40)])
def test_beam_ties_fall_to_the_smaller_row(hip, ctx, n, beam):
    """Integer costs (exact sums): equal finite costs on both sides of the cut, for n = 70 in rows of both waves."""
    E, trans, beam = R.int_tie_case(n, 8, beam)
    rc, rp, gap, st = R.dtw_ref(E, trans, beam=beam, stable=True, want_stats=True)
    assert st["cut_ties"] > 0 and (n <= 64 or st["cut_ties_cross"] > 0)
    b = hip.Batch(ctx, [np.zeros((E.shape[1], 2))])
    try:
        costs, paths = b.dtw(trans, dist=[E], beam=beam)
    finally:
        b.close()
    check(costs[0], paths[0], (rc, rp), "dist")


def test_row0_drops_marked_origins(hip, ctx):
    """Cell (0, 2) has only +inf candidates once the marked origin 0 is dropped from row 0's list: it points at origin 1."""
    E, trans, beam = R.row0_drop_case()
    b = hip.Batch(ctx, [np.zeros((E.shape[1], 2))])
    try:
        costs, paths = b.dtw(trans, dist=[E], beam=beam)
    finally:
        b.close()
    check(costs[0], paths[0], R.dtw_ref(E, trans, beam=beam), "dist")
    np.testing.assert_array_equal(paths[0], [[0, 2], [1, 1], [0, 0]])


# ------------------------------------------------------------------------------------------------- 4. NaN / -inf arcs
@pytest.mark.parametrize("kind", R.KINDS2)
@pytest.mark.parametrize("name", R.job_names("nan"))
def test_nan_and_neginf_arcs(hip, ctx, name, kind):
    """The first NaN candidate wins and costs +inf; -inf arcs on the winning path (end cost -inf) and off it; a cell whose
    candidates are all +inf points at the first one (the walks of the short utterances pass through such cells)."""
    costs, _ = run_job(hip, ctx, name, kind)
    assert any(np.isneginf(c[-1, -1]) for c in costs) and any(np.isposinf(c[-1, -1]) for c in costs)


# ------------------------------------------------------------------------------------------- 5. back-trace windows
@pytest.mark.parametrize("name", R.job_names("window"))
def test_backtrace_across_its_window(hip, ctx, name):
    """T in {w-1, w, w+1, 2w+1} around the window of w back-pointer columns, a two-frame utterance in the same batch."""
    case = R.jobs()[name]["case"]
    assert [len(x) for x in case["xs"]][1] == 2
    run_job(hip, ctx, name, "euclid")


# ---------------------------------------------------------------------------------------- 6. batches and position
@pytest.mark.parametrize("beamed", [False, True])
@pytest.mark.parametrize("kind", R.KINDS2)
@pytest.mark.parametrize("name", R.job_names("batch"))
def test_batch_position(hip, ctx, name, kind, beamed):
    job = R.jobs()[name]
    case, beam = job["case"], job["beams"][1 if beamed else 0]
    xs = case["xs"]
    U = len(xs)
    base_c, base_p = run_job(hip, ctx, name, kind, beam)

    def same(order):
        b = hip.Batch(ctx, [xs[u] for u in order])
        try:
            costs, paths = run(b, case, kind, beam)
            no_costs, paths_only = run(b, case, kind, beam, want_costs=False)
        finally:
            b.close()
        assert no_costs is None
        for k, u in enumerate(order):
            np.testing.assert_array_equal(costs[k], base_c[u])
            np.testing.assert_array_equal(paths[k], base_p[u])
            np.testing.assert_array_equal(paths_only[k], base_p[u])

    for u in range(U):
        same([u])                                             # alone
        same([(u + k) % U for k in range(U)])                 # u first, u - 1 last
    same(list(range(U))[::-1])                                # reversed


# ------------------------------------------------------------------------------ 7. distance matrices on an fp32 batch
@pytest.mark.parametrize("name", R.job_names("batch"))
def test_distance_matrix_route_on_fp32_batch(hip, ctx, name):
    case = R.jobs()[name]["case"]
    dist = R.case_dists(case, "euclid")
    b64, b32 = hip.Batch(ctx, case["xs"]), hip.Batch(ctx, case["xs"], dtype=np.float32)
    try:
        c64, p64 = run(b64, case, "dist", dist=dist)
        c32, p32 = run(b32, case, "dist", dist=dist)
        for kind in R.KINDS2:
            with pytest.raises(hip.BackendError, match="built-in distances need an fp64 batch"):
                run(b32, case, kind)
        c32b, p32b = run(b32, case, "dist", dist=dist)       # the batch still works after the refusal
    finally:
        b64.close()
        b32.close()
    ref = R.reference(name, "dist", np.inf)
    for u in range(len(dist)):
        check(c64[u], p64[u], ref[u], "dist")
        for c, p in ((c32, p32), (c32b, p32b)):
            np.testing.assert_array_equal(c[u], c64[u])
            np.testing.assert_array_equal(p[u], p64[u])


# ------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(hip, ctx):
    name = "inst-n5-D13"
    case = R.jobs()[name]["case"]
    D = case["D"]

    def still_good():
        run_job(hip, ctx, name, "euclid")

    b = hip.Batch(ctx, case["xs"])
    try:
        with pytest.raises(hip.BackendError, match=r"gh_dtw: n=1 \(2\.\.1024"):
            b.dtw(np.zeros((1, 1)), y=np.zeros((1, D)))
        still_good()
        with pytest.raises(hip.BackendError, match=r"gh_dtw: n=1025 \(2\.\.1024"):
            b.dtw(np.zeros((1025, 1025)), y=np.zeros((1025, D)))
        still_good()
        with pytest.raises(hip.BackendError, match="need template rows or a distance matrix"):
            b.dtw(case["trans"])
        still_good()
    finally:
        b.close()
    rng = np.random.default_rng(8)
    b = hip.Batch(ctx, [rng.normal(size=(T, D)) for T in (6, 1, 7)])
    try:
        with pytest.raises(hip.BackendError, match="utterance 1 has fewer than 2 frames"):
            b.dtw(case["trans"], y=case["y"])
    finally:
        b.close()
    still_good()
    # cell (0,0) cannot be reached from the end cell: row 1 only ever reads its own NaN (-inf + inf) self loop
    trans = np.array([[0.3, np.inf], [0.7, -np.inf]])
    with pytest.raises(ValueError, match="back-trace left the matrix"):
        R.dtw_ref(np.ones((2, 4)), trans)
    b = hip.Batch(ctx, [rng.normal(size=(4, D)), rng.normal(size=(9, D))])
    try:
        with pytest.raises(hip.BackendError, match="back-trace left the matrix"):
            b.dtw(trans, y=rng.normal(size=(2, D)))
    finally:
        b.close()
    still_good()


# -------------------------------------------------------------------------------------------------- 9. public routes
def test_public_dtw_callable_equals_fast_path(SR):
    from sr.recognition.hmm_state import euclidean
    case = R.jobs()["batch-n70"]["case"]
    u = int(np.argmax([len(x) == 45 for x in case["xs"]]))
    x = case["xs"][u]
    cf, pf = SR.dtw(x, case["y"], euclidean, case["trans"])
    cc, pc = SR.dtw(x, case["y"], lambda a, b: np.sqrt(np.sum((a - b) ** 2)), case["trans"])      # scored per cell on the host
    ref = R.reference("batch-n70", "euclid", np.inf)[u]
    check(cf, pf, ref, "euclid")
    np.testing.assert_array_equal(pc, pf)
    np.testing.assert_array_equal(np.isinf(cc), np.isinf(cf))
    np.testing.assert_allclose(cc[np.isfinite(cc)], cf[np.isfinite(cf)], rtol=RTOL)


def test_single_gaussian_hmm_evaluate(SR):
    name = "inst-n5-D13"
    case = R.jobs()[name]["case"]
    h = SR.HMM(case["n"])
    h.use_gmm = False
    h.mu, h.sigma, h.transitions = case["y"].copy(), case["var"].copy(), case["trans"].copy()
    for u, x in enumerate(case["xs"]):
        end = R.reference(name, "mahalanobis", np.inf)[u][0][-1, -1]
        assert np.isfinite(end)
        np.testing.assert_allclose(h.evaluate(x), end, rtol=RTOL)


# ------------------------------------------------------------------------------------------------------ 10. gh_fit_dtw
# The session refuses more than 32 groups and more than 64 dimensions (gh_fit_create), so gh_fit_dtw is reachable for
# n = 2 .. 32 at D <= 64 only: its own n <= 255 bound can never decide.
SENTINEL = -7


def fit_session(hip, ctx, case, kmax):
    b = hip.Batch(ctx, case["xs"])
    seg_off = b.offsets[::R.FIT_PER_WORD]                      # FIT_W blocks of FIT_PER_WORD utterances
    return b, hip.FitSession(ctx, b, seg_off, kmax), seg_off


@pytest.mark.parametrize("D", [5, 64])
@pytest.mark.parametrize("n", [2, 5, 32])
def test_fit_dtw(hip, ctx, n, D):
    case = R.fit_case(n, D)
    xs, um = case["xs"], case["utt_word"]
    ref = R.fit_reference(case)
    b, fit, seg_off = fit_session(hip, ctx, case, max(n, 2))
    off = b.offsets
    try:
        fit.set_ids(np.full(b.N, SENTINEL, dtype=np.int32))
        fit.dtw(n, case["y"], case["trans"], um)
        rows = fit.clusters()
        for u, x in enumerate(xs):                            # the row of every frame == Batch.dtw's path == dtw_ref's
            one = hip.Batch(ctx, [x])
            try:
                _, paths = one.dtw(case["trans"][um[u]], y=case["y"][um[u]], want_costs=False)
            finally:
                one.close()
            mine = rows[off[u]:off[u + 1]]
            assert mine[-1] == n - 1
            np.testing.assert_array_equal(mine, R.row_sequence(paths[0], n, len(x)))
            np.testing.assert_array_equal(mine, R.row_sequence(ref[u][1], n, len(x)))
        # group statistics of those ids: per (block of the session, row) numpy's mean and ddof-1 variance
        mean, var, cnt = fit.group_stats(n)
        X = np.concatenate(xs)
        for s in range(R.FIT_W):
            seg, ids = X[seg_off[s]:seg_off[s + 1]], rows[seg_off[s]:seg_off[s + 1]]
            for k in range(n):
                sel = seg[ids == k]
                assert cnt[s, k] == len(sel)
                if len(sel):
                    np.testing.assert_allclose(mean[s, k], sel.mean(axis=0), rtol=1e-12, atol=1e-12)
                if len(sel) > 1:
                    np.testing.assert_allclose(var[s, k], sel.var(axis=0, ddof=1), rtol=1e-12, atol=1e-12)
        # an inactive word keeps what set_ids wrote, the others are aligned as before
        fit.set_ids(np.full(b.N, SENTINEL, dtype=np.int32))
        fit.dtw(n, case["y"], case["trans"], um, active=[1, 0, 1])
        part = fit.clusters()
        for u in range(len(xs)):
            want = SENTINEL if um[u] == 1 else rows[off[u]:off[u + 1]]
            np.testing.assert_array_equal(part[off[u]:off[u + 1]], want)
    finally:
        fit.close()
        b.close()


def test_fit_dtw_refusals(hip, ctx):
    case = R.fit_case(5, 5)
    um = case["utt_word"]
    b, fit, _ = fit_session(hip, ctx, case, 8)
    try:
        for n in (256, 9):                                    # beyond 255 rows; beyond the session's kmax
            y, trans = np.zeros((R.FIT_W, n, 5)), np.zeros((R.FIT_W, n, n))
            with pytest.raises(hip.BackendError, match=r"gh_fit_dtw: n=%d \(2\.\.min\(255, kmax=8\)\)" % n):
                fit.dtw(n, y, trans, um)
        bad = um.copy()
        bad[4] = R.FIT_W
        with pytest.raises(hip.BackendError, match=r"gh_fit_dtw: utt_model\[4\]=3"):
            fit.dtw(5, case["y"], case["trans"], bad)
        fit.dtw(5, case["y"], case["trans"], um)              # the session still works
        ref = R.fit_reference(case)
        rows = fit.clusters()
        for u, x in enumerate(case["xs"]):
            np.testing.assert_array_equal(rows[b.offsets[u]:b.offsets[u + 1]], R.row_sequence(ref[u][1], 5, len(x)))
    finally:
        fit.close()
        b.close()
    rng = np.random.default_rng(3)
    b = hip.Batch(ctx, [rng.normal(size=(T, 5)) for T in (6, 1, 7)])
    fit = hip.FitSession(ctx, b, b.offsets, 8)
    try:
        with pytest.raises(hip.BackendError, match="gh_fit_dtw: utterance 1 has fewer than 2 frames"):
            fit.dtw(5, case["y"], case["trans"], [0, 1, 2])
    finally:
        fit.close()
        b.close()


@pytest.mark.parametrize("n,D", [(64, 5), (70, 5), (255, 5), (5, 130)])
def test_fit_session_refuses_what_gh_fit_dtw_could_not_be_asked(hip, ctx, n, D):
    """Template counts above 32 and D above 64 never reach gh_fit_dtw: the session itself is refused."""
    rng = np.random.default_rng(n + D)
    b = hip.Batch(ctx, [rng.normal(size=(4, D)) for _ in range(3)])
    try:
        with pytest.raises((hip.BackendError, hip.Unsupported)):
            hip.FitSession(ctx, b, b.offsets, n)
    finally:
        b.close()
