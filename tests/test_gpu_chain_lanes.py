# -*- coding: utf-8 -*-
"""The lane = chain form of the chain Viterbi (viterbi_chain_lanes_kernel: graphs whose chains all have n <= 8 rows with
consecutive states; one lane walks one chain, several utterances share a wave, the end selection happens inside the sweep
when no path is wanted) against the lane = row form (viterbi_chain_kernel, GMMHMM_CHAIN=rows in a fresh child process).

Everything is compared BIT FOR BIT (the raw bytes, so that NaN patterns and signs of zero count): end costs, best ends,
paths, the per-cell costs of want_costs, and the error text where a back-trace runs into a row without arcs.  The lane
form changes no arithmetic, so there is no tolerance to choose.  Cases: fp64 and fp32 batches; n in {1, 2, 3, 5, 8};
1, 7, 10, 13, 64 and 70 chains per graph (70: two waves per utterance, end selection by the separate kernel); with and
without skip arcs; rows without arcs; ragged lengths from 2 frames up; emissions holding +inf, -inf and NaN; several
back-pointer chunks.  The G3 / G6 fixtures go through the lane form against their stored outputs, and the headline
graph of bench.py must take the lane form.

Run as a script (`python tests/test_gpu_chain_lanes.py OUT.npz`) the file computes every case with the kernel the
environment selects and stores the results: that is the child process of the comparison."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "speech-recognition_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 5, 8)
CHAINS = (1, 7, 10, 13, 64, 70)
DTYPES = {"f64": np.float64, "f32": np.float32}


# ------------------------------------------------------------------------------------------------------- the cases
def chain_graph(rng, n, C, skip, holes, n_blocks):
    """C chains of n rows.  Chain c reads the states of a randomly drawn block (blocks repeat: equal chains give equal end
    costs, the last one listed has to win).  holes: rows without any arc -- the first row of a chain without its self arc,
    and, under a skip arc (the only way a chain stays one chain), a row in the middle."""
    R = C * n
    block = rng.integers(0, n_blocks, size=C)
    row_state = (block[:, None] * n + np.arange(n)[None, :]).ravel()
    to, frm, cost = [], [], []
    for c in range(C):
        dead = set()
        if holes and C > 1 and rng.random() < 0.3:
            dead.add(0)
        if holes and skip and n >= 3 and rng.random() < 0.4:
            dead.add(int(rng.integers(1, n - 1)))
        for i in range(n):
            r = c * n + i
            if i in dead:
                continue
            if i == 0 or rng.random() < 0.85:                      # self arc
                to.append(r); frm.append(r); cost.append(rng.uniform(0.0, 2.0))
            if i >= 1:                                             # r-1 -> r: always there (it is what makes a chain)
                to.append(r); frm.append(r - 1); cost.append(rng.uniform(0.0, 2.0))
            if skip and i >= 2 and (i + 1 in dead or i - 1 in dead or rng.random() < 0.7):
                to.append(r); frm.append(r - 2); cost.append(rng.uniform(0.0, 2.0))
        if skip and n >= 3 and not any(f == t - 2 for t, f in zip(to, frm) if c * n <= t < (c + 1) * n):
            to.append(c * n + 2); frm.append(c * n); cost.append(rng.uniform(0.0, 2.0))
    cost = np.asarray(cost)
    cost[rng.random(len(cost)) < 0.1] = 0.0                          # -log 1
    start = [c * n for c in range(C)] + [c * n + 1 for c in range(C) if n >= 2 and rng.random() < 0.2]
    end = [c * n + n - 1 for c in range(C)] + [c * n + n // 2 for c in range(C) if n >= 3 and rng.random() < 0.2]
    end = [int(e) for e in rng.permutation(end)]
    return dict(row_state=row_state, arc_to=np.asarray(to), arc_from=np.asarray(frm), arc_cost=cost,
                start_rows=start, end_rows=end)


def write_emissions(hip, ctx, batch, nll):
    """Replace the resident [N, S] likelihood matrix (the library has no call for it: no model produces -inf).  The HIP
    runtime is the one the library has already loaded, found through the process's own mappings."""
    import ctypes
    ctx.sync()
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    rt = ctypes.CDLL(path)
    rt.hipMemcpy.restype = ctypes.c_int
    rt.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    dev = hip.load_library().gh_loglik_dev_ptr(batch.h)
    assert dev
    nll = np.ascontiguousarray(nll)
    assert rt.hipMemcpy(dev, nll.ctypes.data, nll.nbytes, 1) == 0       # hipMemcpyHostToDevice
    assert rt.hipDeviceSynchronize() == 0


def decode(lat, b, **kw):
    """One call, every output as raw bytes; a refused back-trace (a path that runs into a row without arcs) is a result."""
    from sr.recognition._hip import BackendError
    try:
        r = lat.viterbi(b, **kw)
    except BackendError as e:
        return {"error": np.frombuffer(str(e).encode(), dtype=np.uint8)}
    out = {"end_cost": r["end_cost_flat"].view(np.uint8), "best_end": r["best_end"]}
    if "paths" in r:
        out["path_len"] = np.array([len(p) for p in r["paths"]])
        out["paths"] = np.concatenate([p.ravel() for p in r["paths"]]) if r["paths"] else np.zeros(0, np.int64)
    if "costs" in r:
        out["costs"] = np.concatenate([c.ravel() for c in r["costs"]]).view(np.uint8)
    return out


def run_case(hip, ctx, dt, n, skip):
    """Every chain count of one (dtype, n, skip): {key: array}."""
    from test_gpu_seq import forced
    out = {}
    rng = np.random.default_rng(1000 * n + 10 * skip + (dt == "f32"))
    n_blocks, M, D = 9, 2, 4
    S = n_blocks * n
    gmm = hip.PackedGMM(ctx, rng.normal(size=(S, M, D)), rng.uniform(0.5, 1.5, size=(S, M, D)), rng.dirichlet(np.ones(M), size=S))
    for C in CHAINS:
        U = 45 if C <= 13 else 7
        T = rng.integers(2, 41, size=U)
        T[rng.random(U) < 0.25] = rng.integers(2, 5)
        xs = [rng.normal(size=(t, D)) for t in T]
        for variant in ("clean", "holes"):
            b = hip.Batch(ctx, xs, dtype=DTYPES[dt])
            nll = b.loglik(gmm)
            if variant == "holes":
                mark = rng.random(nll.shape)
                nll[mark < 0.04] = np.inf
                nll[(mark >= 0.04) & (mark < 0.05)] = -np.inf
                nll[(mark >= 0.05) & (mark < 0.06)] = np.nan
                nll[(mark >= 0.06) & (mark < 0.07)] = 0.0
                write_emissions(hip, ctx, b, nll)
            lat = hip.Lattices(ctx, [chain_graph(rng, n, C, skip, variant == "holes", n_blocks)])
            assert "chain" in lat.forms()
            calls = {"ends": dict(want_path=False), "path": dict(want_path=True),
                     "costs": dict(want_path=False, want_costs=True), "path+costs": dict(want_path=True, want_costs=True)}
            for name, kw in calls.items():
                for k, v in decode(lat, b, **kw).items():
                    out["C%d/%s/%s/%s" % (C, variant, name, k)] = v
            with forced(GMMHMM_SCRATCH_BUDGET=str(int(T.sum()) * C * n // 4)):      # an eighth of what the planner counts for the batch
                for k, v in decode(lat, b, want_path=True).items():
                    out["C%d/%s/chunked/%s" % (C, variant, k)] = v
                out["C%d/%s/chunked/n" % (C, variant)] = np.array([ctx.last_chunks])
            b.close(); lat.close()
    gmm.close()
    return out


def all_cases():
    return [(dt, n, skip) for dt in DTYPES for n in NS for skip in (False, True) if n >= 3 or not skip]


def main(out_path):
    from sr.recognition import _hip as hip
    ctx = hip.default_context()
    res = {}
    for dt, n, skip in all_cases():
        for k, v in run_case(hip, ctx, dt, n, skip).items():
            res["%s/n%d/skip%d/%s" % (dt, n, skip, k)] = v
    np.savez(out_path, **res)


# ------------------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def hip():
    from sr.recognition import _hip
    return _hip


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.default_context()


@pytest.fixture(scope="module")
def rows_results(tmp_path_factory):
    """Every case through the lane = row kernel, in a fresh process."""
    out = str(tmp_path_factory.mktemp("chain_rows") / "rows.npz")
    env = dict(os.environ, GMMHMM_CHAIN="rows", GMMHMM_HOST_TRACE="1")
    env.pop("GMMHMM_SCRATCH_BUDGET", None)
    flags = ["-s"] if sys.flags.no_user_site else []
    p = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__), out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "chain=rows" in p.stderr and "chain=lanes" not in p.stderr, "the child did not stay on the lane = row kernel"
    return np.load(out)


@pytest.mark.parametrize("dt,n,skip", all_cases())
def test_lane_form_equals_row_form(hip, ctx, rows_results, capfd, dt, n, skip):
    from test_gpu_seq import forced
    with forced(GMMHMM_HOST_TRACE="1"):
        os.environ.pop("GMMHMM_CHAIN", None)
        got = run_case(hip, ctx, dt, n, skip)
    err = capfd.readouterr().err
    assert "chain=lanes" in err and "chain=rows" not in err, "a case left the lane form"
    prefix = "%s/n%d/skip%d/" % (dt, n, skip)
    want = {k[len(prefix):]: rows_results[k] for k in rows_results.files if k.startswith(prefix)}
    assert sorted(want) == sorted(got)
    n_paths = 0
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
        n_paths += k.endswith("/path/paths")
        if k.endswith("chunked/n"):
            assert got[k][0] >= 3, (k, got[k])
    assert n_paths >= len(CHAINS)       # the clean graphs always give paths
    assert not any("/clean/" in k and k.endswith("/error") for k in got)


def _graph(row_state, trans, start_rows, end_rows):
    to, frm = np.nonzero(~np.isinf(trans))
    return dict(row_state=row_state, arc_to=to, arc_from=frm, arc_cost=trans[to, frm], start_rows=start_rows, end_rows=end_rows)


@pytest.mark.parametrize("tag", ["c1", "c2"])
def test_G3_isolated_decode_through_the_lane_form(hip, ctx, capfd, tag):
    """Every word model on its own (one chain per graph) and all of them stacked: costs, paths and evaluate() values of
    the stored reference outputs."""
    from conftest import load_golden
    from test_gpu_seq import forced
    g = load_golden("G3_isolated_decode_" + tag)
    means, vars_, w, trans = g["means"], g["vars"], g["w"], g["trans"]
    W, n, M, D = means.shape
    U = len(g["words"])
    gmm = hip.PackedGMM(ctx, means.reshape(W * n, M, D), vars_.reshape(W * n, M, D), w.reshape(W * n, M))
    b = hip.Batch(ctx, [g["x%d" % u] for u in range(U)])
    b.loglik(gmm, fetch=False)
    with forced(GMMHMM_HOST_TRACE="1"):
        for i in range(W):
            lat = hip.Lattices(ctx, [_graph(np.arange(n) + i * n, trans, [0], [n - 1])])
            r = lat.viterbi(b, want_costs=True)
            for u in range(U):
                ref = g["costs_%d_%d" % (u, i)]
                fin = ~np.isinf(ref)
                np.testing.assert_array_equal(np.isinf(r["costs"][u]), ~fin)
                np.testing.assert_allclose(r["costs"][u][fin], ref[fin], rtol=1e-10)
                np.testing.assert_array_equal(r["paths"][u], g["path_%d_%d" % (u, i)])
            lat.close()
        big = np.full((W * n, W * n), np.inf)
        for i in range(W):
            big[i * n:(i + 1) * n, i * n:(i + 1) * n] = trans
        st = hip.Lattices(ctx, [_graph(np.arange(W * n), big, [i * n for i in range(W)], [i * n + n - 1 for i in range(W)])])
        r = st.viterbi(b, want_path=False)
        rp = st.viterbi(b, want_path=True)
    err = capfd.readouterr().err
    assert "chain=lanes" in err and "chain=rows" not in err
    np.testing.assert_array_equal(r["end_cost_flat"].view(np.uint8), rp["end_cost_flat"].view(np.uint8))
    np.testing.assert_array_equal(r["best_end"], rp["best_end"])
    for u in range(U):
        np.testing.assert_allclose(r["end_cost"][u], g["evaluate_%d" % u], rtol=1e-10)
        best = int(r["best_end"][u])
        assert best == int(np.argmin(r["end_cost"][u])) == int(g["words"][u])
        np.testing.assert_array_equal(rp["paths"][u], g["path_%d_%d" % (u, best)] + np.array([best * n, 0]))
    b.close(); st.close(); gmm.close()


def test_G6_edges_through_the_lane_form(hip, ctx, capfd):
    """T = 2 with an unreachable end (the back-pointers of all-inf cells are still followed), equal end costs (the last
    listed end wins), an empty utterance (best end -1, no path)."""
    from conftest import load_golden
    from test_gpu_seq import forced
    g = load_golden("G6_decode_edges")
    means, vars_, w, trans = g["means"], g["vars"], g["w"], g["trans"]
    gmm = hip.PackedGMM(ctx, means, vars_, w)
    b = hip.Batch(ctx, [g["t2_x"], np.zeros((0, means.shape[2])), g["tie_x"]])
    b.loglik(gmm, fetch=False)
    twice = np.full((10, 10), np.inf)
    twice[:5, :5] = trans
    twice[5:, 5:] = trans
    with forced(GMMHMM_HOST_TRACE="1"):
        lat = hip.Lattices(ctx, [_graph(np.arange(5), trans, [0], [4])])
        r = lat.viterbi(b, want_costs=True)
        r0 = lat.viterbi(b, want_path=False)
        lat2 = hip.Lattices(ctx, [_graph(np.tile(np.arange(5), 2), twice, [0, 5], [4, 9])])
        r2 = lat2.viterbi(b, want_path=False)
        r2p = lat2.viterbi(b, want_path=True)
    err = capfd.readouterr().err
    assert "chain=lanes" in err and "chain=rows" not in err
    ref = g["t2_costs"]
    np.testing.assert_array_equal(np.isinf(r["costs"][0]), np.isinf(ref))
    np.testing.assert_allclose(r["costs"][0][~np.isinf(ref)], ref[~np.isinf(ref)], rtol=1e-10)
    np.testing.assert_array_equal(r["paths"][0], g["t2_path"])
    assert np.isinf(r["end_cost"][0][0])
    for res in (r, r0):
        assert res["best_end"][0] == 0 and res["best_end"][1] == -1
    assert r["paths"][1].shape[0] == 0
    for res in (r2, r2p):                   # two copies of the word: equal end costs everywhere, the last listed end wins
        np.testing.assert_array_equal(res["best_end"], [1, -1, 1])
        assert res["end_cost"][2][0] == res["end_cost"][2][1]
    assert np.all(r2p["paths"][2][:, 0] >= 5)
    b.close(); lat.close(); lat2.close(); gmm.close()


def test_headline_graph_takes_the_lane_form(hip, ctx, capfd):
    """bench.py's stacked word models (10 chains of 5 states): the lane form, its own end selection, same results as the
    back-pointer instantiation and -- GMMHMM_CHAIN is read at every call -- as the row form."""
    import bench
    from test_gpu_seq import forced
    wl = bench.synth_workload(3, 333)
    W, n, M, D = wl["W"], wl["n"], wl["M"], wl["D"]
    gmm = hip.PackedGMM(ctx, wl["means"].reshape(W * n, M, D), wl["vars"].reshape(W * n, M, D), wl["w"].reshape(W * n, M))
    b = hip.Batch(ctx, feats=wl["X"], offsets=wl["off"])
    b.loglik(gmm, fetch=False)
    lat = hip.Lattices(ctx, [bench.stacked_graph(W, n, wl["trans"])])
    with forced(GMMHMM_HOST_TRACE="1"):
        os.environ.pop("GMMHMM_CHAIN", None)
        capfd.readouterr()
        r = lat.viterbi(b, want_path=False)
        err = capfd.readouterr().err
        assert "chain=lanes" in err and "chain=rows" not in err, err
        rp = lat.viterbi(b, want_path=True)
        with forced(GMMHMM_CHAIN="rows"):
            capfd.readouterr()
            rr = lat.viterbi(b, want_path=False)
            err = capfd.readouterr().err
            assert "chain=rows" in err and "chain=lanes" not in err, err
    for other in (rp, rr):
        np.testing.assert_array_equal(r["end_cost_flat"].view(np.uint8), other["end_cost_flat"].view(np.uint8))
        np.testing.assert_array_equal(r["best_end"], other["best_end"])
    assert np.mean(r["best_end"] == wl["words"]) > 0.9
    b.close(); lat.close(); gmm.close()


if __name__ == "__main__":
    main(sys.argv[1])
