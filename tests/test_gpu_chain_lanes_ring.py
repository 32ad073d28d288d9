# -*- coding: utf-8 -*-
"""The "beside" form of the lane = chain Viterbi -- viterbi_chain_lanes_kernel with its shallow prefetch ring of LANE_PF
columns and its strided grid (csrc/gh_viterbi_chain.hip; the launcher takes it by itself only for batches of about a
wave per SIMD, GMMHMM_CHAIN_FORM=beside forces it for the small batches here) -- against the lane = row form
(viterbi_chain_kernel, GMMHMM_CHAIN=rows in a fresh child process).

Everything is compared BIT FOR BIT (raw bytes): end costs, best ends, paths.  The lane form changes no arithmetic, so
there is no tolerance to choose.  The graph is the headline's shape, 10 chains x 5 rows (6 utterances per wave); fp64 and
fp32 emissions; with and without paths.  The lengths bracket the ring depth P: T in {1, 2, P, P+1, 2P, 2P+1, 2P+2,
3P+3} -- the loop without guards starts at 1 + 2P columns, the guarded loop takes whatever is left --
  * every utterance of a batch the same length, U in {1, 6, 7, 13}: a single utterance, a full wave, a full wave and a
    single one, two full waves and a single one;
  * all lengths mixed inside one wave (U = 6: tmin < 1 + 2P <= tmax, the wave leaves the loop without guards while some
    lanes have ended and others go on), and U = 7 / 13 of mixed lengths; a batch that holds a one-frame utterance
    leaves the chain kernels altogether (gh_decode.hip, any_T1), so these start at 2 frames and one more mixed batch
    carries T = 1 through whatever kernel takes it;
  * clean emissions, and emissions with +inf and NaN in the first, the last and the ring-boundary columns.
The strided grid (GMMHMM_CHAIN_WAVES=n, read at every call: n waves walk all positions of the one-wave-per-6-utterances
grid): 43 utterances are 8 positions, 2 waves walk 4 each; the outputs equal those of the plain grid and of the row form.

Run as a script (`python tests/test_gpu_chain_lanes_ring.py OUT.npz`) the file computes every case with the kernel the
environment selects and stores the results: that is the child process of the comparison."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "speech-recognition_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)

P = 2                     # LANE_PF, the shallow ring's depth (test_ring_depth_is_the_one_tested reads it from the source)
LENGTHS = (1, 2, P, P + 1, 2 * P, 2 * P + 1, 2 * P + 2, 3 * P + 3)
N_ROWS, CHAINS = 5, 10
EQUAL_U = (1, 6, 7, 13)
# (a batch that holds an utterance of ONE frame leaves the chain kernels altogether -- gh_decode.hip: any_T1 -- so T = 1
# is compared through whatever kernel takes it, and the mixed batches that have to reach the lane form start at 2)
LANE_LENGTHS = tuple(t for t in LENGTHS if t > 1)
MIXED = {"mixed6a": (2, 2 * P + 2, P + 1, 3 * P + 3, 2, 2 * P + 1), "mixed6b": (P + 1, 2 * P, 2, 3 * P + 3, 2 * P + 1, 2 * P + 2),
         "mixed6_with_T1": (1, 2 * P + 2, P, 3 * P + 3, 2, 2 * P + 1),
         "mixed7": tuple(LANE_LENGTHS[(3 * k) % len(LANE_LENGTHS)] for k in range(7)),
         "mixed13": tuple(LANE_LENGTHS[(5 * k) % len(LANE_LENGTHS)] for k in range(13))}
STRIDED_U, STRIDED_WAVES = 43, 2
DTYPES = {"f64": np.float64, "f32": np.float32}


def batches():
    """name -> lengths"""
    out = {}
    for T in sorted(set(LENGTHS)):
        for U in EQUAL_U:
            out["equal_T%d_U%d" % (T, U)] = (T,) * U
    out.update(MIXED)
    out["strided"] = tuple(LANE_LENGTHS[(3 * k + 1) % len(LANE_LENGTHS)] for k in range(STRIDED_U))
    return out


def mark_columns(nll, offsets, rng):
    """+inf and NaN into the first, the last and the ring-boundary columns of every utterance (a few states each)"""
    S = nll.shape[1]
    for u in range(len(offsets) - 1):
        T = int(offsets[u + 1] - offsets[u])
        for t in sorted({0, T - 1, P - 1, P, P + 1, 2 * P, 2 * P + 1, 2 * P + 2} & set(range(T))):
            cols = rng.choice(S, size=6, replace=False)
            nll[offsets[u] + t, cols[:4]] = np.inf
            nll[offsets[u] + t, cols[4:]] = np.nan
    return nll


def run_dtype(hip, ctx, dt, strided_knob=None):
    """Every batch of one dtype: {key: bytes}; the batch "strided" runs under GMMHMM_CHAIN_WAVES=strided_knob when given."""
    from test_gpu_bigram import forced
    from test_gpu_chain_lanes import chain_graph, decode, write_emissions
    rng = np.random.default_rng(77 + (dt == "f32"))
    n_blocks, M, D = 10, 2, 4
    S = n_blocks * N_ROWS
    gmm = hip.PackedGMM(ctx, rng.normal(size=(S, M, D)), rng.uniform(0.5, 1.5, size=(S, M, D)), rng.dirichlet(np.ones(M), size=S))
    lat = hip.Lattices(ctx, [chain_graph(rng, N_ROWS, CHAINS, False, False, n_blocks)])
    assert "chain" in lat.forms()
    out = {}
    for name, lengths in batches().items():
        xs = [rng.normal(size=(t, D)) for t in lengths]
        for variant in ("clean", "marked"):
            b = hip.Batch(ctx, xs, dtype=DTYPES[dt])
            nll = b.loglik(gmm)
            if variant == "marked":
                write_emissions(hip, ctx, b, mark_columns(nll, b.offsets, rng))
            env = {"GMMHMM_CHAIN_WAVES": strided_knob} if (name == "strided" and strided_knob) else {}
            with forced(**env):
                for call, kw in (("ends", dict(want_path=False)), ("path", dict(want_path=True))):
                    for k, v in decode(lat, b, **kw).items():
                        out["%s/%s/%s/%s" % (name, variant, call, k)] = v
            b.close()
    lat.close(); gmm.close()
    return out


def main(out_path):
    from sr.recognition import _hip as hip
    ctx = hip.default_context()
    res = {}
    for dt in DTYPES:
        for k, v in run_dtype(hip, ctx, dt).items():
            res[dt + "/" + k] = v
    np.savez(out_path, **res)


# ------------------------------------------------------------------------------------------------------- the tests
def test_ring_depth_is_the_one_tested():
    """(no GPU) the lengths above bracket the depth the source has"""
    src = open(os.path.join(ROOT, "speech-recognition_amd", "csrc", "gh_viterbi_chain.hip")).read()
    assert int(re.search(r"#define GH_VL_PF (\d+)", src).group(1)) == P


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
    out = str(tmp_path_factory.mktemp("chain_ring_rows") / "rows.npz")
    env = dict(os.environ, GMMHMM_CHAIN="rows", GMMHMM_HOST_TRACE="1")
    env.pop("GMMHMM_CHAIN_WAVES", None)
    env.pop("GMMHMM_CHAIN_FORM", None)
    flags = ["-s"] if sys.flags.no_user_site else []
    p = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__), out], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "chain=rows" in p.stderr and "chain=lanes" not in p.stderr, "the child did not stay on the lane = row kernel"
    return np.load(out)


def _same(got, rows_results, dt):
    prefix = dt + "/"
    want = {k[len(prefix):]: rows_results[k] for k in rows_results.files if k.startswith(prefix)}
    assert sorted(want) == sorted(got)
    for k in sorted(got):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert sum(k.endswith("/path/paths") for k in got) >= len(batches())     # the clean batches always give paths


@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(DTYPES))
def test_lane_form_equals_row_form_around_the_ring_depth(hip, ctx, rows_results, capfd, dt):
    from test_gpu_bigram import forced
    with forced(GMMHMM_HOST_TRACE="1", GMMHMM_CHAIN_FORM="beside"):
        os.environ.pop("GMMHMM_CHAIN", None)
        os.environ.pop("GMMHMM_CHAIN_WAVES", None)
        got = run_dtype(hip, ctx, dt)
    err = capfd.readouterr().err
    assert "chain=lanes" in err and "chain=rows" not in err, "a case left the lane form"
    assert "] beside grid" in err and "] alone grid" not in err, "a case left the shallow ring"
    _same(got, rows_results, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(DTYPES))
def test_strided_grid_equals_plain_grid_and_row_form(hip, ctx, rows_results, capfd, dt):
    """2 waves walk the 8 positions of 43 utterances; every other batch of the run has fewer positions than 3 per wave."""
    from test_gpu_bigram import forced
    with forced(GMMHMM_HOST_TRACE="1", GMMHMM_CHAIN_FORM="beside"):
        os.environ.pop("GMMHMM_CHAIN", None)
        os.environ.pop("GMMHMM_CHAIN_WAVES", None)
        got = run_dtype(hip, ctx, dt, strided_knob=str(STRIDED_WAVES))
    err = capfd.readouterr().err
    assert "chain=lanes" in err and "chain=rows" not in err, "a case left the lane form"
    grids = sorted(set(l for l in err.splitlines() if "chain lanes]" in l))
    walked = [int(m.group(1)) for l in grids for m in [re.search(r"beside grid %d of (\d+) positions" % STRIDED_WAVES, l)] if m]
    assert walked and max(walked) >= 3 * STRIDED_WAVES, grids          # a wave walks at least 3 positions
    assert not any("] alone grid" in l for l in grids), grids
    _same(got, rows_results, dt)


@pytest.mark.gpu
def test_launch_form_follows_the_batch_size(hip, ctx, capfd):
    """Left to itself the launcher takes the "beside" form from half a wave to two waves per SIMD (1 024 SIMDs on an
    MI355X: 513 .. 2 048 grid positions of 6 utterances) and caps its grid at one wave per SIMD; smaller and larger
    batches keep the ring of 8 columns and one wave per position.  Same results either way."""
    from test_gpu_bigram import forced
    from test_gpu_chain_lanes import chain_graph, decode
    rng = np.random.default_rng(5)
    n_blocks, M, D = 10, 2, 4
    S = n_blocks * N_ROWS
    gmm = hip.PackedGMM(ctx, rng.normal(size=(S, M, D)), rng.uniform(0.5, 1.5, size=(S, M, D)), rng.dirichlet(np.ones(M), size=S))
    lat = hip.Lattices(ctx, [chain_graph(rng, N_ROWS, CHAINS, False, False, n_blocks)])
    for U, want in ((60, "alone grid 10 of 10"), (6 * 600, "beside grid 600 of 600"), (6 * 1500, "beside grid 1024 of 1500"),
                    (6 * 2100, "alone grid 2100 of 2100")):
        T = rng.integers(2, 8, size=U)          # (a one-frame utterance takes the whole batch off the chain kernels)
        off = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
        b = hip.Batch(ctx, feats=rng.normal(size=(int(off[-1]), D)), offsets=off)
        b.loglik(gmm, fetch=False)
        with forced(GMMHMM_HOST_TRACE="1"):
            for k in ("GMMHMM_CHAIN", "GMMHMM_CHAIN_WAVES", "GMMHMM_CHAIN_FORM"):
                os.environ.pop(k, None)
            capfd.readouterr()
            got = decode(lat, b, want_path=False)
            err = capfd.readouterr().err
            assert "] " + want + " positions" in err, (U, err)
            with forced(GMMHMM_CHAIN_FORM="alone" if want.startswith("beside") else "beside"):
                other = decode(lat, b, want_path=False)
        assert sorted(got) == sorted(other)
        for k in got:
            assert np.array_equal(got[k], other[k]), (U, k)
        b.close()
    lat.close(); gmm.close()


if __name__ == "__main__":
    main(sys.argv[1])
