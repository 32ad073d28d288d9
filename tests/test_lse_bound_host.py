# -*- coding: utf-8 -*-
"""The CPU model of the likelihood kernel's two fp64 log-sum-exp epilogues (tools/lse_bound_model.py), on
small shapes.  No GPU.

The bound form (reference point = the state's largest log normaliser, fixed when the model is packed) is taken only
where its sum clears the guard's threshold.  The model rounds the terms to fp64 -- where they underflow is the one thing
the reference point changes -- and the test asserts, over random models and the corners the GPU tests use (frames far
from every mean, variances of 1e-4, zero weights, a state without components), in both compat modes:

* a result -- the bound form where accepted, the fp64 redo elsewhere -- is within 1e-12 relative of the exact (long
  double) log-sum-exp;
* +inf (the reference's linear-domain underflow rule, switched-off states) and NaN (NaN constants) come out exactly
  where the exact form has them;
* the corners do reach the redo (the guard is exercised), the bench workload never does."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("lse_bound_model", os.path.join(ROOT, "tools", "lse_bound_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("compat", [True, False])
def test_guard_on_the_edge_models(tool, compat):
    redo = {}
    for name, X, means, vars_, w in tool.edge_models():
        res = tool.evaluate(X, means, vars_, w, compat)
        worst, wrong_inf, cold_cells, _ = tool.check(res, compat)
        assert worst <= 1e-12, (name, worst)
        assert wrong_inf == 0, name
        redo[name.split(" S")[0]] = max(redo.get(name.split(" S")[0], 0.0), cold_cells)
        if name.startswith("nan constants"):     # NaN only with every padded slot NaN; one NaN component poisons its state
            M = means.shape[1]
            first = res["result"][:, 0]
            assert (np.isnan(first) if tool.m_pad_of(M) == M else np.isposinf(first)).all(), name
            assert np.isnan(res["result"][:, 1]).all() and np.isposinf(res["result"][:, -1]).all(), name
        if name.startswith("zero weights"):      # state 0 has no component: always redone, +inf
            assert res["cold"][:, 0].all() and np.isinf(res["exact"][:, 0]).all()
    assert redo["random"] == 0.0
    assert redo["far frames"] > 0.5 and redo["variance 1e-4"] > 0.4 and redo["zero weights"] > 0.0


def test_threshold_carries_the_mixture_size_in_compat_mode(tool):
    """s <= M_pad 2^(max y / 128): a state whose bound is far below 0 needs s above 2 M_pad 2^(-1075 - mh / ln 2)"""
    mh = np.array([-400.0, 0.0, 50.0], dtype=tool.LD)
    on = np.array([True, True, True])
    t8, t32 = tool.thresholds(mh, on, 8, True), tool.thresholds(mh, on, 32, True)
    assert t8[1] == t8[2] == 2.0 ** -900 and t32[1] == 2.0 ** -900
    want = 16.0 * 2.0 ** (-1075 + 400 / np.log(2.0))
    assert abs(t8[0] / want - 1) < 1e-9 and abs(t32[0] / t8[0] - 4) < 1e-12
    assert (tool.thresholds(mh, on, 8, False) == 2.0 ** -900).all()
    assert np.isinf(tool.thresholds(mh, np.array([False, True, True]), 8, True)[0])


def test_bench_workload_never_takes_the_redo(tool):
    sys.path.insert(0, ROOT)
    import bench
    wl = bench.synth_workload(1002, 200)
    S = wl["W"] * wl["n"]
    means, vars_, w = (wl[k].reshape((S, wl["M"]) + wl[k].shape[3:]) for k in ("means", "vars", "w"))
    rng = np.random.default_rng(0)
    X = wl["X"][rng.choice(len(wl["X"]), size=384, replace=False)]
    for compat in (True, False):
        res = tool.evaluate(X, means, vars_, w, compat)
        worst, wrong_inf, cold_cells, cold_blocks = tool.check(res, compat)
        assert cold_cells == 0.0 and cold_blocks == 0.0
        assert worst <= 1e-12 and wrong_inf == 0
        gap = (res["mh"][None] - res["amax"]).astype(np.float64)
        assert gap.max() < 400.0          # (the guard sits ~620 nats below the bound)
