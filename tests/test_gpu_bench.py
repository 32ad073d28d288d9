# -*- coding: utf-8 -*-
"""A plain `bench.py` run: the headline alone (no CPU baselines, EM leg, other configs or PCIe step; those need
--full), `--steps` timed steps, and with `--dump-outputs DIR` the outputs of its last step, the same from run to run
and equal to the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_bench(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--ramp-seconds", "0.1", "--utts", "400", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_times_the_headline_and_dumps_its_outputs(tmp_path):
    import bench
    from oracle import ref_numpy as O
    out = _plain_bench(tmp_path / "a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out, key
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["dtype"] == "f64" and out["decode_accuracy"] == 1.0
    assert not {"cpu_baseline", "em", "configs", "pcie_inclusive"} & set(out)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["decoded_word.npy", "end_cost.npy", "loglik_sample.npy", "loglik_sample_frames.npy"]
    d = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    # the outputs are those of the workload bench.py draws (seed 1002) ...
    wl = bench.synth_workload(1002, 400)
    W, n, M, D = wl["W"], wl["n"], wl["M"], wl["D"]
    S = W * n
    assert d["end_cost"].shape == (400, W)
    np.testing.assert_array_equal(d["decoded_word"], np.argmin(d["end_cost"], axis=1))
    np.testing.assert_array_equal(d["decoded_word"], wl["words"])
    frames = d["loglik_sample_frames"].astype(np.int64)
    ref = O.gmm_neg_loglik_batch(wl["X"][frames], wl["means"].reshape(S, M, D), wl["vars"].reshape(S, M, D),
                                 wl["w"].reshape(S, M))
    np.testing.assert_allclose(d["loglik_sample"], ref, rtol=1e-10)
    nes = np.zeros(n, dtype=bool)
    for u in (0, 199, 399):
        x = wl["X"][wl["off"][u]:wl["off"][u + 1]]
        nll = O.gmm_neg_loglik_batch(x, wl["means"].reshape(S, M, D), wl["vars"].reshape(S, M, D), wl["w"].reshape(S, M))
        for i in range(W):
            costs, _ = O.decode_states(nll[:, i * n:(i + 1) * n].T, nes, wl["trans"])
            np.testing.assert_allclose(d["end_cost"][u, i], costs[-1, -1], rtol=1e-10)
    # ... and a second run with the same arguments writes the same files
    _plain_bench(tmp_path / "b")
    for name in names:
        np.testing.assert_array_equal(np.load(tmp_path / "b" / name), d[name[:-4]])
