# -*- coding: utf-8 -*-
"""The sharded EM iteration (HIP E-step per rank + ONE all-reduce of the packed statistics) gives the same model as
the single-process iteration.  With two or more GPUs visible the ranks take one GPU each and the collective is RCCL
("nccl") on the device-resident buffer; on a one-GPU box two ranks share GPU 0 over gloo, and a ONE-rank RCCL group
still drives the device-buffer path (gh_bw_accumulate(stats_dev) -> dist.all_reduce on that tensor).  `bench.py
--gpus 2` is run as ONE command, the way the driver starts it."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _problem():
    g = load_golden("G11_continuous_train")
    W, U = int(g["n_words"]), int(g["n_utts"])
    data = [g["x%d" % i] for i in range(U)]
    labels = [list(g["labels%d" % i]) for i in range(U)]
    means = np.array([g["init%d_means" % wi] for wi in range(W)])
    vars_ = np.array([g["init%d_vars" % wi] for wi in range(W)])
    w = np.array([g["init%d_w" % wi] for wi in range(W)])
    trans = [g["init%d_transitions" % wi] for wi in range(W)]
    return means, vars_, w, trans, data, labels


def _n_gpus():
    from sr.recognition import _hip
    return _hip.device_count()


def _worker(rank, world, port, out_dir, backend):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), os.path.join(os.path.dirname(here), "speech-recognition_amd"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = rank if backend == "nccl" else 0     # gloo: both ranks on the single GPU of the box
    os.environ["GMMHMM_DEVICE"] = str(dev)
    if backend == "nccl":
        import torch
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sr.recognition.train import BaumWelchTrainer
        from sr.recognition.parallel import shard_utterances, StatsAllReducer
        means, vars_, w, trans, data, labels = _problem()
        mine = shard_utterances([len(x) for x in data], world)[rank]
        tr = BaumWelchTrainer(means, vars_, w, trans, [data[i] for i in mine], [labels[i] for i in mine],
                              device=dev, reducer=StatsAllReducer(gpu_index=dev), var_floor=1e-3)
        assert tr.reducer.on_gpu == (backend == "nccl")
        hist = tr.fit(2)
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), means=tr.means, vars=tr.vars, w=tr.weights,
                 hist=np.array(hist), mine=mine, collectives=tr.reducer.calls)
        tr.close()
    finally:
        dist.destroy_process_group()


def test_sharded_em_equals_single_process(tmp_path):
    import torch.multiprocessing as mp
    from sr.recognition.train import BaumWelchTrainer
    backend = "nccl" if _n_gpus() >= 2 else "gloo"    # RCCL whenever the box has a GPU per rank
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), backend), nprocs=2, join=True)
    means, vars_, w, trans, data, labels = _problem()
    tr = BaumWelchTrainer(means, vars_, w, trans, data, labels, var_floor=1e-3)
    hist = tr.fit(2)
    r0, r1 = np.load(tmp_path / "rank0.npz"), np.load(tmp_path / "rank1.npz")
    assert sorted(np.concatenate([r0["mine"], r1["mine"]]).tolist()) == list(range(len(data)))
    for r in (r0, r1):
        assert int(r["collectives"]) == 2                      # ONE collective per EM iteration
        np.testing.assert_allclose(r["hist"], hist, rtol=1e-10)
        np.testing.assert_allclose(r["means"], tr.means, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(r["vars"], tr.vars, rtol=1e-7)
        np.testing.assert_allclose(r["w"], tr.weights, rtol=1e-8, atol=1e-12)
    tr.close()


def _one_rank_rccl(rank, port, out_dir):
    """A ONE-rank RCCL group: the device-buffer path of the trainer on whatever single GPU is there."""
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), os.path.join(os.path.dirname(here), "speech-recognition_amd"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        from sr.recognition.train import BaumWelchTrainer
        from sr.recognition.parallel import StatsAllReducer
        means, vars_, w, trans, data, labels = _problem()
        red = StatsAllReducer(gpu_index=0)
        assert red.enabled and red.on_gpu and dist.get_backend() == "nccl"
        tr = BaumWelchTrainer(means, vars_, w, trans, data, labels, device=0, reducer=red, var_floor=1e-3,
                              device_resident=False)       # the torch-tensor path (the native one: test_gpu_em_session.py)
        hist = tr.fit(2)
        np.savez(os.path.join(out_dir, "rccl1.npz"), means=tr.means, vars=tr.vars, w=tr.weights, hist=np.array(hist),
                 collectives=red.calls)
        tr.close()
    finally:
        dist.destroy_process_group()


def test_rccl_allreduce_on_the_device_resident_statistics(tmp_path):
    """gh_bw_accumulate writes into a torch tensor in HBM, RCCL ("nccl") all-reduces THAT tensor, the M-step reads
    the reduced copy: same model as the trainer without a process group (host-buffer path)."""
    import torch.multiprocessing as mp
    from sr.recognition.train import BaumWelchTrainer
    mp.spawn(_one_rank_rccl, args=(_free_port(), str(tmp_path)), nprocs=1, join=True)
    means, vars_, w, trans, data, labels = _problem()
    tr = BaumWelchTrainer(means, vars_, w, trans, data, labels, var_floor=1e-3)
    hist = tr.fit(2)
    r = np.load(tmp_path / "rccl1.npz")
    assert int(r["collectives"]) == 2
    np.testing.assert_allclose(r["hist"], hist, rtol=1e-12)
    np.testing.assert_allclose(r["means"], tr.means, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(r["vars"], tr.vars, rtol=1e-12)
    np.testing.assert_allclose(r["w"], tr.weights, rtol=1e-12, atol=1e-14)
    tr.close()


def _run_bench(extra, extras=False):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--ramp-seconds", "0.1",
           "--utts", "400", "--em-utts", "300", "--em-iters", "2", "--no-cpu-baseline", "--full"] + extra
    cmd += ["--c5-utts", "1000", "--c4-utts", "60", "--c4-em-utts", "40", "--c3-utts", "50"] if extras else ["--no-extra-configs"]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]                   # ONE JSON line, from rank 0
    return json.loads(lines[0])


def test_bench_gpus_2_is_one_command():
    """`python bench.py --gpus 2` without a launcher starts its own two ranks, which talk through the
    library's own RCCL communicator (two GPUs: xGMI; a one-GPU box: both ranks on GPU 0, socket transport), and the
    N-rank line carries every 8-GPU config of BASELINE.json: configs[4] (C5, K-layer lattice and loop grammar) and
    configs[3] (C4) with `n_gpus` and all ranks' utterances."""
    two = _n_gpus() >= 2
    out = _run_bench(["--gpus", "2"] + ([] if two else ["--same-gpu"]), extras=True)
    assert out["n_gpus"] == 2 and out["config"]["parallelism"].endswith("x2") and out["config"]["process_group"] == "native"
    assert out["decode_accuracy"] == 1.0
    em = out["em"]
    assert em["backend"] == "nccl" and em["comm"] == "native" and em["rccl_ranks"] == 2       # ncclCommCount
    assert em["device_resident_iteration"] and em["host_syncs_per_iteration"] == 1
    assert em["loglik_monotone"] and em["em_utterances_per_s"] > 0 and em["allreduce_ms"] > 0
    cfg = out["configs"]
    for key in ("C5_K7_lattice", "C5_loop_grammar"):
        assert cfg[key]["n_gpus"] == 2 and cfg[key]["utterances"] == 2000 and cfg[key]["value"] > 0, cfg[key]
        assert cfg[key]["sequence_accuracy_sampled"] == 1.0
        assert 0.0 <= cfg[key]["fp32_path_mismatch_rate"] <= 0.05 and cfg[key]["fp32_label_mismatch_rate"] <= 0.01
    assert cfg["C4"]["n_gpus"] == 2 and cfg["C4"]["utterances"] == 120
    # (the configs[3]-shape EM runs on the device-resident session too: its 20.7 MB buffer crosses the two ranks on the stream)
    assert cfg["C4_em"]["n_gpus"] == 2 and cfg["C4_em"]["loglik_monotone"] and cfg["C4_em"]["device_resident_iteration"]
    assert cfg["C4_em"]["utterances"] == 80 and cfg["C4_em"]["allreduce_bytes"] == (1024 * 32 * 79 + 1024 + 2) * 8


def test_bench_gpus_2_strong_scaling_em_and_gloo_rehearsal():
    """--em-total: configs[2]'s utterances drawn once and sharded over the ranks by frames (strong scaling); run here
    through the torch.distributed / gloo form with both ranks on GPU 0."""
    out = _run_bench(["--gpus", "2", "--backend", "gloo", "--device", "0", "--em-total", "500"])
    assert out["n_gpus"] == 2 and out["config"]["process_group"] == "torch"
    em = out["em"]
    assert em["scaling"] == "strong" and em["backend"] == "gloo" and em["rccl_ranks"] == 0
    assert not em["device_resident_iteration"] and em["loglik_monotone"]
    assert abs(em["em_utterances_per_s"] * em["ms_per_iteration"] * 1e-3 - 500) < 1e-6


def test_bench_single_gpu_runs_the_collective_on_rccl():
    out = _run_bench(["--gpus", "1"], extras=True)
    assert out["n_gpus"] == 1
    em = out["em"]
    assert "rccl_error" not in em, em
    assert em["backend"] == "nccl" and em["rccl_ranks"] == 1 and em["allreduce_on_device_buffer"]
    assert em["device_resident_iteration"] and em["loglik_monotone"]
    cfg = out["configs"]
    assert not any("error" in v for v in cfg.values() if isinstance(v, dict)), cfg
    assert cfg["C2_fp32_decode"]["fp32_word_mismatch_rate"] == 0.0
    assert cfg["C5_loop_grammar"]["n_gpus"] == 1


def test_bench_under_the_drivers_launcher():
    """The driver starts an N-rank bench as `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`:
    the launcher only provides the environment (RANK / WORLD_SIZE / MASTER_*), the ranks use the library's own RCCL
    communicator -- the unique id travels over MASTER_PORT + 1, next to the launcher's store on MASTER_PORT."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    two = _n_gpus() >= 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--ramp-seconds", "0.1", "--utts", "400", "--em-utts", "300", "--em-iters", "2", "--no-cpu-baseline", "--no-extra-configs",
           "--full"]
    if not two:
        cmd.append("--same-gpu")
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["process_group"] == "native" and out["em"]["rccl_ranks"] == 2
    assert out["decode_accuracy"] == 1.0 and out["em"]["loglik_monotone"]
