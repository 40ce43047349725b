"""bench.py's N > 1 code path on real hardware with what a one-GPU box allows: two ranks pinned to card 0, the collectives through
gloo (RCCL refuses two ranks on one device).  Everything but the transport is the production path: torch.distributed.run launch,
RANK / WORLD_SIZE handling, klab DistributedDataParallel with per-layer buckets and overlap_optimizer, FusedAdam, the barrier /
max-over-ranks timing and the single JSON line on rank 0."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bench_two_ranks_on_one_card_reduce_and_stay_in_sync():
    env = dict(os.environ, KLAB_BENCH_DEVICE="0", KLAB_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--full", "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines  # ONE JSON line, from rank 0
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "weak" and d["config"]["global_batch"] == 128
    rc = d["config"]["rccl"]
    assert rc["ranks"] == 2 and rc["replicas_in_sync_after_run"] is True
    # every trainable T5 gradient crosses the wire once per step: 60.5 M fp32 values
    assert rc["allreduce_bytes_per_step"] == 242026496 and rc["allreduce_calls_per_step"] >= 4
    assert d["value"] > 0 and abs(d["value"] - 2 * 64 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-2 * d["value"]


def test_bench_gpus2_without_a_launcher_starts_its_own_ranks():
    """`python bench.py --gpus 2` with no WORLD_SIZE in the environment (the shape of the driver's one-GPU command): bench.py starts
    the two ranks itself as a child torchrun (ref/run_scripts/caption/train_with_swin.sh:1) and relays ONE line with n_gpus == 2."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(KLAB_BENCH_DEVICE="0", KLAB_BENCH_BACKEND="gloo")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full",
           "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["rccl"]["ranks"] == 2 and d["config"]["rccl"]["replicas_in_sync_after_run"] is True
    assert len(d["config"]["rank_ms_per_step"]["per_rank"]) == 2 and "roofline" in d


def _bench_one_gpu(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_bench_dump_outputs_hold_the_last_timed_step(tmp_path):
    """--dump-outputs writes the last timed step's loss, updated weights and Adam moments (float arrays, <= 64 MB).  That step
    starts from the seeded initial state, so the arrays must satisfy Adam's first update exactly against the model's initial
    weights; a plain run carries no --full figures, and a --full run with the same arguments dumps the same outputs."""
    import types

    import numpy as np
    import torch

    import bench
    from klab_multimodalmodel_amd.models.model import MyModel
    plain, full = tmp_path / "plain", tmp_path / "full"
    d = _bench_one_gpu("--dump-outputs", str(plain))
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and "roofline" not in d and "cpu_baseline" not in d
    f = _bench_one_gpu("--dump-outputs", str(full), "--full", "--no-cpu-baseline")
    assert "roofline" in f
    names = sorted(p.name for p in plain.iterdir())
    assert names == ["adam_exp_avg_sample.npy", "adam_exp_avg_sq_sample.npy", "loss.npy", "transformer_param_sample.npy"]
    assert sum((plain / n).stat().st_size for n in names) <= 64 << 20
    a = {n: np.load(plain / n) for n in names}
    b = {n: np.load(full / n) for n in names}
    assert all(x.dtype in (np.float32, np.float64) and np.isfinite(x).all() for x in a.values())
    assert abs(float(a["loss.npy"][0]) - d["config"]["final_loss"]) < 1e-3 * d["config"]["final_loss"]

    # Adam's first step (lr 1e-3, betas (0.9, 0.999), eps 1e-8) from the seeded initial weights, read off the dumped arrays
    sw, t5 = bench.workload_configs("caption")
    args = types.SimpleNamespace(result_dir=str(tmp_path), language_model_name="-", image_model_name="-", image_model_train=False,
                                 transformer_model_name="-")
    torch.manual_seed(0)  # as bench.py does before it builds the model
    w0 = torch.cat([p.detach().reshape(-1).float() for p in MyModel(args, _configs=(sw, t5, t5), _seed=0, dtype="bf16").transformer.parameters()])
    idx = torch.randint(0, w0.numel(), (bench.DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
    w0 = w0[idx].double().numpy()
    m, v, w = (a[n].astype(np.float64) for n in ("adam_exp_avg_sample.npy", "adam_exp_avg_sq_sample.npy", "transformer_param_sample.npy"))
    g = m / 0.1
    assert np.abs(g).max() > 0 and np.allclose(v, 0.001 * g * g, rtol=1e-4, atol=1e-30)  # exp_avg_sq = (1 - beta2) g^2
    assert np.allclose(w, w0 - 1e-3 * g / (np.sqrt(v / 0.001) + 1e-8), rtol=0, atol=2e-6)
    assert np.mean(np.abs(w - w0) > 0.9e-3) > 0.5  # most sampled weights moved by ~lr

    # same inputs and seeds in both runs: equal up to the order of the engine's atomic floating-point sums.  Measured on MI355X
    # (profiles/bench_dump_reproducibility.txt): loss bit-identical, moments rel-L2 2-3e-3 (bf16 roundings tipped by that order),
    # weights 7e-5 (+-lr where a gradient at rounding level changes sign); a wrong gradient scale or moment update moves them by ~1
    tol = {"loss.npy": 1e-5, "transformer_param_sample.npy": 1e-3, "adam_exp_avg_sample.npy": 1e-2, "adam_exp_avg_sq_sample.npy": 1e-2}
    for n in names:
        x, y = a[n].astype(np.float64), b[n].astype(np.float64)
        assert np.linalg.norm(x - y) <= tol[n] * np.linalg.norm(y), n
