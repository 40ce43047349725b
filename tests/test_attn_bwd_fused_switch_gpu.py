"""KLAB_T5_ATTN_BWD_FUSED=0 (o / co projection dgrad GEMM + attention backward as two launches) selects another form of the same
arithmetic as the default fused launch: the bench workload's loss after a few optimizer steps (BASELINE configs[1], fixed seeds,
dropout on) agrees within bf16 rounding.  One `bench.py` child process per setting (the switch is read once per process)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _final_loss(extra_env):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KLAB_T5_ATTN_BWD_FUSED")}
    env.update(extra_env)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])["config"]["final_loss"]


def test_attn_bwd_fused_switch_keeps_the_loss():
    fused, two = _final_loss({}), _final_loss({"KLAB_T5_ATTN_BWD_FUSED": "0"})
    assert abs(fused - two) <= 5e-3 * abs(two), (fused, two)
