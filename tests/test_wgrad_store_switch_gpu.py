"""KLAB_WGRAD_STORE=0 (both trainable segments of the gradient buffer cleared whole, every weight-gradient product accumulating)
selects another form of the same arithmetic as the default write plan (first writers store, only the rest is cleared): the bench
workload's loss after a few optimizer steps (BASELINE configs[1], fixed seeds, dropout on) agrees within bf16 rounding.  So does
KLAB_WGRAD_STORE=1 with KLAB_WGRAD_GROUP_TILES=0, the plan in which nothing is grouped and everything but the LM-head weight
gradient's slice must be cleared.  One `bench.py` child process per setting (the switches are read once per process)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _final_loss(extra_env):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KLAB_WGRAD_STORE", "KLAB_WGRAD_GROUP_TILES")}
    env.update(extra_env)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])["config"]["final_loss"]


@pytest.fixture(scope="module")
def default_loss():
    return _final_loss({})


@pytest.mark.parametrize("sw", [{"KLAB_WGRAD_STORE": "0"}, {"KLAB_WGRAD_STORE": "1", "KLAB_WGRAD_GROUP_TILES": "0"}],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_wgrad_store_switch_keeps_the_loss(default_loss, sw):
    loss = _final_loss(sw)
    assert abs(loss - default_loss) <= 5e-3 * abs(default_loss), (sw, loss, default_loss)
