"""bench.py's two kinds of run on the GPU: a plain run (`--gpus 1 --steps K --warmup W`) times the headline and nothing else;
`--full` adds what is measured beside it (per-launch event pairs, side legs; the CPU baseline and the live counter passes are
left out here with --no-cpu-baseline)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_LEGS = ("cpu_baseline", "graph_replay", "rollout", "host_boundary", "saturated", "actor", "interior_point_mode", "saturated_2m")
PROBE_KEYS = ("kernel_ms_avg_event_pair_per_launch", "kernel_ms_median_event_pair_per_launch")


def _bench(*argv):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_the_headline_only(tmp_path):
    d = _bench("--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", str(tmp_path))
    assert (d["metric"], d["unit"], d["higher_is_better"], d["dtype"]) == ("env agent-steps/sec", "agent-steps/s", True, "f32")
    assert d["steps"] == 20 and d["warmup"] == 5 and d["full"] is False and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(4096 * 5 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    assert not [k for k in SIDE_LEGS if k in d]
    assert not [k for k in PROBE_KEYS if k in d["roofline"]] and d["roofline"]["kernel_ms_avg"] > 0
    assert d["roofline"]["traffic_kind"].startswith("from_committed_profile")     # no counter passes in a plain run
    obs = np.load(tmp_path / "obs.npy")
    assert obs.shape[0] == 4096 and obs.dtype == np.float32 and np.isfinite(obs).all()
    assert sorted(d["dump_outputs"]["arrays"]) == sorted(["obs", "reward", "done", "dist_travelled", "violation", "remaining"])


def test_full_run_adds_the_side_measurements():
    d = _bench("--gpus", "1", "--steps", "100", "--warmup", "10", "--full", "--no-cpu-baseline")
    assert d["full"] is True and d["value"] == pytest.approx(4096 * 5 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    assert all(d["roofline"][k] > 0 for k in PROBE_KEYS)
    assert [k for k in SIDE_LEGS if k in d] == list(SIDE_LEGS[1:])                   # every side leg but the skipped CPU baseline
    assert "error" not in d["graph_replay"] and d["saturated"]["envs"] == 524288 and d["saturated_2m"]["envs"] == 4 * 524288
    assert d["interior_point_mode"]["ms_per_step"] > 0 and d["actor"]["ms_per_launch"] > 0 and d["rollout"]["ms_per_step"] > 0
