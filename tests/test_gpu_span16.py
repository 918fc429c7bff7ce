"""The env-per-16-lane-row step kernels (step_group.h, step_once SPAN) against the 8-lane-group kernels they replace
(RG_STEP_SPAN=0 at rg_create): free-running rollouts with auto-reset at the batch shapes that dispatch them, every output of
every step and the whole state at the end, word for word.  Plus the new instantiations' resources in the shipped library."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (scenario, overrides, action count, steps, envs): PCP 4096 x 5 (the benchmark), Warehouse 4096 x 8, MaterialTransport
# 2048 x 6 (two envs per wave), and a small batch (one env per wave)
SHAPES = [("PredatorCapturePrey", {"predator": 3, "capture": 2, "n_agents": 5}, 5, 300, 4096),
          ("Warehouse", {"n_agents": 8}, 5, 300, 4096),
          ("MaterialTransport", {"n_agents": 6, "n_fast_agents": 3, "n_slow_agents": 3, "start_dist": 0.25}, 20, 200, 2048),
          ("Simple", {"n_agents": 7}, 5, 200, 300)]


def _make(scenario, ov, E, span, monkeypatch):
    from marbler_amd import VecRobotariumEnv
    monkeypatch.setenv("RG_STEP_KERNEL", "group")
    if span:
        monkeypatch.delenv("RG_STEP_SPAN", raising=False)
    else:
        monkeypatch.setenv("RG_STEP_SPAN", "0")
    env = VecRobotariumEnv(scenario, E, overrides=ov, seed=7, auto_reset=True, collect_qp_stats=True)
    monkeypatch.delenv("RG_STEP_SPAN", raising=False)
    env.reset()
    return env


@pytest.mark.gpu
@pytest.mark.parametrize("scenario,ov,n_act,steps,E", SHAPES)
def test_span16_rows_match_eight_lane_groups_word_for_word(scenario, ov, n_act, steps, E, monkeypatch):
    import torch
    from gpu_helpers import ROW_STATE as STATE, differing
    new = _make(scenario, ov, E, True, monkeypatch)
    old = _make(scenario, ov, E, False, monkeypatch)
    assert new.step_kernel == old.step_kernel == "group"
    rng = np.random.RandomState(11)
    n_done = n_viol = n_sweeps = 0
    for t in range(steps):
        a = torch.as_tensor(rng.randint(0, n_act, size=(E, new.N)).astype(np.int32), device=new.device)
        new.step(a)
        old.step(a)
        bad = differing(new, old, ("obs", "reward", "done_u8", "dist_travelled", "violation", "remaining", "qp_sweeps"))
        assert not bad, f"{scenario} step {t}: {bad} differ"
        n_done += int(new.done_u8.sum())
        n_viol += int((new.violation != 0).sum())
        n_sweeps = max(n_sweeps, int(new.qp_sweeps.max()))
    bad = differing(new, old, STATE)
    assert not bad, f"{scenario}: state {bad} differs"
    # the rollouts went through resets, collisions (the pre-test fall-backs and the exact replay) and multi-sweep QPs
    assert n_done > 0 and n_viol > 0 and n_sweeps > 2, (n_done, n_viol, n_sweeps)


def test_span16_instantiations_have_no_spill():
    """The 16-lane-row kernels of the shipped library (step_kernel<SCN, 8, false, NT, false, 16>): no spilled
    VGPR, scratch <= 128 bytes, at least three waves per SIMD like the 8-lane-group kernels they stand in for."""
    from marbler_amd import build as hip_build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_scan
    if not os.path.exists(hip_build.LIB):
        pytest.skip("librobogym_hip.so is not built")
    try:
        res = {k: r["resources"] for k, r in isa_scan.scan_library(hip_build.LIB).items()}
    except RuntimeError as exc:
        pytest.skip(str(exc))
    hits = {k: r for k, r in res.items() if "2rg11step_kernelILi" in k and "ELb0ELi16ET" in k}
    assert len(hits) == 16, sorted(hits)   # 4 scenarios x N = 5..8
    for k, r in hits.items():
        assert r["spill"] == 0 and r["scratch"] <= 128 and r["occupancy"] >= 3, (k, r)
