"""BASELINE.json's batch shapes and every dispatch width of the lane-group kernel against the float32 oracle.

The lane-group launch picks the number of env slots a wavefront uses from the batch size (`wave_fill`,
csrc/launch_plan.h): at 8 lanes per env a batch of <= 1024 envs runs 1 env per wave, 2048 -> 2, 4096 -> 4 (the
headline: 1024 workgroups through the XCD-aware chunk map), >= 8192 -> 8; at 4 lanes per env the steps are 1 / 2 / 4 /
8 / 16.  The other oracle-checked rollouts (tests/test_gpu_rollout.py) stay below 1024 envs = one env per wave, so
these cases put the lane -> env map the driver's bench line times -- and the per-GPU shapes of configs[2] .. [4] --
under the same bar: free-running rollouts with auto-reset against the oracle stepping the same envs on the host with the
reset twin (what is compared: tests/oracle_check.py), through rg_step and through rg_rollout.

Reference rows: PredatorCapturePrey.py:138-176, warehouse.py:102-122, MaterialTransport.py:113-148.
"""
import pytest

from rollout_harness import MT6, PCP5, SHAPE_CASES as CASES, WH8, shape_rollout_vs_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,scenario,ov,n_act,E,steps,kernel,slots", CASES, ids=[c[0] for c in CASES])
def test_baseline_shape_bit_exact_vs_oracle(name, scenario, ov, n_act, E, steps, kernel, slots, oracle_lib, monkeypatch):
    if kernel is None:
        monkeypatch.delenv("RG_STEP_KERNEL", raising=False)
    else:
        monkeypatch.setenv("RG_STEP_KERNEL", kernel)
    shape_rollout_vs_oracle(name, scenario, ov, n_act, E, steps, slots, oracle_lib)


@pytest.mark.parametrize("scenario,ov,threshold", [
    ("PredatorCapturePrey", PCP5, 65536),
    ("PredatorCapturePrey", {"predator": 2, "capture": 1, "n_agents": 3}, 98304),
    ("PredatorCapturePrey", {}, 196608),                                                   # the reference's default: 4 agents
    ("Simple", {}, 393216),
    ("MaterialTransport", MT6, 65536),
    ("MaterialTransport", {"n_agents": 5, "n_fast_agents": 3, "n_slow_agents": 2, "start_dist": 0.25}, 49152),
    ("Warehouse", {}, 262144),                                                             # default: 6 agents
    ("PredatorCapturePrey", {"predator": 3, "capture": 3, "n_agents": 6}, 98304),
    ("Warehouse", WH8, None),                                                              # N >= 7: never
])
def test_kernel_choice_follows_the_measured_cross_overs(scenario, ov, threshold, monkeypatch):
    """`rg_create` picks the step kernel from (scenario, agent count, batch size): the table of robogym_capi.hip
    `tpe_min_envs`, measured with tools/crossover_probe.py (profiles/r3_crossover_probe.txt).  `rg_step_kernel` reports it."""
    from marbler_amd import VecRobotariumEnv
    monkeypatch.delenv("RG_STEP_KERNEL", raising=False)
    for E, want in ((4096, "group"),) + (((threshold - 1, "group"), (threshold, "tpe")) if threshold else ((524288, "group"),)):
        env = VecRobotariumEnv(scenario, E, overrides=ov, seed=0)
        assert env.step_kernel == want, (scenario, E, env.step_kernel)
        env.close()
    monkeypatch.setenv("RG_STEP_KERNEL", "tpe")
    env = VecRobotariumEnv(scenario, 64, overrides=ov, seed=0)
    assert env.step_kernel == ("tpe" if env.N <= 6 else "group")   # N <= 6 has a thread-per-env instantiation; above, the lane-group kernel
    env.close()
