"""GPU parity (the -m gpu tier): the HIP step kernels, called through the C ABI, against
  (1) the float32 oracle (oracle/oracle.c, tier 3)  -- BIT-EXACT on every output and on the state (tests/oracle_check.py),
  (2) the golden vectors captured from the reference's own Python (float64) -- the bar of
      tests/parity.py: masks exact, observations / rewards / dist / xy within 1e-5 in every scenario,
      headings within the committed per-fixture bound, near-tie rows explained one by one.
"""
import numpy as np
import pytest

from helpers import golden_files, gpu_from_state, load_golden, oracle_from_state, pre_state
from oracle_check import assert_outputs, assert_state, gpu_outputs, gpu_state, load_oracle

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("step_kernel")]


def _run_gpu(scenario, cfg, state, actions):
    import torch
    env = gpu_from_state(scenario, cfg, state)
    a = torch.as_tensor(np.asarray(actions, dtype=np.int32), device=env.device)
    obs, rew, done, info = env.step(a)
    torch.cuda.synchronize()
    out = {"obs": obs.cpu().numpy(), "reward": rew.cpu().numpy(), "done": done.cpu().numpy().astype(np.uint8),
           "dist": info["dist_travelled"].cpu().numpy(), "viol": info["violation"].cpu().numpy(),
           "remaining": info["remaining"].cpu().numpy(), "qp_sweeps": env.qp_sweeps.cpu().numpy()}
    post = {k: v.cpu().numpy() for k, v in env.state_dict().items()}
    env.close()
    return out, post


@pytest.mark.parametrize("path", golden_files(), ids=lambda p: p.split("/")[-1][:-4])
def test_step_bit_exact_vs_f32_oracle(path, oracle_lib):
    g, scenario, cfg = load_golden(path)
    state = pre_state(g)
    import torch
    env = gpu_from_state(scenario, cfg, state)
    orc = oracle_from_state(oracle_lib, scenario, cfg, state, np.float32)
    # the arrays the fixture does not carry (another scenario's) start from the product's own fill: goal_col is 1 there
    load_oracle(orc, {k: v for k, v in gpu_state(env).items() if k not in state})
    orc.step(g["actions"])
    env.step(torch.as_tensor(np.asarray(g["actions"], dtype=np.int32), device=env.device))
    torch.cuda.synchronize()
    assert_outputs(gpu_outputs(env), orc, path)
    assert_state(gpu_state(env), orc, label=path)
    env.close()


@pytest.mark.parametrize("path", golden_files(), ids=lambda p: p.split("/")[-1][:-4])
def test_step_vs_reference_golden(path):
    """The bar of tests/parity.py against the reference's own vectors: masks exact; x, y, dist, rewards and
    observations within 1e-5 in EVERY scenario (74 sub-steps included); headings within 2x the maximum
    measured for the fixture (PARITY_REPORT.json); an observation row over 1e-5 must be explained by a
    float64 near-tie of the neighbour order / nearest prey -- zero unexplained rows."""
    import os
    import parity
    g, scenario, cfg = load_golden(path)
    name = os.path.basename(path)[:-4]
    out, post = _run_gpu(scenario, cfg, pre_state(g), g["actions"])
    assert int(out["qp_sweeps"].max()) < 40, "a barrier QP hit its sweep cap: the result would be an unconverged iterate"
    got = dict(out, poses=post["poses"])
    for k in parity.MASK_KEYS:
        got[k] = post[k]
    m = parity.check_step_parity(scenario, cfg, name, got, parity.golden_want(g), theta_limit=parity.theta_bound(name, cfg))
    rep = parity.load_report()["fixtures"][name]
    # the kernels are bit-identical to the float32 oracle the report was generated from
    assert m["tie_rows"] == rep["tie_rows"] and abs(m["max_xy"] - rep["max_xy"]) < 1e-12, (m, rep)
