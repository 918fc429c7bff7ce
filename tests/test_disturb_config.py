"""The pose disturbance on the CPU tier (DESIGN.md "Pose disturbance"): the C ABI's struct and exports next to an unchanged ABI
version, the config keys' validation, the NumPy twin's own properties (tests/disturb_twin.py: range, moments, independence of the
three variates, what a draw is keyed by, no collision with the team pool's block), its scale against a stand-alone C++ evaluation
of the same expression, the Python refusals that need no device, and the set of kernels the library ships for it."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

from disturb_twin import C_MAX, C_STD, DISTURB_BLOCK, displace, scale, variates, wrap_spec
from team_twin import TEAM_BLOCK, philox4x32_10

from marbler_amd import _lib
from marbler_amd.params import disturbance_params, load_config, make_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the C ABI
def _library():
    from marbler_amd import build as hip_build
    if not os.path.exists(hip_build.LIB):
        pytest.skip("librobogym_hip.so is not built")
    return _lib.load()


def test_struct_layout_and_exports():
    f = {name: getattr(_lib.RgDisturbanceParams, name) for name, _ in _lib.RgDisturbanceParams._fields_}
    assert [(n, f[n].offset, f[n].size) for n in ("sigma_xy", "sigma_theta", "reserved")] == \
        [("sigma_xy", 0, 4), ("sigma_theta", 4, 4), ("reserved", 8, 8)]
    assert C.sizeof(_lib.RgDisturbanceParams) == 16
    assert {"rg_sizeof_disturbance_params", "rg_set_disturbance"} <= set(_lib.EXPORTS)
    lib = _library()
    assert lib.rg_abi_version() == 7 == _lib.ABI_VERSION
    assert lib.rg_sizeof_disturbance_params() == 16
    dp = _lib.RgDisturbanceParams(0.01, 0.05)
    assert lib.rg_set_disturbance(None, C.byref(dp)) == -1
    assert "handle" in lib.rg_last_error().decode()
    assert lib.rg_set_disturbance(None, None) == -1


def test_header_declares_the_disturbance():
    text = open(os.path.join(ROOT, "include", "robogym.h")).read()
    assert "#define RG_ABI_VERSION 7" in text
    for s in ("typedef struct rg_disturbance_params", "float sigma_xy;", "float sigma_theta;", "float reserved[2];",
              "int rg_set_disturbance(rg_handle *h, const rg_disturbance_params *dp);", "int rg_sizeof_disturbance_params(void);"):
        assert s in text, s


# ---------------------------------------------------------------- config keys
def _params(scenario="PredatorCapturePrey", **ov):
    cfg = load_config(scenario, overrides=ov)
    return disturbance_params(scenario, cfg, make_params(scenario, cfg))


def test_absent_or_zero_keys_mean_off():
    for scenario in ("PredatorCapturePrey", "Warehouse", "MaterialTransport", "Simple", "ArcticTransport"):
        assert _params(scenario) is None                                      # the shipped YAMLs carry both keys at 0
        assert _params(scenario, pose_noise_xy=0, pose_noise_theta=0.0) is None
    cfg = load_config("Simple")
    cfg.pop("pose_noise_xy")
    cfg.pop("pose_noise_theta")
    assert disturbance_params("Simple", cfg, make_params("Simple", cfg)) is None


def test_values_reach_the_block_as_binary32():
    dp = _params(pose_noise_xy=0.01, pose_noise_theta=0.05)
    assert dp.sigma_xy == float(np.float32(0.01)) and dp.sigma_theta == float(np.float32(0.05))
    assert tuple(dp.reserved) == (0.0, 0.0)
    dp = _params(pose_noise_xy=0.1, pose_noise_theta=0.5)                     # the bounds themselves are admitted
    assert dp.sigma_xy == float(np.float32(0.1)) and dp.sigma_theta == 0.5
    assert _params(pose_noise_xy=0.02).sigma_theta == 0.0 and _params(pose_noise_theta=0.02).sigma_xy == 0.0
    assert _params(pose_noise_xy=np.float32(0.03)).sigma_xy == float(np.float32(0.03))


@pytest.mark.parametrize("key,bad", [("pose_noise_xy", -1e-9), ("pose_noise_xy", 0.1000001), ("pose_noise_xy", float("nan")),
                                     ("pose_noise_xy", float("inf")), ("pose_noise_xy", "0.01"), ("pose_noise_xy", True),
                                     ("pose_noise_xy", None), ("pose_noise_xy", [0.01]),
                                     ("pose_noise_theta", -0.001), ("pose_noise_theta", 0.5000001), ("pose_noise_theta", float("nan")),
                                     ("pose_noise_theta", float("-inf")), ("pose_noise_theta", "x"), ("pose_noise_theta", False)])
def test_bad_values_are_refused_by_name(key, bad):
    with pytest.raises(ValueError, match=key):
        _params(**{key: bad})


def test_lidar_and_pool_exclusions():
    with pytest.raises(ValueError, match="lidar"):
        _params(pose_noise_xy=0.01, lidar_rays=8)
    with pytest.raises(ValueError, match="team pool"):
        _params(pose_noise_theta=0.01, teams=[{}])
    # ... and not when the disturbance is off
    assert _params(lidar_rays=8) is None and _params(teams=[{}]) is None
    with pytest.raises(KeyError, match="not built"):
        disturbance_params("Nowhere", {}, None)


# ---------------------------------------------------------------- the twin
def test_variates_stay_in_range_and_reach_its_ends_only_by_construction():
    c = variates(3, np.arange(1 << 16), 0, 0, 0)
    for cj in c:
        assert cj.dtype == np.int32 and cj.min() >= -C_MAX and cj.max() <= C_MAX
    # the extreme words give the extreme sums
    assert 4 * 1023 - C_MAX == C_MAX and 0 - C_MAX == -C_MAX
    assert abs(C_MAX / C_STD - 3.46) < 0.01


def test_moments_and_independence_of_the_three_variates():
    n = 1 << 18
    ge = np.arange(n) % 4096
    s = np.arange(n) // 4096
    z = [cj / C_STD for cj in variates(11, ge, 2, s, 1)]
    for zj in z:
        assert abs(zj.mean()) < 0.01, zj.mean()
        assert abs(zj.var() - 1.0) < 0.02, zj.var()
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert abs(np.mean(z[i] * z[j]) - z[i].mean() * z[j].mean()) < 0.01, (i, j)
    # exact variance of the sum of four uniforms on 0..1023
    assert C_STD ** 2 == pytest.approx(4 * (1024 ** 2 - 1) / 12.0, rel=1e-15)


def test_a_draw_is_keyed_by_env_episode_step_agent_and_seed():
    ge = np.arange(512)
    base = np.stack(variates(5, ge, 3, 7, 2))
    assert np.array_equal(base, np.stack(variates(5, ge, 3, 7, 2)))
    for other in (variates(5, ge + 512, 3, 7, 2), variates(5, ge, 4, 7, 2), variates(5, ge, 3, 8, 2), variates(5, ge, 3, 7, 3),
                  variates(6, ge, 3, 7, 2), variates(5 + (1 << 32), ge, 3, 7, 2), variates(5, ge + (1 << 32), 3, 7, 2)):
        assert (np.stack(other) != base).mean() > 0.9
    # the block: 0x40000000 | (s & 0x3FFFFFF) << 4 | a -- the step count wraps at 2^26, agents 0..15 never reach the step's bits
    assert np.array_equal(np.stack(variates(5, ge, 3, 7 + (1 << 26), 2)), base)
    w = philox4x32_10(ge, 0, 3, DISTURB_BLOCK | (7 << 4) | 2, 5, 0)
    want = [sum(((wi >> np.uint32(10 * j)) & np.uint32(1023)).astype(np.int64) for wi in w) - C_MAX for j in range(3)]
    assert np.array_equal(np.stack(want), base)


def test_blocks_do_not_collide_with_the_reset_sampler_or_the_team_draw():
    s = np.array([0, 1, (1 << 26) - 1, 1 << 26, -1 & 0xFFFFFFFF], np.int64)[:, None]
    a = np.arange(16)[None, :]
    blk = DISTURB_BLOCK | ((s & 0x3FFFFFF) << 4) | a
    assert blk.min() >= DISTURB_BLOCK > 32 and blk.max() < TEAM_BLOCK
    assert len(np.unique(blk[:3])) == 3 * 16


def test_displace_is_the_float32_update():
    rng = np.random.RandomState(0)
    E, N = 40, 6
    poses = np.stack([rng.uniform(-1.5, 1.5, (E, N)), rng.uniform(-1, 1, (E, N)), rng.uniform(-np.pi, np.pi, (E, N))], axis=1).astype(np.float32)
    poses[:, 2, 0] = np.float32(np.pi)       # at the wrap
    poses[:, 2, 1] = -np.float32(np.pi)
    rc, st = rng.randint(1, 5, E), rng.randint(0, 30, E)
    out = displace(poses, 9, 100, rc, st, 0.01, 0.05)
    assert out.dtype == np.float32 and out.shape == poses.shape
    c = variates(9, (100 + np.arange(E))[:, None], (rc - 1)[:, None], st[:, None], np.arange(N)[None, :])
    for e in range(0, E, 7):
        for a in range(N):
            x = np.float32(poses[e, 0, a] + np.float32(scale(0.01) * np.float32(c[0][e, a])))
            th = np.float32(poses[e, 2, a] + np.float32(scale(0.05) * np.float32(c[2][e, a])))
            assert out[e, 0, a] == x and out[e, 2, a] == wrap_spec(th)
    assert (np.abs(out[:, 2]) <= np.float32(np.pi)).all()
    assert (out[:, 2, 0] != poses[:, 2, 0]).any() and (out != poses).mean() > 0.9
    dxy = (out[:, :2].astype(np.float64) - poses[:, :2]) / 0.01
    assert np.abs(dxy).max() <= 3.47 and 0.7 < dxy.std() < 1.3
    # a zero sigma leaves that part alone
    assert np.array_equal(displace(poses, 9, 100, rc, st, 0.0, 0.05)[:, :2], poses[:, :2])
    assert np.array_equal(displace(poses, 9, 100, rc, st, 0.01, 0.0)[:, 2], poses[:, 2])


def test_scale_equals_a_stand_alone_cpp_evaluation(tmp_path):
    """k = binary32(double(sigma) * sqrt(3.0 / 1048575.0)) as a C++ compiler evaluates it (the expression of csrc/kernel_args.h
    disturb_scale), bit for bit, for a handful of sigma."""
    import shutil
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    sigmas = [0.01, 0.05, 0.1, 0.5, 1e-4, 0.0333, 0.0]
    src = tmp_path / "k.cpp"
    src.write_text('#include <cmath>\n#include <cstdio>\n#include <cstring>\n#include <cstdlib>\n'
                   'static float disturb_scale(float sigma) { return static_cast<float>(static_cast<double>(sigma) * sqrt(3.0 / 1048575.0)); }\n'
                   'int main(int argc, char **argv) {\n'
                   '    for (int i = 1; i < argc; ++i) { volatile float s = strtof(argv[i], nullptr); float k = disturb_scale(s);\n'
                   '        unsigned u; memcpy(&u, &k, 4); printf("%08x\\n", u); }\n    return 0;\n}\n')
    exe = tmp_path / "k"
    subprocess.check_call([cxx, "-O2", "-ffp-contract=off", str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)] + [repr(float(np.float32(s))) for s in sigmas], text=True).split()
    assert [int(v, 16) for v in out] == [int(np.float32(scale(s)).view(np.uint32)) for s in sigmas]
    text = open(os.path.join(ROOT, "marbler_amd", "csrc", "kernel_args.h")).read()
    assert "static_cast<float>(static_cast<double>(sigma) * sqrt(3.0 / 1048575.0))" in text
    assert float(scale(0.01)) * C_STD == pytest.approx(0.01, rel=1e-6)


# ---------------------------------------------------------------- Python refusals that need no device
def _stub_env(**kw):
    d = dict(params=types.SimpleNamespace(qp_mode=0), teams=None, lidar=None, disturbance=None, D=9, N=4, E=3, auto_reset=True, seed=0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_one_launch_paths_refuse_a_disturbed_env_before_touching_it():
    from marbler_amd.evaluate import policy_rollout, run_eval
    actor = types.SimpleNamespace(use_rnn=True, pack_gru="f16x2", hidden_dim=64, input_dim=13)
    with pytest.raises(ValueError, match="pose disturbance"):
        policy_rollout(_stub_env(disturbance=object()), actor, T=2, io=None, hidden=None, actions=None)
    with pytest.raises(ValueError, match="pose disturbance"):
        run_eval(_stub_env(disturbance=object()), actor, 4, one_launch=True)       # (the stub has no reset(): nothing was called)
    from marbler_amd.gymma import BatchedRunner
    runner = BatchedRunner.__new__(BatchedRunner)
    runner.venv = types.SimpleNamespace(env=_stub_env(disturbance=object(), device="cpu"), E=3, n_agents=4, obs_size=9, n_actions=5)
    with pytest.raises(ValueError, match="pose disturbance"):
        runner.run(2, one_launch=True)


# ---------------------------------------------------------------- the shipped kernels
@pytest.fixture(scope="module")
def shipped():
    from marbler_amd import build as hip_build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_scan
    if not os.path.exists(hip_build.LIB):
        pytest.skip("librobogym_hip.so is not built")
    try:
        return isa_scan.scan_library(hip_build.LIB)
    except RuntimeError as exc:
        pytest.skip(str(exc))


def test_disturbance_kernel_set(shipped):
    """disturb_step_kernel<SCN, GW, ROLLOUT, GYM, QPM>.  Exact mode: single step, gymma single step and rollout for GW 4 / 8 / 16 of
    four scenarios (36) and ArcticTransport's GW 4 (3); interior-point mode: the same three for GW 4 / 8 (24) and ArcticTransport (3)."""
    ks = {k: r["resources"] for k, r in shipped.items() if "disturb_step_kernel" in k}
    exact = {k: r for k, r in ks.items() if k.endswith("ELi0EEEvNS_11DisturbArgsE")}
    ipm = {k: r for k, r in ks.items() if k.endswith("ELi1EEEvNS_11DisturbArgsE")}
    assert len(exact) == 39 and len(ipm) == 27 and len(ks) == 66, (len(exact), len(ipm), len(ks))
    for scn in range(5):
        for gw in ((4, 8, 16) if scn < 4 else (4,)):
            for rollout, gym in ((0, 0), (0, 1), (1, 0)):
                assert any(f"disturb_step_kernelILi{scn}ELi{gw}ELb{rollout}ELb{gym}ELi0E" in k for k in exact), (scn, gw, rollout, gym)
                if gw != 16:
                    assert any(f"disturb_step_kernelILi{scn}ELi{gw}ELb{rollout}ELb{gym}ELi1E" in k for k in ipm), (scn, gw, rollout, gym)
    # exact mode: no spilled register and scratch within the lane-group kernels' bound (tests/test_kernel_resources.py); the
    # single-launch forms -- what rg_step runs -- keep at least the waves per SIMD of the lidar family's kernel of the same form
    # (the same generic body).  The multi-step forms are not held to that: at 16 lanes per env every family's rollout sits on the
    # 256-register boundary (lidar 254..268, team 254..266, plain 297..416 registers; this family 257..270), one allocator
    # decision away from either side, and DESIGN.md reports them instead.
    lidar = {k: r["resources"] for k, r in shipped.items() if "lidar_step_kernel" in k}
    for k, r in exact.items():
        m = re.fullmatch(r"_ZN2rg19disturb_step_kernelILi(\d)ELi(\d+)ELb(\d)ELb(\d)ELi0EEEvNS_11DisturbArgsE", k)
        assert m, k
        twin = "_ZN2rg17lidar_step_kernelILi%sELi%sELb0ELb%sELb%sELi0EEEvNS_9LidarArgsE" % m.groups()      # OBS_ONLY = false
        assert twin in lidar, (k, twin)
        assert r["spill"] == 0 and r["scratch"] <= 128, (k, r)
        if m.group(3) == "0":
            assert r["occupancy"] >= lidar[twin]["occupancy"], (k, r, lidar[twin])
