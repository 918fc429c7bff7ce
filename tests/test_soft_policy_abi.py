"""Soft-policies sampling on the CPU tier: the two entry points and the struct exist next to an unchanged ABI version, every
argument refusal that needs no device returns its code with a reason, and the Python layers refuse bad arguments before the env
or the device is touched.  (rg_create needs a device, so the refusals of rg_policy_rollout that look at a handle -- interior-point
mode, lidar, team pool, packing -- are reached here through marbler_amd.evaluate.policy_rollout's own checks with stub objects, and
with a real handle in tests/test_gpu_soft_policy.py.)"""
import ctypes as C
import os
import sys
import tempfile
import types

import pytest
import torch


def _lib():
    from marbler_amd import _lib
    return _lib, _lib.load()


def test_exports_and_struct():
    _l, lib = _lib()
    assert lib.rg_abi_version() == 7
    assert lib.rg_sizeof_policy_io() == C.sizeof(_l.RgPolicyIO)            # no existing struct changed
    assert lib.rg_sizeof_policy_sample() == C.sizeof(_l.RgPolicySample) == 16
    for name in ("rg_actor_forward_sample", "rg_policy_rollout_sample", "rg_sizeof_policy_sample"):
        assert hasattr(lib, name) and name in _l.EXPORTS


def test_actor_forward_sample_refusals():
    _l, lib = _lib()
    buf = (C.c_float * 64)()
    w = _l.RgActorWeights()
    p = C.addressof(buf)
    # NULL sample_u, NULL actions
    assert lib.rg_actor_forward_sample(C.byref(w), 1, 1, p, 4, 0, None, p, None, p, None, None, None) == -12
    assert b"sample_u is NULL" in lib.rg_actor_last_error()
    assert lib.rg_actor_forward_sample(C.byref(w), 1, 1, p, 4, 0, None, p, None, None, p, None, None) == -12
    assert b"actions" in lib.rg_actor_last_error()
    # the actor launch's own checks apply behind them
    assert lib.rg_actor_forward_sample(None, 1, 1, p, 4, 0, None, p, None, p, p, None, None) == -1
    assert b"NULL" in lib.rg_actor_last_error()
    assert lib.rg_actor_forward_sample(C.byref(w), 1, 1, p, 4, 0, None, p, None, p, p, None, None) == -2
    assert b"weight array" in lib.rg_actor_last_error()
    for k in ("w1", "b1", "wih", "bih", "whh", "bhh", "w2", "b2"):
        setattr(w, k, p)
    w.n_sets, w.input_dim, w.hidden_dim, w.n_actions, w.use_rnn, w.gru_packed = 1, 4, 96, 5, 1, 3
    assert lib.rg_actor_forward_sample(C.byref(w), 1, 1, p, 4, 0, None, p, None, p, p, None, None) == -3
    assert b"hidden_dim" in lib.rg_actor_last_error()
    w.hidden_dim, w.n_actions = 64, 33
    assert lib.rg_actor_forward_sample(C.byref(w), 1, 1, p, 4, 0, None, p, None, p, p, None, None) == -4
    assert b"n_actions" in lib.rg_actor_last_error()


def test_policy_rollout_sample_refusals():
    _l, lib = _lib()
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    w, io = _l.RgActorWeights(), _l.RgStepIO()
    pio = _l.RgPolicyIO()
    # NULL sample / NULL sample_u
    assert lib.rg_policy_rollout_sample(None, C.byref(w), 1, C.byref(pio), None, C.byref(io), 1, 0) == -55
    assert b"sample_u is NULL" in lib.rg_last_error()
    ps = _l.RgPolicySample(None, p)
    assert lib.rg_policy_rollout_sample(None, C.byref(w), 1, C.byref(pio), C.byref(ps), C.byref(io), 1, 0) == -55
    # sample_u together with explore_u
    ps = _l.RgPolicySample(p, None)
    pio.explore_u, pio.epsilon = p, 0.1
    assert lib.rg_policy_rollout_sample(None, C.byref(w), 1, C.byref(pio), C.byref(ps), C.byref(io), 1, 0) == -56
    assert b"explore_u" in lib.rg_last_error()
    # behind them: rg_policy_rollout's own refusals, the first of which is the handle
    pio.explore_u = None
    assert lib.rg_policy_rollout_sample(None, C.byref(w), 1, C.byref(pio), C.byref(ps), C.byref(io), 1, 0) == -1
    assert b"handle is NULL" in lib.rg_last_error()
    assert lib.rg_policy_rollout(None, C.byref(w), 1, C.byref(pio), C.byref(io), 1, 0) == -1


def test_sampling_kernels_are_in_the_shipped_library_and_fit():
    """Six actor_sample_kernel<H, SPLIT> (two tiles per CU: at most 256 registers, no scratch, the actor's LDS) and 26
    policy_rollout_sample_kernel<SCN, GW, H> (LDS within the CU's 160 KB), next to the unchanged greedy kernels.  The DOT-hazard
    and exec-restore scans of tests/test_kernel_resources.py run over every kernel of the library, these included."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import isa_scan
    from marbler_amd import build
    actor, policy, greedy = {}, {}, {}
    with tempfile.TemporaryDirectory() as d:
        for co in isa_scan.extract_code_objects(build.LIB, d):
            for k, r in isa_scan.resources(co).items():
                if "actor_sample_kernel" in k:
                    actor[k] = r
                elif "policy_rollout_sample_kernel" in k:
                    policy[k] = r
                elif "actor_kernel" in k or "policy_rollout_kernel" in k:
                    greedy[k] = r
    assert len(actor) == 6 and len(policy) == 26 and len(greedy) == 32
    for k, r in actor.items():
        planes2 = "ELi2EEE" in k
        assert r["vgpr"] + r["agpr"] <= 256 and r["scratch"] == 0 and r["lds"] <= (48 if planes2 else 32) * 1024, (k, r)
    for k, r in policy.items():
        h = 128 if "ELi128E" in k else 64
        assert (3 * 32 + 64) * h * 4 <= r["lds"] <= 160 * 1024, (k, r)
        twin = greedy[k.replace("28policy_rollout_sample_kernel", "21policy_rollout_kernel")]
        assert r["lds"] == twin["lds"], (k, r, twin)      # the same shared arrays


def _stub_env(**kw):
    d = dict(params=types.SimpleNamespace(qp_mode=0), teams=None, lidar=None, D=9, N=4, E=3, auto_reset=True, seed=0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _stub_actor(**kw):
    d = dict(use_rnn=True, pack_gru="f16x2", hidden_dim=64, input_dim=13)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_python_policy_rollout_refusals_need_no_device():
    from marbler_amd.evaluate import policy_rollout
    u = torch.zeros(2, 3, 4)
    args = dict(T=2, io=None, hidden=None, actions=None)
    for env, actor, what in ((_stub_env(params=types.SimpleNamespace(qp_mode=1)), _stub_actor(), "interior-point"),
                             (_stub_env(teams=object()), _stub_actor(), "team pool"),
                             (_stub_env(lidar=object()), _stub_actor(), "lidar"),
                             (_stub_env(), _stub_actor(pack_gru="bf16x3"), "two binary16 planes"),
                             (_stub_env(), _stub_actor(use_rnn=False), "two binary16 planes"),
                             (_stub_env(), _stub_actor(hidden_dim=96), "hidden size"),
                             (_stub_env(), _stub_actor(input_dim=9), "inputs per agent")):
        with pytest.raises(ValueError, match=what):
            policy_rollout(env, actor, sample_u=u, **args)
    with pytest.raises(ValueError, match="do not combine"):
        policy_rollout(_stub_env(), _stub_actor(), sample_u=u, explore_u=u, epsilon=0.1, **args)
    with pytest.raises(ValueError, match="prob needs sample_u"):
        policy_rollout(_stub_env(), _stub_actor(), prob=u, **args)
    for bad in (torch.zeros(2, 3, 5), torch.zeros(2, 3, 4, dtype=torch.float64), torch.zeros(2, 4, 3).transpose(1, 2)):
        with pytest.raises(ValueError, match="sample_u must be a contiguous float32"):
            policy_rollout(_stub_env(), _stub_actor(), sample_u=bad, **args)
    with pytest.raises(ValueError, match="prob must be a contiguous float32"):
        policy_rollout(_stub_env(), _stub_actor(), sample_u=u, prob=torch.zeros(2, 3), **args)


class _NoTouch(object):
    """An env that fails the test the moment anything reads it."""

    def __getattr__(self, name):
        raise AssertionError(f"the env was touched ({name}) before the arguments were checked")


def test_batched_runner_argument_errors_come_first():
    from marbler_amd.gymma import BatchedRunner
    with pytest.raises(ValueError, match="does not combine with epsilon"):
        BatchedRunner(_NoTouch(), _NoTouch(), epsilon=0.05, action_selector="soft_policies")
    with pytest.raises(ValueError, match="action_selector must be one of"):
        BatchedRunner(_NoTouch(), _NoTouch(), action_selector="gumbel")
    with pytest.raises(ValueError, match="action_selector must be one of"):
        BatchedRunner(_NoTouch(), _NoTouch(), action_selector=None)
