"""The sweep loop of the 16-lane-row step kernels (step_group.h controller<>, SPAN): envs leave the loop one by one with their
own verdict, and the sweeps that follow run under the mask of the envs that are left.  Free-running rollouts against the float32
oracle, bit for bit (every output, `qp_sweeps` and the state: _rollout_bit_exact), at shapes where the envs of a wave stop at
different sweeps, where the cap `qp_max_sweeps` ends a QP at every phase of a block of four sweeps, and with a ragged last wave.
Each case also asserts that the run really held those QPs: the histogram of `qp_sweeps` over all steps and envs (the oracle's,
which the helper has just compared with the kernel's step by step) contains the listed counts.  The counts were taken from the
oracle alone, with the helper's seeds (env seed 99, action seed 5)."""
import numpy as np
import pytest

from physical_cases import MT6, PCP5
from rollout_harness import rollout_bit_exact



class _SweepHistogram(object):
    """The oracle module, with OracleVecEnv instances that add every step's `qp_sweeps` to a histogram."""

    def __init__(self, lib):
        self._lib = lib
        self.hist = np.zeros(128, np.int64)

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def OracleVecEnv(self, *args, **kwargs):
        orc = self._lib.OracleVecEnv(*args, **kwargs)
        step = orc.step

        def recording_step(actions, **kw):
            out = step(actions, **kw)
            self.hist += np.bincount(orc.qp_sweeps, minlength=128)[:128]
            return out
        orc.step = recording_step
        return orc


def _run(scenario, ov, n_act, steps, E, oracle_lib, monkeypatch):
    monkeypatch.setenv("RG_STEP_KERNEL", "group")
    monkeypatch.delenv("RG_STEP_SPAN", raising=False)
    rec = _SweepHistogram(oracle_lib)
    rollout_bit_exact(scenario, ov, n_act, steps, rec, E, require_done=False)
    assert rec.hist.sum() == steps * E
    print(scenario, ov, E, steps, "qp_sweeps histogram:", {int(k): int(v) for k, v in enumerate(rec.hist) if v})
    return rec.hist


@pytest.mark.gpu
def test_one_env_per_wave_every_sweep_count(oracle_lib, monkeypatch):
    """PredatorCapturePrey 64 x 5, 150 steps: one env per wave; every count 1 .. 12 occurs at least twice."""
    h = _run("PredatorCapturePrey", PCP5, 5, 150, 64, oracle_lib, monkeypatch)
    assert all(h[c] >= 2 for c in range(1, 13)), h[:16]


@pytest.mark.gpu
def test_four_envs_per_wave_leave_at_different_sweeps(oracle_lib, monkeypatch):
    """PredatorCapturePrey 2052 x 5, 40 steps: four envs per wave, converging at different sweeps; counts 1 .. 13 occur."""
    h = _run("PredatorCapturePrey", PCP5, 5, 40, 2052, oracle_lib, monkeypatch)
    assert all(h[c] >= 1 for c in range(1, 14)), h[:16]


# (qp_max_sweeps, how often a QP of the run ends AT the cap): a sweep run past the cap, or a verdict taken one sweep late, cannot hide
CAPS = [(1, 6400), (2, 3670), (3, 788), (4, 713), (5, 146), (7, 112), (8, 87)]


@pytest.mark.gpu
@pytest.mark.parametrize("cap,at_cap", CAPS)
def test_cap_reached_at_every_phase(cap, at_cap, oracle_lib, monkeypatch):
    """PredatorCapturePrey 64 x 5, 100 steps, with qp_max_sweeps = 1, 2, 3, 4, 5, 7, 8 (every phase of a block of four sweeps,
    the restart's included)."""
    h = _run("PredatorCapturePrey", dict(PCP5, qp_max_sweeps=cap), 5, 100, 64, oracle_lib, monkeypatch)
    assert h[cap] == at_cap and h[cap + 1:].sum() == 0, h[:16]


@pytest.mark.gpu
def test_cap_with_four_envs_per_wave(oracle_lib, monkeypatch):
    """qp_max_sweeps = 5 at 2052 envs, 20 steps: 935 capped QPs beside envs of the same wave that stop earlier."""
    h = _run("PredatorCapturePrey", dict(PCP5, qp_max_sweeps=5), 5, 20, 2052, oracle_lib, monkeypatch)
    assert h[5] == 935 and h[6:].sum() == 0, h[:16]


@pytest.mark.gpu
def test_eight_agents_ragged_last_wave(oracle_lib, monkeypatch):
    """Warehouse 2049 x 8, 30 steps: NT = 8 (all seven rounds hold real pairs), one env alone in the last wave, counts up to 16."""
    h = _run("Warehouse", {"n_agents": 8}, 5, 30, 2049, oracle_lib, monkeypatch)
    assert h[16] >= 1 and h[3:16].sum() > 0, h[:24]


@pytest.mark.gpu
@pytest.mark.parametrize("scenario,ov,n_act", [("MaterialTransport", MT6, 20), ("Simple", {"n_agents": 7}, 5)])
def test_six_and_seven_agents(scenario, ov, n_act, oracle_lib, monkeypatch):
    """NT = 6 and 7 at 64 envs, 100 steps: multi-sweep QPs in the other two agent counts' instantiations."""
    h = _run(scenario, ov, n_act, 100, 64, oracle_lib, monkeypatch)
    assert h[3:].sum() > 0, h[:24]
