"""The resident row kernels of the reference shapes (csrc/kernel_args.h RG_REF_SHAPES, csrc/robogym_resident_shapes.hip) against
the generic resident kernels: the same source with run-time values replaced by equal constants, so every word must agree.

A handle whose parameter block matches a row of the table launches that row's kernel (rg_step_form says so); a handle created
under RG_STEP_SHAPE=0 launches the generic resident kernel.  Both from the same seed, fed the same seeded random actions, with
auto-reset: every output array and the whole state after every step, word for word.

Batch sizes: 5 (one env per wave), 1026 (two per wave, ragged last wave), 2050 (four per wave, ragged): wave_fill's three
fillings of the 16-lane rows.  The stressed runs lower max_episode_steps to 8 and start the robots close together, and assert
from the outputs that episodes ended, violations occurred and a QP needed more than two sweeps: the resets, the drawn-ahead copy,
the chunk replays and the long QPs all ran.
"""
import ctypes as C

import pytest

from gpu_helpers import expected_slots, lane_group_kernel  # noqa: F401  (the fixture)
from shape_kernel_harness import OUTS, SHAPE_IDS, actions as _actions, differing as _differing, make as _make
from test_shape_kernels import REFERENCE, _match, _params, perturbed_cases

pytestmark = pytest.mark.gpu

STEPS = 100
STRESS = {"PredatorCapturePrey": {"max_episode_steps": 8, "start_dist": 0.2}, "Warehouse": {"max_episode_steps": 8, "start_dist": 0.3},
          "MaterialTransport": {"max_episode_steps": 8, "start_dist": 0.2}}
PERTURBED = perturbed_cases()


class _Happened:
    def __init__(self):
        self.done = self.viol = self.sweeps = 0

    def step(self, env):
        self.done += int(env.done_u8.sum())
        self.viol += int((env.violation != 0).sum())
        self.sweeps = max(self.sweeps, int(env.qp_sweeps.max()))


def _run_pair(scenario, ov, E, monkeypatch, steps=STEPS, guarded=False, other=(("RG_STEP_SHAPE", "0"),)):
    """-> (what happened, the shaped env's forms seen, the twin's)"""
    from marbler_amd import _lib
    new = _make(scenario, ov, E, monkeypatch, guarded=guarded)
    old = _make(scenario, ov, E, monkeypatch, env_vars=other)
    assert 5 <= new.N <= 8 and expected_slots(new.N, E) <= 4, "the case no longer dispatches a row kernel"
    acts = _actions(new, scenario, 16)
    seen, forms_new, forms_old = _Happened(), set(), set()
    for t in range(steps):
        new.step(acts[t % 16])
        old.step(acts[t % 16])
        forms_new.add(new.step_form)
        forms_old.add(old.step_form)
        bad = _differing(new, old)
        assert not bad, f"step {t}: {bad} differ"
        seen.step(new)
    if guarded:
        hit = new.red_zones_intact()
        assert hit.size == 0, f"{hit.size} red-zone bytes damaged, first after `{new.owner_of(int(hit[0]))}`"
    assert forms_old <= {_lib.FORM_RESIDENT, _lib.FORM_BY_VALUE}, forms_old
    new.close()
    old.close()
    return seen, forms_new, forms_old


@pytest.mark.parametrize("E", [5, 1026, 2050])
@pytest.mark.parametrize("scenario", sorted(REFERENCE))
def test_shape_kernel_equals_the_generic_kernel_word_for_word(scenario, E, monkeypatch):
    from marbler_amd import _lib
    seen, forms, twin = _run_pair(scenario, REFERENCE[scenario], E, monkeypatch)
    assert forms == {_lib.FORM_SHAPE + SHAPE_IDS[scenario]}, forms
    assert twin == {_lib.FORM_RESIDENT}, twin
    print(f"{scenario} E={E}: {seen.done} episodes ended, {seen.viol} violations, longest QP {seen.sweeps} sweeps")


@pytest.mark.parametrize("scenario", sorted(REFERENCE))
def test_stressed_run(scenario, monkeypatch):
    """Short episodes, robots started close together: resets (drawn-ahead copies and sampler runs), chunk replays, long QPs."""
    from marbler_amd import _lib
    seen, forms, _ = _run_pair(scenario, dict(REFERENCE[scenario], **STRESS[scenario]), 2050, monkeypatch)
    assert forms == {_lib.FORM_SHAPE + SHAPE_IDS[scenario]}, forms   # (neither override is a field of the shape)
    print(f"{scenario}: {seen.done} episodes ended, {seen.viol} violations, longest QP {seen.sweeps} sweeps")
    assert seen.done > 2050, "fewer than one ended episode per env"
    assert seen.viol > 0, "no violation: no chunk was replayed"
    assert seen.sweeps > 2, "no QP of more than two sweeps"


@pytest.mark.parametrize("scenario", sorted(REFERENCE))
def test_red_zones(scenario, monkeypatch):
    """E = 2049: a last wave with one env, whose replica half and idle rows store nothing; every array on the red-zone slab."""
    from marbler_amd import _lib
    seen, forms, _ = _run_pair(scenario, dict(REFERENCE[scenario], max_episode_steps=8), 2049, monkeypatch, steps=50, guarded=True)
    assert forms == {_lib.FORM_SHAPE + SHAPE_IDS[scenario]}, forms
    assert seen.done > 0


@pytest.mark.parametrize("name,scenario,ov,field", PERTURBED, ids=[c[0] for c in PERTURBED])
def test_a_perturbed_configuration_takes_the_generic_form(name, scenario, ov, field, monkeypatch):
    """Every configuration the matcher test perturbs: the generic resident kernel (where the agent count has row kernels at all),
    and the results of a handle on 8-lane groups (RG_STEP_SPAN=0) over 20 steps.  (A perturbation of a field that the table leaves
    to run time still matches, tests/test_shape_kernels.py: the shape's kernel then, with the same results.)"""
    from marbler_amd import _lib
    E = 67
    sid = _match(_params(scenario, ov))
    assert sid == 0 or field != "n_agents"
    new = _make(scenario, ov, E, monkeypatch)
    old = _make(scenario, ov, E, monkeypatch, env_vars=(("RG_STEP_SPAN", "0"),))
    acts = _actions(new, scenario, 4)
    for t in range(20):
        new.step(acts[t % 4])
        old.step(acts[t % 4])
        want = _lib.FORM_SHAPE + sid if sid else _lib.FORM_RESIDENT if 5 <= new.N <= 8 else _lib.FORM_BY_VALUE
        assert new.step_form == want, (t, new.step_form, want)
        assert old.step_form == _lib.FORM_BY_VALUE
        bad = _differing(new, old)
        assert not bad, f"step {t}: {bad} differ"
    new.close()
    old.close()


def test_a_change_to_the_handle_is_matched_again(monkeypatch):
    """What makes the image stale re-matches with the next image.  No rg_set_* changes a field a shape compiles in (the parameter
    block is fixed at rg_create); the setters that exist take the handle off the row kernels altogether: rg_set_disturbance on ->
    the disturbance family's by-value kernel at the next step, off -> a fresh image, matched again.  A re-bind: a fresh image,
    matched again.  Results against a twin under RG_STEP_SHAPE=0 that goes through the same changes."""
    from marbler_amd import _lib
    scenario, E = "PredatorCapturePrey", 1026
    shaped = _lib.FORM_SHAPE + SHAPE_IDS[scenario]
    new = _make(scenario, REFERENCE[scenario], E, monkeypatch)
    old = _make(scenario, REFERENCE[scenario], E, monkeypatch, env_vars=(("RG_STEP_SHAPE", "0"),))
    acts = _actions(new, scenario, 4)
    on = _lib.RgDisturbanceParams(0.01, 0.05)
    STATE = new.STATE_KEYS
    keep = []

    def run(n, want_new, want_old):
        for t in range(n):
            new.step(acts[t % 4])
            old.step(acts[t % 4])
            assert (new.step_form, old.step_form) == (want_new, want_old), (t, new.step_form, old.step_form)
            bad = _differing(new, old)
            assert not bad, f"step {t}: {bad} differ"

    run(10, shaped, _lib.FORM_RESIDENT)
    for env in (new, old):
        _lib.check(env.lib.rg_set_disturbance(env._h, C.byref(on)), "rg_set_disturbance")
    run(10, _lib.FORM_BY_VALUE, _lib.FORM_BY_VALUE)
    for env in (new, old):
        _lib.check(env.lib.rg_set_disturbance(env._h, None), "rg_set_disturbance")
    run(10, shaped, _lib.FORM_RESIDENT)
    for env in (new, old):   # a re-bind to copies of the arrays
        arrays = {k: getattr(env, k).clone() for k in STATE + ("next_init", "next_episode")}
        keep.append(arrays)
        st = _lib.RgState(*(arrays[k].data_ptr() for k in STATE), arrays["next_init"].data_ptr(), arrays["next_episode"].data_ptr())
        _lib.check(env.lib.rg_bind_state(env._h, C.byref(st)), "rg_bind_state")
        for k, v in arrays.items():
            setattr(env, k, v)
    run(10, shaped, _lib.FORM_RESIDENT)
    new.close()
    old.close()


@pytest.mark.parametrize("scenario", sorted(REFERENCE))
def test_a_captured_graph_of_shaped_steps(scenario, monkeypatch):
    """Ten rg_step launches of a shaped handle recorded into a graph, replayed twice, against twenty plain steps of a twin."""
    import torch
    from marbler_amd import _lib
    E = 1026
    new = _make(scenario, REFERENCE[scenario], E, monkeypatch)
    old = _make(scenario, REFERENCE[scenario], E, monkeypatch, env_vars=(("RG_STEP_SHAPE", "0"),))
    acts = _actions(new, scenario, 10)
    for t in range(5):   # (eager steps first: the image written, the seed known to the handle)
        new.step(acts[t])
        old.step(acts[t])
    assert new.step_form == _lib.FORM_SHAPE + SHAPE_IDS[scenario]
    dev = new.device
    io = _lib.RgStepIO(*(getattr(new, k).data_ptr() for k in OUTS))
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    prev = new._stream
    new.set_stream(side)
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            for i in range(10):
                assert new.lib.rg_step(new._h, acts[i].data_ptr(), C.byref(io), 1, new.seed) == 0
        assert new.step_form == _lib.FORM_SHAPE + SHAPE_IDS[scenario]   # the captured launches are the shape's kernel
        graph.replay()
        graph.replay()
    torch.cuda.synchronize(dev)
    new.set_stream(prev)
    torch.cuda.current_stream(dev).wait_stream(side)
    for t in range(20):
        old.step(acts[t % 10])
    torch.cuda.synchronize(dev)
    bad = _differing(new, old)
    assert not bad, bad
    del graph
    new.close()
    old.close()
