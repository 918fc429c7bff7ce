"""marbler_amd._args: the rules every Python launch wrapper shares (the tensor check, the episode pitch), and the entry table
of marbler_amd._lib.  Host code only: no library, no device."""
import numpy as np
import pytest
import torch

from marbler_amd import _args, _lib

CLASSES = ((TypeError, ValueError), (TypeError, TypeError), (ValueError, ValueError))     # episodes, render, unroll / td_targets


@pytest.mark.parametrize("errors", CLASSES)
def test_check_tensor_refusals(errors):
    good = torch.zeros(3, 4, 5)
    kw = dict(dtypes=(torch.float32, torch.float64), shape=(3, 4, 5), errors=errors)
    assert _args.check_tensor("x", good, **kw) is good
    assert _args.check_tensor("x", good.double(), device=torch.device("cpu"), **kw).dtype == torch.float64
    with pytest.raises(errors[0], match="x must be a contiguous float32 or float64 tensor of shape .3, 4, 5., got ndarray") as err:
        _args.check_tensor("x", np.zeros((3, 4, 5), np.float32), **kw)
    assert type(err.value) is errors[0]
    with pytest.raises(errors[1], match="got torch.int32") as err:
        _args.check_tensor("x", good.to(torch.int32), **kw)
    assert type(err.value) is errors[1]
    for bad, word in ((torch.zeros(3, 4, 6), "got the shape .3, 4, 6."), (torch.zeros(3, 4), "got the shape"),
                      (torch.zeros(3, 4, 10)[..., ::2], "got the strides .40, 10, 2."), (torch.zeros(4, 3, 5).transpose(0, 1), "strides"),
                      (torch.zeros(3, 4, 5, device="meta"), "x is on meta, not on cpu")):
        with pytest.raises(ValueError, match=word) as err:
            _args.check_tensor("x", bad, device=torch.device("cpu"), **kw)
        assert type(err.value) is ValueError
    # what a caller may leave open: the device, the shape, contiguity
    assert _args.check_tensor("x", torch.zeros(3, 4, 5, device="meta"), **kw).device.type == "meta"
    assert _args.check_tensor("x", torch.zeros(7), (torch.float32,), None, errors=errors).shape == (7,)
    strided = torch.zeros(3, 4, 10)[..., ::2]
    assert _args.check_tensor("x", strided, contiguous=False, **kw) is strided
    with pytest.raises(ValueError, match="x must be a tensor of dtype float32 or float64 and shape .3, 4, 5., got the shape"):
        _args.check_tensor("x", torch.zeros(3, 4, 6)[..., ::2], contiguous=False, **kw)


def test_episode_pitch():
    pitch = lambda t, inner=(3, 5): _args.episode_pitch("obs", t, inner)  # noqa: E731
    assert pitch(torch.zeros(4, 7, 3, 5)) == 7                                      # contiguous
    assert pitch(torch.zeros(4, 9, 3, 5)[:, :7]) == 9                               # a slice of longer episodes, read in place
    assert pitch(torch.zeros(1, 9, 3, 5)[:, :7]) == 7                               # B == 1: there is no batch stride to speak of
    assert pitch(torch.zeros(1, 7, 3, 5).as_strided((1, 7, 3, 5), (1, 15, 5, 1))) == 7
    assert pitch(torch.zeros(4, 7, 1, 5).as_strided((4, 7, 1, 5), (35, 5, 999, 1)), (1, 5)) == 7      # a size-1 inner dimension
    assert pitch(torch.zeros(4, 7, 3, 1).as_strided((4, 7, 3, 1), (21, 3, 1, 999)), (3, 1)) == 7
    assert pitch(torch.zeros(4, 2, 3, 5)[:, :1]) == 2 and pitch(torch.zeros(120).as_strided((4, 1, 3, 5), (30, 999, 5, 1))) == 2     # a single row
    assert _args.episode_pitch("reward", torch.zeros(4, 9)[:, :7], ()) == 9 and _args.episode_pitch("sel", torch.zeros(4, 8, 3)[:, :7], (3,)) == 8
    for what, bad, word in (("transposed", torch.zeros(7, 4, 3, 5).transpose(0, 1), "must be contiguous"),
                            ("row stride", torch.zeros(4, 7, 3, 10)[..., ::2], "must be contiguous"),
                            ("agent stride", torch.zeros(4, 7, 6, 5)[:, :, ::2], "must be contiguous"),
                            ("time stride", torch.zeros(4, 14, 3, 5)[:, ::2], "must be contiguous"),
                            ("batch stride not a multiple of a row", torch.zeros(4, 7 * 15 + 4)[:, :7 * 15].view(4, 7, 3, 5), "batch stride 109"),
                            ("overlapping episodes", torch.zeros(10, 3, 5).unfold(0, 7, 1).permute(0, 3, 1, 2), "batch stride 15 .* at least 105")):
        with pytest.raises(ValueError, match="obs: .*" + word):
            pitch(bad)
    with pytest.raises(ValueError, match="batch stride"):
        _args.episode_pitch("reward", torch.zeros(10).unfold(0, 7, 1), ())


def test_shared_pitch():
    q, a = torch.zeros(4, 8, 3, 6)[:, :7], torch.zeros(4, 8, 3, dtype=torch.int32)[:, :7]
    assert _args.shared_pitch("f: ", (("q", q, (3, 6)), ("a", a, (3,))), 7) == 8
    assert _args.shared_pitch("f: ", (("q", None, (3, 6)), ("a", a, (3,))), 7) == 8
    assert _args.shared_pitch("f: ", (("q", None, (3, 6)), ("a", None, (3,))), 7) == 7             # nothing given: dense
    with pytest.raises(ValueError, match="f: q, a must take the same number of rows per episode .8, 7."):
        _args.shared_pitch("f: ", (("q", q, (3, 6)), ("a", torch.zeros(4, 7, 3, dtype=torch.int32), (3,))), 7)
    one = (("q", torch.zeros(1, 8, 3, 6)[:, :7], (3, 6)), ("a", torch.zeros(1, 7, 3, dtype=torch.int32), (3,)))
    assert _args.shared_pitch("f: ", one, 7) == 7                                                   # B == 1: any two agree


def test_launch_error_classes():
    assert type(_args.launch_error(-30, "the launch failed")) is _lib.RobogymError
    assert type(_args.launch_error(-7, "refused")) is ValueError and "(-7) refused" in str(_args.launch_error(-7, "refused"))
    assert type(_args.launch_error(-7, "refused", refuses=False)) is _lib.RobogymError


# the two tuples as marbler_amd/_lib.py spelled them out before they were derived from ENTRIES
EXPORTS = ("rg_abi_version", "rg_last_error", "rg_sizeof_params", "rg_sizeof_state", "rg_sizeof_step_io", "rg_next_init_stride",
           "rg_create", "rg_destroy", "rg_bind_state", "rg_set_stream", "rg_reset", "rg_step", "rg_rollout", "rg_get_obs", "rg_step_kernel",
           "rg_actor_forward", "rg_actor_forward_explore", "rg_actor_pack_gru", "rg_actor_pack_gru_bf16x3", "rg_actor_pack_gru_f16x2", "rg_actor_last_error",
           "rg_sizeof_policy_io", "rg_policy_rollout", "rg_sizeof_lidar_params", "rg_set_lidar",
           "rg_sizeof_team_params", "rg_set_teams",
           "rg_actor_forward_sample", "rg_sizeof_policy_sample", "rg_policy_rollout_sample",
           "rg_sizeof_disturbance_params", "rg_set_disturbance", "rg_step_form", "rg_shape_match", "rg_shape_info",
           "rg_sizeof_render_params", "rg_render", "rg_render_last_error",
           "rg_sizeof_episode_buffer", "rg_sizeof_episode_stream", "rg_episodes_append", "rg_episodes_last_error",
           "rg_sizeof_actor_unroll_io", "rg_actor_unroll", "rg_actor_unroll_last_error",
           "rg_sizeof_mixer_weights", "rg_sizeof_td_targets_io", "rg_td_targets", "rg_td_targets_last_error")
LATE_QUERIES = ("rg_step_form", "rg_shape_match", "rg_shape_info", "rg_sizeof_render_params", "rg_render", "rg_render_last_error",
                "rg_sizeof_episode_buffer", "rg_sizeof_episode_stream", "rg_episodes_append", "rg_episodes_last_error",
                "rg_sizeof_actor_unroll_io", "rg_actor_unroll", "rg_actor_unroll_last_error",
                "rg_sizeof_mixer_weights", "rg_sizeof_td_targets_io", "rg_td_targets", "rg_td_targets_last_error")


def test_exports_and_late_queries_are_what_they_were():
    assert set(_lib.EXPORTS) == set(EXPORTS) and set(_lib.LATE_QUERIES) == set(LATE_QUERIES)
    assert _lib.EXPORTS == EXPORTS and _lib.LATE_QUERIES == LATE_QUERIES                 # tuples, in the same order
    assert len(set(EXPORTS)) == len(EXPORTS) and set(LATE_QUERIES) <= set(EXPORTS)
    # every sizeof query is checked against a struct, and only those are
    assert {q for q, _ in _lib.LAYOUTS} == {n for n in EXPORTS if n.startswith("rg_sizeof_")}
    assert len({s for _, s in _lib.LAYOUTS}) == len(_lib.LAYOUTS)


def test_group_units_and_side_blocks_come_from_their_tables():
    """The build's lane-group units are derived from csrc/kernel_args.h RG_GROUP_ENTRIES, the Python side blocks from
    params.SIDE_BLOCKS: every row of the first is defined by exactly one unit, whose flags are its mode's; the second names
    exactly the three rg_set_* entries of _lib.ENTRIES."""
    import os
    import re
    from marbler_amd import build, params
    rows = build.group_rows()
    assert len(rows) == 21 and len({r[0] for r in rows}) == 21
    assert {r[1] for r in rows} == {"GROUP_PLAIN", "GROUP_LIDAR", "GROUP_TEAM", "GROUP_DISTURB"} and {r[2] for r in rows} == {"RG_QP_EXACT", "RG_QP_CVXOPT"}
    by_entry = {r[0]: r for r in rows}
    slp, ilp, preload = ["-mllvm", "-slp-threshold=-60"], ["-mllvm", "-amdgpu-sched-strategy=max-ilp"], ["-mllvm", "-amdgpu-kernarg-preload-count=16"]
    units = build.units()
    assert len({name for name, _, _, _ in units}) == len(units)          # one object file per unit
    defined = []
    for name, src, flags, defines in units:
        if src == build.GROUP_UNIT:
            (d,) = defines
            assert d.startswith("RG_UNIT_ROWS=")
            mine = re.findall(r"X\((\w+),(\w+),(\w+),(\w+)\)", d)
            assert mine and "".join("X(%s,%s,%s,%s)" % m for m in mine) == d[len("RG_UNIT_ROWS="):]
            assert all(by_entry[m[0]] == m for m in mine)                 # the rows as the table has them
            # a family's single launches of one mode, or its rollout alone
            assert len({m[1:3] for m in mine}) == 1
            assert [m[3] for m in mine] in (["GROUP_STEP"], ["GROUP_STEP", "GROUP_OBS"], ["GROUP_ROLLOUT"])
            mine = [m[0] for m in mine]
        else:
            with open(os.path.join(build.CSRC, src)) as f:
                mine = [e for e in re.findall(r"^hipError_t (\w+)\(const KernelArgs &\w+, const GroupSide &", f.read(), re.M) if e in by_entry]
        defined += mine
        if mine:
            modes = {by_entry[e][2] for e in mine}
            assert len(modes) == 1, (name, modes)
            resident = {by_entry[e][3] for e in mine} <= {"GROUP_STEP_RESIDENT", "GROUP_STEP_SHAPE"}
            assert flags == slp + (ilp if modes == {"RG_QP_CVXOPT"} else []) + (preload if resident else []), (name, flags)
    assert sorted(defined) == sorted(by_entry)                            # every row once, by one unit
    # the four policy-rollout units: one source, the exact mode's lane-group flags
    policy = [(flags, sorted(defines)) for _, src, flags, defines in units if src == build.POLICY_UNIT]
    assert sorted(policy) == sorted((slp, sorted([f"RG_UNIT_H={h}", f"RG_UNIT_SAMPLE={s}"])) for h in (64, 128) for s in (0, 1))
    # every define and every source is part of what the rebuild check compares
    stamp = build.flags_stamp()
    assert all(d in stamp for _, _, _, defines in units for d in defines) and build.GROUP_UNIT in stamp and build.POLICY_UNIT in stamp
    # the side blocks
    setters = [n for n, _, _, _ in _lib.ENTRIES if n.startswith("rg_set_") and n != "rg_set_stream"]
    assert sorted(b.setter for b in params.SIDE_BLOCKS) == sorted(setters) and len(setters) == 3
    assert [(b.attr, b.setter, b.value_errors) for b in params.SIDE_BLOCKS] == [
        ("lidar", "rg_set_lidar", (-60, -50)), ("teams", "rg_set_teams", (-70, -60)), ("disturbance", "rg_set_disturbance", (-80, -70))]
    assert [b.read for b in params.SIDE_BLOCKS] == [params.lidar_params, params.team_pool, params.disturbance_params]
