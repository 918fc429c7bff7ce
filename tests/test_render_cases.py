"""Rendering without a GPU: the float64 twin on hand-placed states with known answers, the degenerate share of the cases the GPU
tier renders, every refusal of rg_render's host half (host pointers that are never dereferenced), the binding, and the Python
argument errors that are decided before a device is touched.  The picture: csrc/render.h (it replaces what
scenarios/*/visualize.py draws through utilities/roboEnv.py:67-76 of the reference)."""
import ctypes
import math

import numpy as np
import pytest

import render_cases as rc
from render_twin import EDGE_TOL, PALETTE, count, render_twin


def _params(scenario, ov=None):
    from marbler_amd import load_config, make_params
    return make_params(scenario, load_config(scenario, None, ov))


def _far(n):
    """poses [3, n] far outside every view"""
    p = np.zeros((3, n))
    p[0] = 50.0 + np.arange(n)
    p[1] = 50.0
    return p


# ---------------------------------------------------------------- the twin on known answers
def test_twin_one_robot_at_the_origin_facing_east():
    p = _params("Simple")
    n = int(p.n_agents)
    poses = _far(n)
    poses[:, 0] = 0.0                                   # robot 0: origin, theta 0
    state = {"poses": poses, "prey_loc": np.array([[50.0, 50.0]]), "prey_sensed": [0], "prey_captured": [0]}
    W = H = 101                                         # the twin takes any width: an odd one puts a pixel centre ON the origin
    view = (-0.505, -0.505, 1.01, 1.01)                 # 1 cm pixels
    frame, deg = render_twin(p, state, W, H, view=view, layers=("arena", "robots"))
    assert tuple(frame[50, 50]) == PALETTE["class0"]
    r_px = float(p.robot_diameter) / 2 / 0.01
    assert abs(count(frame, "class0") - math.pi * r_px ** 2) < 2 * math.pi * r_px      # the disk's area, to within its rim
    frame, deg = render_twin(p, state, W, H, view=view)
    assert tuple(frame[50, 51]) == PALETTE["heading"]                                  # the segment leaves the centre to the right
    assert tuple(frame[50, 50 + int(r_px)]) == PALETTE["heading"]                      # ... and reaches the rim, one radius away
    assert tuple(frame[50, 50 - 2]) == PALETTE["class0"] and tuple(frame[50 - 3, 50]) == PALETTE["class0"]
    assert tuple(frame[50, 50 + int(r_px) + 2]) == PALETTE["background"]
    assert tuple(frame[0, 0]) == PALETTE["background"] and count(frame, "surround") == 0
    assert not deg[50, 50 - 2] and not deg[0, 0]                                       # no edge within 1e-4 m of these centres


def test_twin_prey_flags():
    p = _params("PredatorCapturePrey")
    n, P = int(p.n_agents), int(p.num_prey)
    loc = np.full((P, 2), 50.0)
    loc[0] = (0.2, 0.1)
    state = {"poses": _far(n), "prey_loc": loc, "prey_sensed": np.zeros(P, np.uint8), "prey_captured": np.zeros(P, np.uint8)}
    view = (-0.3, -0.4, 1.0, 1.0)
    free, _ = render_twin(p, state, 200, 200, view=view)
    area = math.pi * (0.025 / 0.005) ** 2
    assert abs(count(free, "prey") - area) < 0.25 * area and count(free, "prey_sensed") == 0
    state["prey_sensed"][0] = 1
    sensed, _ = render_twin(p, state, 200, 200, view=view)
    assert count(sensed, "prey") == 0 and count(sensed, "prey_sensed") == count(free, "prey")
    assert np.array_equal((sensed != free).any(-1), (free == np.asarray(PALETTE["prey"], np.uint8)).all(-1))
    state["prey_captured"][0] = 1
    gone, _ = render_twin(p, state, 200, 200, view=view)
    assert count(gone, "prey") == 0 and count(gone, "prey_sensed") == 0


def test_twin_arctic_cells_colour_exactly_their_squares():
    p = _params("ArcticTransport")
    grid = np.zeros((8, 12), np.uint8)
    grid[2, 3], grid[5, 7], grid[0, 11] = 1, 2, 3
    state = {"poses": _far(4), "grid": grid.reshape(-1)}
    H, W = 160, 240                                     # the view below: 1.25 cm pixels, 20 x 20 of them per cell, none on the lattice
    view = (-1.5, -1.0, 3.0, 2.0)
    frame, deg = render_twin(p, state, W, H, view=view, layers=("arena", "zones"))
    for (i, j), colour in (((2, 3), "ice"), ((5, 7), "water"), ((0, 11), "goal")):
        want = np.zeros((H, W), bool)
        want[20 * i:20 * i + 20, 20 * j:20 * j + 20] = True
        assert np.array_equal((frame == np.asarray(PALETTE[colour], np.uint8)).all(-1), want), colour
    assert count(frame, "background") == H * W - 3 * 400 and not deg.any()


def test_palettes_agree_and_are_distinct():
    from marbler_amd import render
    assert render.PALETTE == PALETTE and len(set(PALETTE.values())) == len(PALETTE)
    text = open(render.__file__.replace("render.py", "csrc/render.h")).read()
    body = text.split("#define RG_RENDER_PALETTE")[1].split("\n\n")[0]
    import re
    triples = [tuple(int(v) for v in m) for m in re.findall(r"\{(\d+), (\d+), (\d+)\}", body)]
    assert triples == list(PALETTE.values())            # index order of the enum = the dict's order


# ---------------------------------------------------------------- the degenerate share of the GPU tier's hand-made cases
@pytest.mark.parametrize("case", list(rc.all_cases()), ids=lambda c: c[0])
def test_degenerate_share_of_the_shared_cases(case):
    """About 20 m of edges x 2e-4 m over 6.4 m^2 is 0.06 % at any resolution; the cap of 0.5 % keeps the comparison from excusing a
    real error.  Over the frames of the case."""
    name, _, scenario, ov, shape, E, envs, (H, W), view = case
    p = _params(scenario, ov)
    state = rc.synthetic_state(p, E, seed=len(name))
    envs = list(range(E)) if envs is None else envs
    v = rc.case_view(scenario, shape, view, state["poses"][envs[0]])
    deg = np.stack([render_twin(p, rc.env_state(state, e), W, H, view=v)[1] for e in envs])
    print(name, "degenerate share %.4f %%" % (100 * deg.mean()))
    assert deg.mean() <= rc.MAX_DEGENERATE_SHARE, (name, deg.mean())
    assert EDGE_TOL == 1e-4


# ---------------------------------------------------------------- the host half of rg_render
def _call(lib, p=None, st=None, E=4, rgb=0x1000, **rp_fields):
    from marbler_amd import _lib
    p = _params("PredatorCapturePrey") if p is None else p
    if st is None:
        st = _lib.RgState()
        st.poses, st.prey_loc, st.prey_sensed, st.prey_captured, st.grid = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    rp = _lib.RgRenderParams(48, 32, 2, 0, None, 0.0, 0.0, 0.0, 0.0)
    for k, v in rp_fields.items():
        setattr(rp, k, v)
    return lib.rg_render(ctypes.byref(p), ctypes.byref(st), E, ctypes.byref(rp), ctypes.c_void_p(rgb), None)


def test_rg_render_is_exported_and_its_struct_matches():
    from marbler_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "rg_render") and hasattr(lib, "rg_render_last_error") and hasattr(lib, "rg_sizeof_render_params")
    assert {"rg_render", "rg_render_last_error", "rg_sizeof_render_params"} <= set(_lib.EXPORTS)
    assert lib.rg_sizeof_render_params() == ctypes.sizeof(_lib.RgRenderParams) == 40
    assert lib.rg_abi_version() == 7


def test_rg_render_refuses_every_bad_argument_before_touching_a_device():
    from marbler_amd import _lib
    lib = _lib.load()
    nan, inf = float("nan"), float("inf")
    seen = {}

    def refused(word, rc_, what):
        msg = lib.rg_render_last_error()
        assert rc_ < 0 and rc_ != -30, (what, rc_)
        assert word in msg, (what, rc_, msg)
        assert seen.setdefault(rc_, word) == word, (what, rc_, "one code, two meanings")

    p = _params("PredatorCapturePrey")
    st = _lib.RgState()
    rp = _lib.RgRenderParams(48, 32, 2, 0, None, 0.0, 0.0, 0.0, 0.0)
    refused(b"params", lib.rg_render(None, ctypes.byref(st), 4, ctypes.byref(rp), ctypes.c_void_p(0x1000), None), "params NULL")
    refused(b"state", lib.rg_render(ctypes.byref(p), None, 4, ctypes.byref(rp), ctypes.c_void_p(0x1000), None), "state NULL")
    refused(b"rp", lib.rg_render(ctypes.byref(p), ctypes.byref(st), 4, None, ctypes.c_void_p(0x1000), None), "rp NULL")
    refused(b"rgb is NULL", _call(lib, rgb=0), "rgb NULL")
    refused(b"rgb must be 4-byte aligned", _call(lib, rgb=0x1002), "rgb alignment")
    for value in (7, 0, -4, 1028):
        refused(b"width outside", _call(lib, width=value), ("width", value))
    for value in (10, 50, 1022):
        refused(b"width must be a multiple of 4", _call(lib, width=value), ("width", value))
    for value in (7, 0, -1, 1025):
        refused(b"height outside", _call(lib, height=value), ("height", value))
    for value in (0, -3):
        refused(b"n_frames must be", _call(lib, n_frames=value), ("n_frames", value))
    refused(b"n_frames: more than", _call(lib, n_frames=2 ** 31 - 1, width=1024, height=1024, env_index=0x6000), "grid limit")
    for value in (64, -1, 1 << 20):
        refused(b"layers", _call(lib, layers=value), ("layers", value))
    refused(b"env_index is NULL", _call(lib, n_frames=5, E=4), "K > E without env_index")
    assert _call(lib, n_frames=5, E=4, env_index=0x6000, width=6) < 0          # (with an index list K > E is no refusal by itself)
    assert b"width" in lib.rg_render_last_error()
    refused(b"num_envs", _call(lib, E=0), "num_envs")
    for field in ("view_x0", "view_y0"):
        for value in (nan, inf, -inf, 1001.0, -2000.0):
            refused(b"view_x0 / view_y0", _call(lib, view_w=1.0, view_h=1.0, **{field: value}), (field, value))
    for value in (nan, inf, -1.0, 1001.0):
        refused(b"view_w", _call(lib, view_w=value, view_h=1.0), ("view_w", value))
        refused(b"view_h must be finite, not negative", _call(lib, view_w=1.0, view_h=value), ("view_h", value))
    refused(b"view_h must be positive", _call(lib, view_w=1.0, view_h=0.0), "view_h 0 with view_w")
    # the state arrays the scenario's picture needs
    st = _lib.RgState()
    refused(b"state.poses", _call(lib, st=st), "poses NULL")
    for scenario in ("PredatorCapturePrey", "Simple"):
        for missing in ("prey_loc", "prey_sensed", "prey_captured"):
            st = _lib.RgState()
            st.poses, st.prey_loc, st.prey_sensed, st.prey_captured = 0x1000, 0x2000, 0x3000, 0x4000
            setattr(st, missing, None)
            refused(b"prey", _call(lib, p=_params(scenario), st=st), (scenario, missing))
    st = _lib.RgState()
    st.poses = 0x1000
    refused(b"state.grid", _call(lib, p=_params("ArcticTransport"), st=st), "grid NULL")
    # the fields of the parameter block the picture reads
    for field, value, word in (("scenario", 9, b"scenario"), ("scenario", -1, b"scenario"), ("n_agents", 0, b"n_agents"),
                               ("n_agents", 17, b"n_agents"), ("num_prey", 0, b"num_prey"), ("num_prey", 65, b"num_prey"),
                               ("bound_w", 0.0, b"bound_x0 / bound_y0 / bound_w / bound_h"), ("bound_h", nan, b"bound_x0 / bound_y0 / bound_w / bound_h"),
                               ("bound_x0", inf, b"bound_x0 / bound_y0 / bound_w / bound_h"),
                               ("bound_y0", -1500.0, b"bound_x0 / bound_y0 / bound_w / bound_h"),
                               ("bound_w", 1200.0, b"bound_x0 / bound_y0 / bound_w / bound_h"),
                               ("robot_diameter", 0.0, b"robot_diameter"), ("robot_diameter", nan, b"robot_diameter")):
        q = _params("PredatorCapturePrey")
        setattr(q, field, value)
        refused(word, _call(lib, p=q), (field, value))
    assert len(seen) >= 20


# ---------------------------------------------------------------- Python argument errors that need no device
def test_size_layers_view_and_out_are_checked_on_the_host():
    import torch
    from marbler_amd import render
    assert render.parse_size(84) == (84, 84) and render.parse_size((32, 48)) == (32, 48)
    for bad in (7, 1025, (32, 50), (4, 48), (32, 2048), 0, -84):
        with pytest.raises(ValueError):
            render.parse_size(bad)
    for bad in (84.0, "84", (32,), (32, 48, 3), None, True, (32.0, 48)):
        with pytest.raises(TypeError):
            render.parse_size(bad)
    assert tuple(render.LAYERS) == ("arena", "zones", "markers", "rings", "robots", "heading")
    assert render.layer_mask(None) == 63 and render.layer_mask(["robots", "heading"]) == 48 and render.layer_mask("rings") == 8
    assert render.layer_mask(None, default=63 & ~8) == 55
    for bad in (["robot"], ["arena", "text"], [], "all"):
        with pytest.raises(ValueError):
            render.layer_mask(bad)
    assert render.parse_view(None) == (0.0, 0.0, 0.0, 0.0) and render.parse_view((-1, -1, 2, 2.5)) == (-1.0, -1.0, 2.0, 2.5)
    for bad in ((0, 0, 0, 1), (0, 0, 1, -1), (float("nan"), 0, 1, 1), (0, 0, float("inf"), 1)):
        with pytest.raises(ValueError):
            render.parse_view(bad)
    with pytest.raises(TypeError):
        render.parse_view((0, 0, 1))
    good = torch.zeros(3, 32, 48, 3, dtype=torch.uint8)
    assert render.check_out(good, (3, 32, 48, 3)) is good
    with pytest.raises(ValueError):
        render.check_out(good, (2, 32, 48, 3))
    with pytest.raises(ValueError):
        render.check_out(torch.zeros(3, 32, 48, 4, dtype=torch.uint8), (3, 32, 48, 3))
    with pytest.raises(TypeError):
        render.check_out(torch.zeros(3, 32, 48, 3, dtype=torch.int8), (3, 32, 48, 3))
    with pytest.raises(TypeError):
        render.check_out(np.zeros((3, 32, 48, 3), np.uint8), (3, 32, 48, 3))
    with pytest.raises(ValueError):
        render.check_out(torch.zeros(3, 32, 48, 6, dtype=torch.uint8)[..., :3], (3, 32, 48, 3))       # not contiguous
    with pytest.raises(IndexError):
        render.env_indices([0, 5], 5, torch.device("cpu"))
    with pytest.raises(IndexError):
        render.env_indices(-1, 5, torch.device("cpu"))
    with pytest.raises(IndexError):
        render.env_indices(torch.tensor([1, 7]), 5, torch.device("cpu"))
    k, idx = render.env_indices([4, 0, 2], 5, torch.device("cpu"))
    assert k == 3 and idx.dtype == torch.int32 and idx.tolist() == [4, 0, 2]
    assert render.env_indices(None, 5, torch.device("cpu")) == (5, None)
