"""Rendering: batched RGB frames of the envs' state from one HIP launch (rg_render, include/robogym.h).

    frames = env.render()                                   # uint8 [E, 84, 84, 3] on the env's device
    frames = env.render(envs=[1337], size=(256, 384))       # one env, larger
    clip = record(env, actions)                             # uint8 [T + 1, E, 84, 84, 3]: the trajectory a GIF is made of

What is drawn -- the arena, the scenario's zones or terrain, prey / goal markers, PredatorCapturePrey's capability rings, the
robots in their class colour and their headings, the roles of the reference's visualisers (scenarios/*/visualize.py) -- is
stated once in csrc/render.h and DESIGN.md section 4 "Render".  There is no host path: the frames are rasterised on the GPU from
the state it already holds.
"""
import ctypes as C

import torch

from . import _args, _lib

# layer names, in draw order -> bits of rg_render_params.layers
LAYERS = {"arena": _lib.RENDER_ARENA, "zones": _lib.RENDER_ZONES, "markers": _lib.RENDER_MARKERS, "rings": _lib.RENDER_RINGS,
          "robots": _lib.RENDER_ROBOTS, "heading": _lib.RENDER_HEADING}
ALL_LAYERS = sum(LAYERS.values())

# the palette of csrc/render.h (RG_RENDER_PALETTE), name -> (R, G, B); every colour is distinct
PALETTE = {"background": (255, 255, 255), "surround": (224, 224, 224), "zone_a": (255, 221, 128), "zone_b": (170, 238, 153),
           "ice": (190, 230, 255), "water": (70, 130, 220), "goal": (120, 200, 120), "prey": (0, 170, 90),
           "prey_sensed": (170, 60, 200), "zone1": (230, 130, 40), "class0": (220, 40, 40), "class1": (40, 90, 220),
           "class2": (240, 190, 20), "heading": (30, 30, 30)}

MIN_SIZE, MAX_SIZE = 8, 1024


def parse_size(size):
    """size: an int (square) or (H, W) -> (H, W); both in 8..1024, W a multiple of 4 (a lane stores 4 pixels as three dwords)."""
    if isinstance(size, bool):
        raise TypeError("size must be an int or (H, W)")
    if isinstance(size, int):
        h = w = size
    else:
        try:
            h, w = size
        except (TypeError, ValueError):
            raise TypeError(f"size must be an int or (H, W), got {size!r}") from None
        if not (isinstance(h, int) and isinstance(w, int)) or isinstance(h, bool) or isinstance(w, bool):
            raise TypeError(f"size must be an int or (H, W) of ints, got {size!r}")
    if not (MIN_SIZE <= h <= MAX_SIZE and MIN_SIZE <= w <= MAX_SIZE):
        raise ValueError(f"size {size!r}: height and width must lie in {MIN_SIZE}..{MAX_SIZE}")
    if w % 4:
        raise ValueError(f"size {size!r}: the width must be a multiple of 4")
    return h, w


def layer_mask(layers, default=ALL_LAYERS):
    """layers: None (-> default) or names from LAYERS -> the bit mask."""
    if layers is None:
        return default
    if isinstance(layers, str):
        layers = (layers,)
    mask = 0
    for name in layers:
        if name not in LAYERS:
            raise ValueError(f"unknown layer {name!r} (have {list(LAYERS)})")
        mask |= LAYERS[name]
    if mask == 0:
        raise ValueError("layers is empty: name at least one of " + ", ".join(LAYERS))
    return mask


def parse_view(view):
    """view: None (the arena) or (x0, y0, w, h), the world rectangle the image shows."""
    if view is None:
        return 0.0, 0.0, 0.0, 0.0
    try:
        x0, y0, w, h = (float(v) for v in view)
    except (TypeError, ValueError):
        raise TypeError(f"view must be None or (x0, y0, w, h), got {view!r}") from None
    if not all(abs(v) <= 1000.0 for v in (x0, y0, w, h)) or w <= 0.0 or h <= 0.0:
        raise ValueError(f"view {view!r}: x0, y0 within 1000 m of the origin, w and h positive and at most 1000 m")
    return x0, y0, w, h


def check_out(out, shape, device=None):
    """out: the caller's frame tensor -- uint8, contiguous, of `shape` [K, H, W, 3] (on `device`, 4-byte aligned)."""
    _args.check_tensor("out", out, (torch.uint8,), shape, device, errors=(TypeError, TypeError))
    if out.data_ptr() % 4:
        raise ValueError("out must be 4-byte aligned")
    return out


def env_indices(envs, num_envs, device):
    """envs: None (all), an int, a sequence or an int tensor -> (K, int32 device tensor or None).  Host data is range-checked
    here (IndexError); a device tensor is taken as it is (rg_render draws an index outside [0, E) without the env's shapes)."""
    if envs is None:
        return num_envs, None
    if isinstance(envs, torch.Tensor) and envs.device.type != "cpu":
        if envs.dtype in (torch.float16, torch.float32, torch.float64, torch.bfloat16, torch.bool):
            raise TypeError(f"envs must be an int tensor, got {envs.dtype}")
        idx = envs.reshape(-1).to(device=device, dtype=torch.int32).contiguous()
    else:
        if isinstance(envs, torch.Tensor):
            if envs.dtype in (torch.float16, torch.float32, torch.float64, torch.bfloat16, torch.bool):
                raise TypeError(f"envs must be an int tensor, got {envs.dtype}")
            host = [int(v) for v in envs.reshape(-1).tolist()]
        elif isinstance(envs, int) and not isinstance(envs, bool):
            host = [envs]
        else:
            host = [int(v) for v in envs]
        bad = [v for v in host if not 0 <= v < num_envs]
        if bad:
            raise IndexError(f"envs: {bad[:4]} outside [0, {num_envs})")
        idx = torch.tensor(host, dtype=torch.int32).to(device)
    if idx.numel() < 1:
        raise ValueError("envs is empty")
    return int(idx.numel()), idx


def render_frames(env, envs=None, size=84, out=None, layers=None, view=None):
    """VecRobotariumEnv.render (see there)."""
    h, w = parse_size(size)
    # with a team pool the rings would show the config's radii, not the episode's: dropped unless asked for by name
    mask = layer_mask(layers, ALL_LAYERS & ~LAYERS["rings"] if env.teams is not None else ALL_LAYERS)
    vx, vy, vw, vh = parse_view(view)
    k, idx = env_indices(envs, env.E, env.device)
    if out is not None:
        check_out(out, (k, h, w, 3), env.device)
    with torch.cuda.device(env.device):
        if out is None:
            out = torch.empty((k, h, w, 3), dtype=torch.uint8, device=env.device)
        rp = _lib.RgRenderParams(w, h, k, mask, idx.data_ptr() if idx is not None else None, vx, vy, vw, vh)
        rc = env.lib.rg_render(C.byref(env.params), C.byref(env._state), env.E, C.byref(rp), out.data_ptr(),
                               _args.launch_stream(None, env.device)[1])
    if rc != 0:
        raise _args.launch_error(rc, "rg_render: " + env.lib.rg_render_last_error().decode(), refuses=False)
    return out


def record(env, actions, size=84, envs=None):
    """Render, then step and render once per row of `actions` [T, E, N] (int, on the env's device): uint8
    [T + 1, K, H, W, 3], frame 0 the state before the first step."""
    h, w = parse_size(size)
    k, idx = env_indices(envs, env.E, env.device)
    steps = int(actions.shape[0])
    frames = torch.empty((steps + 1, k, h, w, 3), dtype=torch.uint8, device=env.device)
    render_frames(env, envs=idx, size=(h, w), out=frames[0])
    for t in range(steps):
        env.step(actions[t])
        render_frames(env, envs=idx, size=(h, w), out=frames[t + 1])
    return frames
