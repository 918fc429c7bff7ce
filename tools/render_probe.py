"""Times VecRobotariumEnv.render() against the yardstick a raster cannot beat: writing its output once.

    python tools/render_probe.py [--out profiles/render_probe.txt] [--launches 200]

Per case (PredatorCapturePrey 4096 x 5 and Warehouse 4096 x 8, at 84 x 84 and 64 x 64): warm-up, then `launches` render calls
between two device events, device-complete, the median of several such windows; in the same run the same for `out.zero_()` (a
device memset of the same buffer), and for rg_render called straight through ctypes with a prepared argument block (what the
launch costs without render()'s Python).  Prints microseconds per call, GB/s of output bytes and the ratio to the memset.  The envs are
stepped first, so that the pictures are those of running episodes.  Needs the GPU: there is no host path to time.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("PredatorCapturePrey", {"predator": 3, "capture": 2, "n_agents": 5}, 5),
         ("Warehouse", {"n_agents": 8}, 5))
SIZES = (84, 64)
E = 4096


def _window(fn, launches):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / launches     # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    import ctypes as C

    import torch
    from marbler_amd import VecRobotariumEnv, _lib
    lines = [f"render_probe: {E} envs, {args.launches} launches per window, median of {args.windows} windows, "
             f"{torch.cuda.get_device_name(0)}",
             f"{'case':<34}{'render us':>11}{'GB/s':>9}{'memset us':>11}{'GB/s':>9}{'ratio':>8}{'rg_render us':>14}{'ratio':>8}"]
    for scenario, ov, n_act in CASES:
        env = VecRobotariumEnv(scenario, E, overrides=ov, seed=1)
        env.reset()
        g = torch.Generator(device="cpu").manual_seed(0)
        for _ in range(10):
            env.step(torch.randint(0, n_act, (E, env.N), generator=g, dtype=torch.int32).to(env.device))
        for size in SIZES:
            out = torch.empty((E, size, size, 3), dtype=torch.uint8, device=env.device)
            nbytes = out.numel()
            render = lambda: env.render(size=size, out=out)   # noqa: E731
            memset = lambda: out.zero_()                      # noqa: E731
            rp = _lib.RgRenderParams(size, size, E, 0, None, 0.0, 0.0, 0.0, 0.0)
            call = (C.byref(env.params), C.byref(env._state), E, C.byref(rp), out.data_ptr(),
                    C.c_void_p(torch.cuda.current_stream(env.device).cuda_stream))
            raw = lambda: env.lib.rg_render(*call)            # noqa: E731
            for fn in (render, memset, raw):
                _window(fn, 20)                               # warm-up
            # alternate the two, so that a clock or a neighbour's load hits both alike
            tr, tm, tw = [], [], []
            for _ in range(args.windows):
                tr.append(_window(render, args.launches))
                tm.append(_window(memset, args.launches))
                tw.append(_window(raw, args.launches))
            r, m, w = (sorted(t)[len(t) // 2] for t in (tr, tm, tw))
            lines.append(f"{scenario + ' ' + str(E) + ' x ' + str(env.N) + ', ' + str(size) + ' x ' + str(size):<34}"
                         f"{r:>11.1f}{nbytes / r / 1e3:>9.0f}{m:>11.1f}{nbytes / m / 1e3:>9.0f}{r / m:>8.2f}{w:>14.1f}{w / m:>8.2f}")
        env.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
