#!/usr/bin/env python3
"""Driver of tools/ubench/sload.hip: ticks per `s_load_dword ; s_waitcnt lgkmcnt(0)` pair for one wave alone on a SIMD.  Build first:
   hipcc --offload-arch=gfx950 -O2 -shared -fPIC -o tools/ubench/libsload.so tools/ubench/sload.hip"""
import ctypes, os
import torch
lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsload.so"))
lib.run_sload.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
nbytes = lib.sload_buffer_bytes()
out = torch.zeros(64, device="cuda")
cyc = torch.zeros(1, dtype=torch.int64, device="cuda")
names = ["s_load_dword + wait, line in the scalar cache", "s_load_dword + wait, line first touched", "dependent v_fma_f32 (yardstick)"]
N = 16 * 16
for mode in range(3):
    ticks = []
    for _ in range(5):
        buf = torch.ones(nbytes // 4, dtype=torch.int32, device="cuda")   # a fresh buffer, written just before the launch
        torch.cuda.synchronize()
        assert lib.run_sload(mode, buf.data_ptr(), out.data_ptr(), cyc.data_ptr()) == 0
        torch.cuda.synchronize()
        ticks.append(int(cyc[0]))
    print(f"{names[mode]:48s} {N} in a row: ticks {ticks}  -> {min(ticks) / N:.1f} .. {max(ticks) / N:.1f} per unit", flush=True)
