// What does a scalar load cost a LONE wavefront when its result is waited for at once (diagnostic, not shipped)?
// The step kernels' argument reloads have this shape: `s_load_dword ; s_waitcnt lgkmcnt(0)` right in front of the instruction
// that needs the value.  One wave on a SIMD, each load-wait pair in one asm block, timed with s_memtime:
//   MODE 0: every load from the SAME dword (after the first: a line that is in the scalar cache)
//   MODE 1: every load from a line this launch has not touched yet (256 bytes on: past the 64-byte scalar-cache line and the
//           128-byte L2 line), the buffer written by the host-side fill just before the launch
//   MODE 2: the dependent v_fma_f32 chain of issue.hip, as the yardstick of one dependent VALU instruction
// Driver: tools/ubench/sload.py.
#include <hip/hip_runtime.h>

constexpr int REP = 16;       // loop trips; 16 load-wait pairs per trip
constexpr int STRIDE = 256;   // bytes between two first-touch loads
extern "C" int sload_buffer_bytes() { return REP * 16 * STRIDE; }

#define X4(a) a a a a
#define X16(a) X4(a) X4(a) X4(a) X4(a)

template <int MODE>
__global__ void bench(const int *buf, float *out, long long *cyc) {
    int acc = 0, v = 0, off = 0;
    float a0 = threadIdx.x * 1e-3f;
    const float m = 0.999f, c = 1e-3f;
    if constexpr (MODE == 0) asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(v) : "s"(buf));   // warm the line
    const long long t0 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)");
    for (int i = 0; i < REP; ++i) {
        if constexpr (MODE == 0)
            asm volatile(X16("s_load_dword %0, %2, 0x0\n\ts_waitcnt lgkmcnt(0)\n\ts_add_u32 %1, %1, %0\n\t") : "=&s"(v), "+s"(acc) : "s"(buf));
        else if constexpr (MODE == 1)   // (the last load of the last trip reads byte REP * 16 * STRIDE - STRIDE: inside the buffer)
            asm volatile(X16("s_load_dword %0, %3, %2\n\ts_waitcnt lgkmcnt(0)\n\ts_add_u32 %1, %1, %0\n\ts_add_u32 %2, %2, 0x100\n\t")
                         : "=&s"(v), "+s"(acc), "+s"(off) : "s"(buf));
        else
            asm volatile(X16("v_fma_f32 %0, %0, %1, %2\n\t") : "+v"(a0) : "v"(m), "v"(c));
    }
    const long long t1 = __builtin_amdgcn_s_memtime();
    out[threadIdx.x] = a0 + static_cast<float>(acc);
    if (threadIdx.x == 0) cyc[0] = t1 - t0;
}
static_assert(STRIDE == 0x100, "the asm's increment");

extern "C" int run_sload(int mode, const int *buf, float *out, long long *cyc) {
    switch (mode) {
        case 0: bench<0><<<1, 64>>>(buf, out, cyc); break;
        case 1: bench<1><<<1, 64>>>(buf, out, cyc); break;
        case 2: bench<2><<<1, 64>>>(buf, out, cyc); break;
        default: return -1;
    }
    return (int)hipGetLastError();
}
