// What is a step launch's FIRST link worth -- the trip to the kernel-argument segment in front of the first load of state -- and
// what would a device-resident argument block and preloaded leading arguments take out of it (diagnostic, not shipped)?
// One wave per SIMD (1024 x 64 lanes, the headline launch's shape), host-launched back to back.  Every wave stamps s_memtime at its
// entry and when its first words of "state" have arrived, then runs a dependent chain of ~10 us, so that the launch is GPU-bound
// and the host's time per launch sees whatever the ticks cannot (see below).  Three argument shapes:
//   1  by value:  the 0.8 KB block as the kernel's argument, the state pointers inside it (what rg_step does)
//   2  resident:  a pointer to a device-resident copy of the block in ordinary kernargs, the block read through the constant
//                 address space
//   3  window:    the same, with the image pointer, the state pointers and what the env index is computed from as leading plain
//                 arguments -- the ones -mllvm -amdgpu-kernarg-preload-count=N lets the command processor hand over in SGPRs
// Built twice from this one file (tools/ubench/resident_args.py): plain, and with the preload flag.  Only leading plain arguments
// are preloaded, so the flag changes shapes 2 and 3 (their descriptors then carry a preload length) and leaves shape 1 alone.
// CAVEAT of the ticks: a kernel compiled for preloading has two entries.  Firmware that preloads enters 256 bytes in; any other
// runs the compatibility prologue (the same dwords by s_load, a wait, a branch) BEFORE the code that stamps the entry, so there the
// ticks of a preload build leave the kernarg trip out although the wave paid it.  The host's us per launch judge; ticks explain.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

struct Block {                 // the size and the mix of rg::KernelArgs: pointers, ints, floats (792 bytes)
    const float *state[4];     // first wave of loads
    const float *late[8];      // read after the first wave of loads
    float *out;
    long long *ticks;
    int E, envs_per_wave, n[38];
    float k[134];
};
static_assert(sizeof(Block) >= 780 && sizeof(Block) <= 832, "about the 0.8 KB of KernelArgs");

constexpr int WAVES = 1024, LANES = 64, CHAIN = 2500;
typedef const __attribute__((address_space(4))) Block *ConstBlock;

template <bool FENCE>   // FENCE: no load moves across the stamp
__device__ __forceinline__ long long stamp() {
    long long t;
    if constexpr (FENCE) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    else asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t));
    return t;
}

// the part every shape shares: first loads through `s0..s3` at the env index, stamp, then the block's other fields and the chain
template <typename B>
__device__ __forceinline__ void body(long long t0, const float *s0, const float *s1, const float *s2, const float *s3, int E, int envs_per_wave,
                                     int grid, B blk) {
    const int lane = threadIdx.x, i = blockIdx.x * LANES + lane;
    const int slot = envs_per_wave == 4 ? lane >> 4 : envs_per_wave == 2 ? lane >> 5 : 0;
    const int e = min((static_cast<int>(blockIdx.x) + slot * grid) * 16 + (lane & 15), E * 16 - 1);   // 16 words per env, in bounds whatever the arguments
    // the block's other fields are requested with the first loads (the step kernels fetch all their arguments together), and
    // nothing waits for them before the state is on its way: the second stamp is no fence
    const float *late3 = blk->late[3];
    const float n7 = static_cast<float>(blk->n[7]), k100 = blk->k[100], m = blk->k[5], c = blk->k[77];
    float v = s0[e] + s1[e] + s2[e] + s3[e];
    asm volatile("" : "+v"(v));   // the words have arrived
    const long long t1 = stamp<false>();
    v += late3[lane] * n7 + k100;
    for (int k = 0; k < CHAIN; ++k) v = v * m + c;
    blk->out[i] = v;
    if (lane == 0) blk->ticks[blockIdx.x] = t1 - t0;
}

extern "C" __global__ __launch_bounds__(64) void shape1_by_value(Block b) {
    const long long t0 = stamp<true>();
    body(t0, b.state[0], b.state[1], b.state[2], b.state[3], b.E, b.envs_per_wave, gridDim.x, &b);
}
// The image is never written while a launch can read it, so it may be read through the constant address space: the compiler then
// keeps s_load for its uniform fields, as it does for kernargs.
extern "C" __global__ __launch_bounds__(64) void shape2_resident(const Block *img) {
    const long long t0 = stamp<true>();
    ConstBlock b = (ConstBlock)img;
    body(t0, b->state[0], b->state[1], b->state[2], b->state[3], b->E, b->envs_per_wave, gridDim.x, b);
}
extern "C" __global__ __launch_bounds__(64) void shape3_window(const Block *img, const float *s0, const float *s1, const float *s2, const float *s3,
                                                               int E, int envs_per_wave, int grid) {
    const long long t0 = stamp<true>();
    body(t0, s0, s1, s2, s3, E, envs_per_wave, grid, (ConstBlock)img);
}

#define CHECK(x)                                                                 \
    do {                                                                         \
        hipError_t err_ = (x);                                                   \
        if (err_ != hipSuccess) {                                                \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(err_));            \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

int main(int argc, char **argv) {
    const char *tag = argc > 1 ? argv[1] : "build";
    const int n = WAVES * LANES, reps = 3000, rounds = argc > 2 ? atoi(argv[2]) : 3;
    float *state, *late, *out;
    long long *ticks;
    Block *img;
    CHECK(hipMalloc(&state, 4 * n * sizeof(float)));
    CHECK(hipMalloc(&late, 4096));
    CHECK(hipMalloc(&out, n * sizeof(float)));
    CHECK(hipMalloc(&ticks, WAVES * sizeof(long long)));
    CHECK(hipMalloc(&img, sizeof(Block)));
    CHECK(hipMemset(state, 0, 4 * n * sizeof(float)));
    CHECK(hipMemset(late, 0, 4096));
    Block b;
    memset(&b, 0, sizeof b);
    for (int j = 0; j < 4; ++j) b.state[j] = state + j * n;
    for (auto &p : b.late) p = late;
    b.out = out, b.ticks = ticks, b.E = 4096, b.envs_per_wave = 4;
    for (auto &x : b.n) x = 1;
    for (auto &x : b.k) x = 0.5f;
    b.k[5] = 1.0001f;
    CHECK(hipMemcpy(img, &b, sizeof b, hipMemcpyHostToDevice));
    CHECK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::vector<long long> h(WAVES);
    auto launch = [&](int shape) {
        if (shape == 1) hipLaunchKernelGGL(shape1_by_value, dim3(WAVES), dim3(LANES), 0, 0, b);
        else if (shape == 2) hipLaunchKernelGGL(shape2_resident, dim3(WAVES), dim3(LANES), 0, 0, img);
        else hipLaunchKernelGGL(shape3_window, dim3(WAVES), dim3(LANES), 0, 0, img, b.state[0], b.state[1], b.state[2], b.state[3], b.E, b.envs_per_wave, WAVES);
    };
    for (int round = 0; round < rounds; ++round)
        for (int shape = 1; shape <= 3; ++shape) {   // the shapes alternate inside a process, the builds outside it
            for (int i = 0; i < 200; ++i) launch(shape);
            CHECK(hipEventRecord(e0, 0));
            for (int i = 0; i < reps; ++i) launch(shape);
            CHECK(hipEventRecord(e1, 0));
            CHECK(hipEventSynchronize(e1));
            CHECK(hipGetLastError());
            float ms;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            CHECK(hipMemcpy(h.data(), ticks, WAVES * sizeof(long long), hipMemcpyDeviceToHost));   // the last launch's waves
            std::sort(h.begin(), h.end());
            double mean = 0;
            for (long long t : h) mean += static_cast<double>(t) / WAVES;
            printf("%-8s shape %d: %7.3f us per launch; entry -> first state words, ticks over %d waves: min %lld median %lld mean %.0f max %lld\n", tag,
                   shape, ms * 1e3 / reps, WAVES, h[0], h[WAVES / 2], mean, h[WAVES - 1]);
            fflush(stdout);
        }
    return 0;
}
