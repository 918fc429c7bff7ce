// actor_unroll.h -- the rule of rg_actor_unroll (include/robogym.h), stated once, and its kernel: the recurrent actor over every
// time step of a batch of episodes in ONE launch (instantiated by robogym_actor_unroll.hip).  DESIGN.md section 4 "Actor unroll"
// is the same rule.
//
// What a learner does first with an episode batch obs [B][L + 1][N][D] (EPyMARL: mac.init_hidden(B), then mac.forward(batch, t) for
// t = 0 .. L; twice per training step, the second time for the target network):
//
// For every episode b < B and agent n < N independently:
//   - h_{-1} = hidden_in[b][n], or zero when hidden_in is NULL.
//   - For t = 0 .. rows-1 in order, (q[b][t][n][:], h_t) = actor(obs[b][t][n][:] (+ one-hot n), h_{t-1}).
//   - actions[b][t][n] is the greedy action, by the existing epilogue's arg-max rule: the first maximum, with NaN counted as the
//     largest value.
//   - hidden_out[b][n] = h_{rows-1}.
//   - The observation at t = 0 is read as stored.  This is not rg_actor_forward's `restart` flag, which also zeroes the observation.
//   - There are no `filled` masks.  Every one of the `rows` time steps is computed, as EPyMARL does.  The caller limits `rows` with
//     `trim`.
// The result equals `rows` calls of rg_actor_forward (gru_packed == 3, restart = NULL) on the time slices, with the hidden state
// carried through memory: bit for bit, because a time step here IS that launch's tile computation (actor_body.inc with SPLIT = 2),
// and a row's result does not depend on the tile or the neighbours it is computed with.
//
// The kernel.  One workgroup of H / 32 wavefronts owns one tile of TM = 32 rows for the whole call -- with shared weights 32 flat
// rows of [B N], with one weight set per agent 32 episodes of one agent index (actor_kernel's own tiling) -- and walks it through
// the time steps.  The tile's hidden state sits in an LDS block [32][H] float32, loaded (or zeroed) once at the head and written
// back once at the end; each step reads it and replaces it through the body's hidden-state hooks, as policy_tile does.  The batch
// is episode-major, so a flat row r = b N + n is found at row (r / N) pitch N + t N + r % N of the observations and of the outputs
// (the body's RG_ACTOR_IN_ROW / RG_ACTOR_OUT_ROW hooks; the two pitches may differ).
// LDS (from the code): the body's three [32][H] images + the resident block: 48 KB + 16 KB = 64 KB at H = 128, 24 KB + 8 KB = 32 KB
// at H = 64: two workgroups per CU out of 160 KB, with 256 registers per lane as in the other includers.
// Barriers: the body's own, and ONE workgroup barrier between two time steps (the epilogue's reads of fc2's partial sums against
// the next step's staging stores into the same image), which orders LDS only: the q rows of step t drain under step t + 1.  The
// body's barriers already stand between a step's stores to the resident block and the next step's loads from it, and behind the
// last step's stores.  Nothing in the launch produces data the launch itself reads from memory (hidden_out may be hidden_in: a
// tile reads its rows at the head and writes the same rows at the end), there are no cross-workgroup dependencies and no
// device-wide synchronisation.
// Not here: sampling and exploration (a learner wants logits), masks, and a prefetch of step t + 1's observation rows under step
// t's GRU -- nothing has been measured that says it is needed.
#pragma once
#include "actor_common.h"
#include "device_common.h"   // kernarg_block

namespace rg {

struct UnrollArgs {
    ActorArgs act;             // weights, obs, q, actions, E = the number of episodes B, N, D, append_agent_id, ip; no restart, no
                               // uniforms; `hidden` is not used
    const float *hidden_in;    // [B][N][H] or NULL: zeros
    float *hidden_out;         // [B][N][H] or NULL
    int32_t rows, in_pitch, out_pitch;   // time steps computed; rows per episode of obs; of q and actions
    uint32_t tile_inv;         // ceil(2^32 / N) with one weight set per agent (unroll_tile), else 0
};

// Tile row i of a tile is flat row r0 + i * stride (stride 1 with shared weights, N with one set per agent).  The body's hooks are
// handed the flat row: i = (r - r0) / stride, as a multiplication -- inv = ceil(2^32 / stride), from the host, and i = the high
// word of (r - r0) * inv, exact for i < 32 and 1 < stride < 2^26 (i stride inv = i 2^32 + i e with e < stride, and i e < 2^31; the
// host refuses more agents than that; N = 1 is the flat case).  A row outside the tile (the body passes r = 0 for one) reads some row of the block; what comes back is
// not used.
template <int H>
__device__ __forceinline__ void unroll_tile(const ActorArgs &a, float *hres, int t_set, int t_base, unsigned u_r0, unsigned u_inv,
                                            int u_t, int u_in_pitch, int u_out_pitch, int u_tid) {
    constexpr int SPLIT = 2;
    const bool u_flat = a.w.n_sets == 1 || a.N == 1;
    auto u_tile_row = [&](int r) {
        const unsigned x = static_cast<unsigned>(r) - u_r0, i = u_flat ? x : __umulhi(x, u_inv);
        return i < static_cast<unsigned>(TM) ? i : 0u;
    };
#define RG_ACTOR_LOCATE(shared, E, set, base) \
    set = t_set;                              \
    base = t_base
#define RG_ACTOR_HIDDEN_LOAD(r, k4) *reinterpret_cast<const float4 *>(&hres[u_tile_row(r) * H + 4 * (k4)])
#define RG_ACTOR_HIDDEN_STORE(r, j, v) hres[u_tile_row(r) * H + (j)] = (v)
#define RG_ACTOR_IN_ROW(r) (((r) / a.N) * u_in_pitch * a.N + u_t * a.N + (r) % a.N)
#define RG_ACTOR_OUT_ROW(r) (((r) / a.N) * u_out_pitch * a.N + u_t * a.N + (r) % a.N)
#define RG_ACTOR_THREAD u_tid
#include "actor_body.inc"
#undef RG_ACTOR_LOCATE
#undef RG_ACTOR_HIDDEN_LOAD
#undef RG_ACTOR_HIDDEN_STORE
#undef RG_ACTOR_IN_ROW
#undef RG_ACTOR_OUT_ROW
#undef RG_ACTOR_THREAD
}

template <int H>
__attribute__((amdgpu_waves_per_eu(2, 2)))   // 256 registers (VGPR + AGPR), as actor_kernel: two tiles per CU
__global__ __launch_bounds__(64 * (H / 32)) void unroll_kernel(const UnrollArgs ua_in) {
    constexpr int NTHREADS = 64 * (H / 32), HV = (TM * (H / 4)) / NTHREADS;
    __shared__ __attribute__((aligned(16))) float hres[TM * H];   // the tile's hidden state, row i = tile row i
    const UnrollArgs &ua = ua_in;
    const int tid = threadIdx.x;
    const int B = ua.act.E, N = ua.act.N, rows = ua.rows;
    const bool shared = ua.act.w.n_sets == 1;
    // tile -> weight set and first row, as actor_kernel
    int set = 0, base;
    if (shared) {
        base = blockIdx.x * TM;
    } else {
        const int tiles_per_agent = (B + TM - 1) / TM;
        set = blockIdx.x / tiles_per_agent;
        base = (blockIdx.x - set * tiles_per_agent) * TM;
    }
    const int stride = shared ? 1 : N, r0 = shared ? base : base * N + set;
    const int left = (shared ? B * N : B) - base, nrows = left < TM ? left : TM;   // valid tile rows

    // (thread tid holds float4 tid + NTHREADS m of the block here, in the body's loads and in the write-back below)
#pragma unroll
    for (int m = 0; m < HV; ++m) {
        const int idx = tid + NTHREADS * m, i = idx / (H / 4), k4 = idx % (H / 4);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (ua.hidden_in && i < nrows) v = *reinterpret_cast<const float4 *>(ua.hidden_in + static_cast<size_t>(r0 + i * stride) * H + 4 * k4);
        reinterpret_cast<float4 *>(hres)[idx] = v;
    }
    __syncthreads();

    for (int t = 0; t < rows; ++t) {
        // The argument block is re-addressed every time step (device_common.h kernarg_block), as in policy_body.inc: left
        // loop-invariant, the compiler hoists every kernel-argument load of the body out of the time loop and holds them across it.
        const UnrollArgs &ua = *(const UnrollArgs *)kernarg_block<UnrollArgs>();
        // So is the thread's index: everything the body derives from it alone -- a hundred swizzled LDS addresses and weight-stream
        // offsets per lane -- is loop-invariant too, and held across the loop it spilled 86 registers per lane (340 bytes of scratch).
        int tid_t = tid;
        asm volatile("" : "+v"(tid_t));
        if (t) lds_barrier();   // the previous step's last reads of the body's images
        unroll_tile<H>(ua.act, hres, set, base, static_cast<unsigned>(r0), ua.tile_inv, t, ua.in_pitch, ua.out_pitch, tid_t);
    }
    // (the body's barriers stand behind the last step's stores to the block)
    if (ua.hidden_out) {
#pragma unroll
        for (int m = 0; m < HV; ++m) {
            const int idx = tid + NTHREADS * m, i = idx / (H / 4), k4 = idx % (H / 4);
            if (i < nrows)
                *reinterpret_cast<float4 *>(ua.hidden_out + static_cast<size_t>(r0 + i * stride) * H + 4 * k4) = reinterpret_cast<const float4 *>(hres)[idx];
        }
    }
}

}  // namespace rg
