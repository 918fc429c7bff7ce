// nstep_returns.h -- the rule of rg_nstep_returns (include/robogym_returns.h), stated once, and its kernel: what a PPO learner
// computes under no_grad every epoch -- the episode mask, the TARGET CRITIC over every row of the episode batch, and EPyMARL's
// nstep_returns -- in ONE launch (instantiated by robogym_nstep_returns.hip).  DESIGN.md section 4 "N-step returns" is the same rule.
//
// EPyMARL's ppo_learner with critic_type cv_critic / cv_critic_ns, q_nstep n and add_value_last_step; `state` is the concatenated
// observations.  Where the rule follows or leaves EPyMARL it says so.
//
// Inputs.
//   - obs [B][obs_pitch][N][D] f32: the state of row (b, t) is the S = N D contiguous floats of obs[b][t], read in place.
//   - reward f32, terminated u8 and filled u8, each [B][flag_pitch].
//   - rows >= 2, with T = rows - 1.
//   - gamma in [0, 1]; nstep n in 1..32; add_value_last_step (0 / 1).
//   - value_scale and value_shift, finite: EPyMARL's standardise_returns de-normalisation v sqrt(var) + mean (1 and 0: none).
//   - The critic: kind in {cv, cv_ns}, hidden width H in {64, 128}, and its packed weights.
// Outputs.
//   - returns [B][out_pitch][N] f32, rows 0 .. T-1.
//   - values [B][value_pitch][N] f32, rows 0 .. T.
//   - Optional mask [B][out_pitch] f32, rows 0 .. T-1.
// For every episode b independently:
//   - Mask.  m[t] = filled[b][t] && (t == 0 || !terminated[b][t-1]) for t < T, exactly rg_td_targets's mask (EPyMARL's
//     mask[:, 1:] *= 1 - terminated[:, :-1]), written as 0.0 / 1.0.
//   - Needed rows.  Row t < T is needed iff m[t].  Row T is needed iff add_value_last_step && m[T-1].  An obs row that is not
//     needed is not read.  A reward[t] with m[t] == 0 is not read.  reward[T] is not read.
//   - Values.  values[b][t][a] = fl(fl(value_scale c) + value_shift) for needed rows and 0.0 otherwise, for t in 0 .. T.  Rows behind
//     `rows` of the outputs are not touched.  c is the critic's output in float32 arithmetic with a summation order of the kernel's
//     choosing:
//       - cv (EPyMARL's CentralVCritic with obs_individual_obs and obs_last_action false):
//         fc3(relu(fc2(relu(fc1([state, onehot_N(a)]))))) with fc1.weight [H, S+N], fc2.weight [H, H], fc3.weight [1, H].  The first
//         layer's state part is shared by a row's N agents, and the identity column is added per agent.
//       - cv_ns (CentralVCriticNS): N separate such networks on `state` alone, so fc1.weight [H, S].
//   - Discounts.  g[k] = (float) pow((double) gamma, (double) k) for k = 0 .. n+1, computed on the host by the C entry point: what
//     `gamma ** k * tensor` multiplies by in torch.
//   - Returns.  For every t0 < T and agent a: if m[t0] == 0 the return is 0.0 and nothing is read.  Otherwise start from
//     ret = +0.0 and for k = 0, 1, .., n take t = t0 + k:
//       - if t >= T: stop;
//       - if k == n: when m[t], ret = fl(ret + fl(g[k] values[t][a]));
//       - if k < n: when m[t], ret = fl(ret + fl(g[k] reward[t])); then, if t == T-1 && add_value_last_step && m[T-1],
//         ret = fl(ret + fl(g[k+1] values[T][a])).
//     Products are rounded before sums and nothing is contracted.  Given `values`, this fixes every bit of `returns`.
//   - One deliberate difference from EPyMARL: EPyMARL adds the last-step value term WITHOUT the factor m[T-1].  For an episode that
//     ended before row T-1 it so puts the critic's value of a padding row into up to n live rows' returns; this project does not read
//     padding.  On every other row with m == 1 the rule equals EPyMARL's line for line (skipping a masked term equals adding its
//     (g r) 0 for finite rewards).
//   - NaNs.  A NaN in one needed obs row reaches only the values of that row and the returns that the rule says read them.
//
// The kernel (nstep_returns_kernel<H>): ONE WORKGROUP PER EPISODE, H / 32 wavefronts (4 at H = 128, 2 at H = 64) -- the scan
// needs an episode's values together, and one workgroup that computes them and then scans them needs no cross-workgroup
// dependency, no device-wide synchronisation and no atomics.  At B = 32 this leaves most of the chip idle and a call takes one
// episode's serial time (measured: 67 us at 85 rows x 4 agents, against 14 ms for the torch lines); a split of an episode over
// workgroups would need a second launch or a cross-workgroup dependency for the scan, and was not pursued.
//   1. Every thread walks the flags: m[t] goes to LDS as bytes (rows <= 4096) and, as 0.0 / 1.0, to `mask`.
//   2. The rows are walked in tiles of 32 consecutive rows t; a tile is 32 (row, agent) pairs per agent, taken agent by agent.  A
//      tile without a needed row writes its zeros and is skipped: this is how the padding behind an episode's end costs nothing, and
//      an episode with no live row writes zeros only.
//        a. The tile's state rows go to LDS (st [32][SP + 1], SP = S padded to a multiple of 8 with zeros; rows that are not needed
//           are zeros and read nothing).
//        b. fc1's state part [32 x SP] [SP x H] on v_mfma_f32_32x32x2_f32, the exact f32 matrix instruction (a k-ordered fmaf chain
//           at the vector rate, a 32 x 32 block in 16 accumulator registers with ONE register per operand): wavefront w owns the
//           columns 32 w .. 32 w + 31.  A operand: one LDS word per lane and k step (the row stride SP + 1 is odd: no bank
//           conflicts); B operand: one word of the K-major packed weights from memory (32 lanes contiguous).  cv: once per tile,
//           the block stays in registers for the tile's N agents.  cv_ns: per agent, with that agent's network.
//        c. Per agent a: bias (cv: and the identity column of a) and ReLU from the accumulators to LDS (h1 [32][H + 1]); barrier;
//           fc2 [32 x H] [H x H], again one 32-column block per wavefront, A from h1, B FROM REGISTERS: the wavefront's [H x 32]
//           block of fc2.weight is H / 2 registers per lane (64 at H = 128), loaded once per workgroup (cv) or once per agent and
//           tile (cv_ns).  Neither LDS (64 KB at H = 128 would leave one workgroup per CU) nor L2 (16 KB per wavefront and tile,
//           behind the matrix pipe's back) is read for fc2's weights inside the k loop.
//        d. Bias, ReLU and the product with fc3.weight from the accumulators; a butterfly sum over the 32 columns of a lane half,
//           the wavefronts' partial sums meet in LDS (part [4][32]); barrier; 32 lanes add them in wavefront order, add fc3.bias,
//           scale and shift, and store values[b][t][a] (0.0 for a row that is not needed).
//      Every product is summed in FOUR chains, the k steps dealt out in turn and the chains added at the end ((c0 + c1) + (c2 + c3)):
//      a quarter of the chain length (the error of a chain grows with its length) and four independent accumulators, with which one
//      wavefront per SIMD keeps the matrix pipe at its issue rate.
//   3. Barrier (the values were written by this workgroup; the barrier's workgroup-scope fence makes them visible to it); then
//      one thread per (t0, a) runs the n-step pass as the rule states it, reading m from LDS, reward and values from memory.
//   LDS at H = 128: 32 x 257 (st) + 32 x 129 (h1) + 4 x 32 (part) words + 32 (tile flags) + 4096 (mask bytes) = 54 144 bytes, and at
//   H = 64 45 696 bytes: two workgroups per CU of 160 KiB.  Registers: at most 256 (vector + accumulator) per lane, which is what two
//   workgroups of one wavefront per SIMD each leave a wavefront.  No scratch.
//   A row's values depend on that row's inputs alone (an MFMA output element is a function of its A row and B column), so a NaN
//   stays in its row, and a row computes the same whatever tile it is in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/robogym_returns.h"

namespace rg {

constexpr int NR_TM = 32;                 // rows of a tile
constexpr int NR_MAX_SP = 256;            // the padded state width the LDS image holds
constexpr int NR_MAX_ROWS = RG_RETURNS_MAX_ROWS;

struct NrArgs {
    rg_critic_weights w;
    rg_nstep_returns_io io;
    int32_t T;                    // rows - 1
    int32_t sp;                   // S padded to a multiple of 8
    float g[RG_NSTEP_MAX + 2];    // the discounts g[0 .. n + 1]
};

using nr_f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ float nr_relu(float x) { return x > 0.0f ? x : (x != x ? x : 0.0f); }   // a NaN stays a NaN
__device__ __forceinline__ int nr_acc_row(int j, int lh) { return (j & 3) + 8 * (j >> 2) + 4 * lh; }

template <int H>
__global__ __launch_bounds__(2 * H, 2) void nstep_returns_kernel(const NrArgs a) {
    constexpr int NT = 2 * H, NW = H / 32, HS = H + 1, KS = H / 2;   // threads, wavefronts, h1's row stride, fc2's k steps
    __shared__ float st[NR_TM * (NR_MAX_SP + 1)];    // the tile's state rows
    __shared__ float h1[NR_TM * HS];                 // relu(fc1) of the tile's rows for one agent
    __shared__ float part[NW * NR_TM];               // the wavefronts' partial fc3 sums
    __shared__ int need[NR_TM];                      // the tile's rows: needed (1), not needed (0), behind the last row (-1)
    __shared__ uint8_t m[NR_MAX_ROWS];               // the episode's mask, t < T
    const rg_nstep_returns_io &io = a.io;
    const rg_critic_weights &cw = a.w;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int N = io.n_agents, S = N * io.obs_dim, sp = a.sp, sps = sp + 1, T = a.T, rows = io.rows;
    const int b = blockIdx.x;
    const bool cv = cw.kind == RG_CRITIC_CV;
    const uint8_t *filled = io.filled + static_cast<size_t>(b) * io.flag_pitch, *terminated = io.terminated + static_cast<size_t>(b) * io.flag_pitch;
    const float *reward = io.reward + static_cast<size_t>(b) * io.flag_pitch;
    const float *obs = io.obs + static_cast<size_t>(b) * io.obs_pitch * S;
    float *values = io.values + static_cast<size_t>(b) * io.value_pitch * N;
    float *returns = io.returns + static_cast<size_t>(b) * io.out_pitch * N;

    // 1. the mask
    for (int t = tid; t < T; t += NT) {
        const bool on = filled[t] != 0 && (t == 0 || terminated[t - 1] == 0);
        m[t] = on;
        if (io.mask) io.mask[static_cast<size_t>(b) * io.out_pitch + t] = on ? 1.0f : 0.0f;
    }
    __syncthreads();
    const bool last_needed = io.add_value_last_step != 0 && m[T - 1] != 0;

    // fc2's [H x 32] block of this wavefront, in registers: k step s of lane (lr, lh) is w2[2 s + lh][32 wave + lr]
    float w2r[KS];
    const int col = 32 * wave + lr;
    if (cv) {
#pragma unroll
        for (int s = 0; s < KS; ++s) w2r[s] = cw.w2[(2 * s + lh) * H + col];
    }

    // 2. the tiles
    for (int base = 0; base < rows; base += NR_TM) {
        int mine = -1;
        if (tid < NR_TM) {
            const int t = base + tid;
            if (t < rows) mine = t < T ? m[t] : last_needed;
            need[tid] = mine;
        }
        const int any = __syncthreads_or(mine == 1);   // (also: every read of st, h1 and part of the tile before is done)
        if (!any) {
            for (int idx = tid; idx < NR_TM * N; idx += NT) {
                const int t = base + idx / N;
                if (t < rows) values[static_cast<size_t>(base) * N + idx] = 0.0f;
            }
            continue;
        }
        // a. the state rows
        for (int i = wave; i < NR_TM; i += NW) {
            const bool on = need[i] == 1;
            const float *src = obs + static_cast<size_t>(on ? base + i : 0) * S;
            for (int k = lane; k < sp; k += 64) st[i * sps + k] = (on && k < S) ? src[k] : 0.0f;
        }
        __syncthreads();

        nr_f32x16 pre = {0};
        const float *arow1 = st + lr * sps + lh;
        for (int ag = 0; ag < N; ++ag) {
            const int net = cv ? 0 : ag * cw.net_stride;
            // b. fc1's state part
            if (!cv || ag == 0) {
                nr_f32x16 c0 = {0}, c1 = {0}, c2 = {0}, c3 = {0};
                const float *wb = cw.w1 + net + lh * H + col;
                for (int k = 0; k < sp; k += 8) {   // (sp is a multiple of 8: four k steps of the product at a time)
                    const float a0 = arow1[k], a1 = arow1[k + 2], a2 = arow1[k + 4], a3 = arow1[k + 6];
                    const float b0 = wb[k * H], b1 = wb[(k + 2) * H], b2 = wb[(k + 4) * H], b3 = wb[(k + 6) * H];
                    c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, c0, 0, 0, 0);
                    c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, c1, 0, 0, 0);
                    c2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b2, c2, 0, 0, 0);
                    c3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, b3, c3, 0, 0, 0);
                }
                pre = (c0 + c1) + (c2 + c3);
                if (!cv) {
#pragma unroll
                    for (int s = 0; s < KS; ++s) w2r[s] = cw.w2[net + (2 * s + lh) * H + col];
                }
            }
            // c. bias (cv: and the identity column) and ReLU to LDS
            {
                const float bias = cw.b1[net + col], idc = cv ? cw.w1_id[ag * H + col] : 0.0f;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const float x = cv ? (pre[j] + idc) + bias : pre[j] + bias;
                    h1[nr_acc_row(j, lh) * HS + col] = nr_relu(x);
                }
            }
            __syncthreads();   // h1 is complete (and every read of part of the agent before is done)
            // fc2 from LDS and registers
            float y[16];
            {
                nr_f32x16 c0 = {0}, c1 = {0}, c2 = {0}, c3 = {0};
                const float *arow = h1 + lr * HS + lh;
#pragma unroll
                for (int s = 0; s < KS; s += 4) {
                    c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * s], w2r[s], c0, 0, 0, 0);
                    c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * s + 2], w2r[s + 1], c1, 0, 0, 0);
                    c2 = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * s + 4], w2r[s + 2], c2, 0, 0, 0);
                    c3 = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * s + 6], w2r[s + 3], c3, 0, 0, 0);
                }
                const nr_f32x16 acc = (c0 + c1) + (c2 + c3);
                // d. bias, ReLU, the product with fc3.weight, the sum over this wavefront's 32 columns
                const float bias = cw.b2[net + col], w3 = cw.w3[net + col];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    float s = nr_relu(acc[j] + bias) * w3;
#pragma unroll
                    for (int d = 16; d >= 1; d >>= 1) s += __shfl_xor(s, d, 32);
                    y[j] = s;
                }
            }
            if (lr == 0) {
#pragma unroll
                for (int j = 0; j < 16; ++j) part[wave * NR_TM + nr_acc_row(j, lh)] = y[j];
            }
            __syncthreads();   // part is complete, and every read of h1 is done
            if (tid < NR_TM && need[tid] >= 0) {
                float c = part[tid];
#pragma unroll
                for (int w = 1; w < NW; ++w) c += part[w * NR_TM + tid];
                c += cw.b3[net];
                const float v = __fadd_rn(__fmul_rn(io.value_scale, c), io.value_shift);
                values[static_cast<size_t>(base + tid) * N + ag] = need[tid] == 1 ? v : 0.0f;
            }
        }
    }
    __syncthreads();   // the episode's values are written, by this workgroup, and visible to it

    // 3. the n-step pass: one thread per (t0, agent)
    const int n = io.nstep;
    const float *vlast = values + static_cast<size_t>(T) * N;
    for (int idx = tid; idx < T * N; idx += NT) {
        const int t0 = idx / N, ag = idx - t0 * N;
        float ret = 0.0f;
        if (m[t0]) {
            for (int k = 0; k <= n; ++k) {
                const int t = t0 + k;
                if (t >= T) break;
                if (k == n) {
                    if (m[t]) ret = __fadd_rn(ret, __fmul_rn(a.g[k], values[static_cast<size_t>(t) * N + ag]));
                } else {
                    if (m[t]) ret = __fadd_rn(ret, __fmul_rn(a.g[k], reward[t]));
                    if (t == T - 1 && last_needed) ret = __fadd_rn(ret, __fmul_rn(a.g[k + 1], vlast[ag]));
                }
            }
        }
        returns[idx] = ret;
    }
}

}  // namespace rg
