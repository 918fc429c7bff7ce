// td_targets.h -- the rule of rg_td_targets (include/robogym.h), stated once, and its kernels: the gradient-free half of a
// Q-learner's training step -- episode mask, double-Q gather, TARGET MIXER, reward + gamma (1 - terminated) mixed -- in ONE launch
// (instantiated by robogym_td_targets.hip).  DESIGN.md section 4 "TD targets" is the same rule.
//
// What EPyMARL's q_learner.train computes under detach() from the target network's unroll (double_q: true, mixer: qmix / vdn / none;
// QMixer with mixing_embed_dim 32, hypernet_layers 2, hypernet_embed 64; `state` is the concatenated observations):
//
// Inputs.
//   - qt [B][q_pitch][N][A] f32: the target actor's unroll.
//   - sel [B][q_pitch][N] i32 or NULL: the online actor's greedy actions, which is double-Q.
//   - obs [B][obs_pitch][N][D] f32: the state of row (b, t) is the S = N D contiguous floats of obs[b][t], read in place.
//   - reward f32, terminated u8 and filled u8, each [B][flag_pitch].
//   - rows >= 2, with T = rows - 1.
//   - gamma.
//   - kind in {none, vdn, qmix} and the mixer's weights.
// Outputs.
//   - targets [B][out_pitch] f32.  For `none` it is [B][out_pitch][N].
//   - Optional mask [B][out_pitch] f32.
//   - Optional agent_q [B][out_pitch][N] f32: the per-agent value before mixing.
// For every b < B and t < T independently:
//   - Mask.  mask[b][t] = filled[b][t] && (t == 0 || !terminated[b][t-1]), as 0.0 / 1.0.  This is EPyMARL's
//     mask[:, 1:] *= 1 - terminated[:, :-1].
//   - Masked rows.  A row with mask == 0 gets targets = 0.0 and agent_q = 0.0.  None of its qt, sel or obs rows is read.
//   - Terminal rows.  A row with mask == 1 and terminated[b][t] gets targets = reward[b][t] and agent_q = 0.0.  Row t+1 is not read.
//   - Agent values.  Otherwise a_n = sel[b][t+1][n] and agent_q[n] = qt[b][t+1][n][a_n].
//       - An a_n outside [0, A) makes agent_q[n] NaN, and with it that row's target (with `none`: that agent's), and reads nothing
//         out of bounds.
//       - With sel == NULL, agent_q[n] is the maximum of qt[b][t+1][n][:] by the actor epilogue's existing rule: the first maximum,
//         with a NaN counting as the largest value.
//       - avail_actions is all ones in this project and plays no part.
//   - Mixing.
//       - none: y_n = agent_q[n].
//       - vdn: y is the binary32 sum over n = 0 .. N-1 in that order: ((agent_q[0] + agent_q[1]) + agent_q[2]) + ...
//       - qmix: EPyMARL's QMixer.forward on (agent_q, state[b][t+1]):
//           w1 = |W1b relu(W1a s + b1a) + b1b|, viewed [N][32].
//           b1 = Wb s + bb.
//           hidden = elu(agent_q w1 + b1).
//           wf = |Wfb relu(Wfa s + bfa) + bfb|, [32].
//           v = Vb relu(Va s + ba) + bv.
//           y = hidden wf + v.
//   - Target.  targets = fl(reward[b][t] + fl(gamma y)).  The product is rounded before the sum, with no contraction.
// Rows t >= T of the outputs are not touched.
// With none and vdn this fixes every bit.  The qmix arithmetic is float32 with a summation order of the kernel's choosing.
//
// The kernels.
//   none / vdn (td_gather_kernel): a gather and a sum, a few dozen bytes per row: one thread per (b, t) row, 256 rows per workgroup.
//   qmix (td_qmix_kernel): one workgroup of 3 wavefronts owns a tile of TM = 32 consecutive flat rows r = b T + t.
//     1. Lanes 0..31 read the tile's flags.  A tile without a live row (mask == 1 and not terminal) writes its zeros / rewards and
//        leaves: this is how the padding behind the episodes' ends is skipped.
//     2. The tile's agent values go to LDS (aq [32][16]) and its state rows to LDS (st [32][SP + 1], SP = S padded to a multiple of
//        4 with zeros; rows that are not live are zeros and read nothing).
//     3. The first layers of the four hypernetworks side by side, [32 x SP] [SP x 192] (columns: 64 of hyper_w_1.0, 64 of
//        hyper_w_final.0, 32 of V.0, 32 of hyper_b_1), as six 32 x 32 blocks on v_mfma_f32_32x32x2_f32, two per wavefront: the A
//        operand is one LDS word per lane and k step (the row stride SP + 1 is odd: no bank conflicts), the B operand one word of
//        the K-major packed weights from memory (32 lanes contiguous).  The exact f32 matrix instruction, not plain FMAs: it is a
//        k-ordered fmaf chain at the vector rate, and it keeps a 32 x 32 block in 16 accumulator registers with ONE register per
//        operand, where an FMA form of the same block needs each lane to re-read or hold a row of the state for every column it owns.
//        Every block is summed in TWO chains, the k steps dealt out in turn (steps 0, 2, 4 .. and 1, 3, 5 ..) and the chains added
//        at the end: half the chain length (measured against float64 the error falls by about a sixth) and independent accumulators.
//        Bias and ReLU are applied from the accumulators, and the result goes to LDS (h1 [32][193]).
//     4. The second layers from LDS: N + 1 blocks [32 x 64] [64 x 32] spread over the wavefronts -- block n < N is w1[:, n, :],
//        folded into the wavefront's partial `hidden` as agent_q[n] |.| straight from the accumulators; block N is wf.
//     5. The partial hiddens and wf meet in LDS (the state's image, dead by then); 32 lanes per row finish elu, the product with
//        wf and V's second layer, a butterfly sum gives y, and lane 0 of the row forms the target and stores.
//   LDS: 32 x 257 + 32 x 193 + 32 x 16 words + flags = 60 032 bytes: two workgroups per CU.  No scratch.  Three workgroup barriers.
//   A row's result depends on that row's inputs alone (an MFMA output element is a function of its A row and B column), so a NaN
//   stays in its row, and a row computes the same whatever tile it is in.
//   No cross-workgroup dependency, no device-wide synchronisation, no atomics.  Not here: compaction of the live rows into dense
//   tiles -- nothing has been measured that says it is needed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/robogym.h"
#include "mixer_tile.h"

namespace rg {

struct TdArgs {
    rg_mixer_weights m;
    rg_td_targets_io io;
    int32_t T;            // rows - 1
    int32_t total;        // B T flat rows
    int32_t sp;           // S padded to a multiple of 4 (qmix)
};

// 0: masked, 1: terminal, 2: live
__device__ __forceinline__ int td_row_flag(const rg_td_targets_io &io, int b, int t) {
    const size_t f = static_cast<size_t>(b) * io.flag_pitch + t;
    const bool m = io.filled[f] != 0 && (t == 0 || io.terminated[f - 1] == 0);
    return !m ? 0 : (io.terminated[f] != 0 ? 1 : 2);
}

// agent_q[n] of a live row (b, t): from row t + 1 of qt (and sel)
__device__ __forceinline__ float td_agent_value(const rg_td_targets_io &io, int b, int t, int n) {
    const size_t an = (static_cast<size_t>(b) * io.q_pitch + t + 1) * io.n_agents + n;
    const float *q = io.qt + an * io.n_actions;
    if (io.sel) {
        const int a = io.sel[an];
        return static_cast<unsigned>(a) < static_cast<unsigned>(io.n_actions) ? q[a] : __builtin_nanf("");
    }
    float best = q[0];
    for (int c = 1; c < io.n_actions; ++c) {
        const float v = q[c];
        if (v > best || (v != v && best == best)) best = v;   // the first maximum, a NaN counting as the largest value
    }
    return best;
}

__device__ __forceinline__ float td_target(float reward, float gamma, float y) { return __fadd_rn(reward, __fmul_rn(gamma, y)); }

// none / vdn: one thread per row
__global__ __launch_bounds__(256) void td_gather_kernel(const TdArgs a) {
    const rg_td_targets_io &io = a.io;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.total) return;
    const int b = r / a.T, t = r - b * a.T, N = io.n_agents;
    const bool vdn = a.m.kind == RG_MIXER_VDN;
    const int flag = td_row_flag(io, b, t);
    const size_t o = static_cast<size_t>(b) * io.out_pitch + t;
    if (io.mask) io.mask[o] = flag ? 1.0f : 0.0f;
    if (flag != 2) {
        const float v = flag == 1 ? io.reward[static_cast<size_t>(b) * io.flag_pitch + t] : 0.0f;
        if (vdn) io.targets[o] = v;
        for (int n = 0; n < N; ++n) {
            if (!vdn) io.targets[o * N + n] = v;
            if (io.agent_q) io.agent_q[o * N + n] = 0.0f;
        }
        return;
    }
    const float reward = io.reward[static_cast<size_t>(b) * io.flag_pitch + t];
    float y = 0.0f;
    for (int n = 0; n < N; ++n) {
        const float q = td_agent_value(io, b, t, n);
        if (io.agent_q) io.agent_q[o * N + n] = q;
        if (!vdn) io.targets[o * N + n] = td_target(reward, io.gamma, q);
        y = n ? __fadd_rn(y, q) : q;
    }
    if (vdn) io.targets[o] = td_target(reward, io.gamma, y);
}

// qmix: one workgroup per tile of 32 rows
__global__ __launch_bounds__(TD_NT) void td_qmix_kernel(const TdArgs a) {
    __shared__ float st[TD_TM * (TD_MAX_SP + 1)];   // the state rows; from step 4 on the partial hiddens [3][32][33] and wf [32][33]
    __shared__ float h1[TD_TM * TD_H1S];            // the first layers' outputs
    __shared__ float aq[TD_TM * RG_MAX_AGENTS];     // agent_q of the tile's rows (zero for a row that is not live)
    __shared__ int flags[TD_TM];                    // td_row_flag, or -1 behind the last row
    const rg_td_targets_io &io = a.io;
    const rg_mixer_weights &m = a.m;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = io.n_agents, S = N * io.obs_dim, sp = a.sp, sps = sp + 1, T = a.T;
    const int base = blockIdx.x * TD_TM;

    // 1. flags
    int mine = -1;
    if (tid < TD_TM) {
        const int r = base + tid;
        if (r < a.total) {
            const int b = r / T;
            mine = td_row_flag(io, b, r - b * T);
        }
        flags[tid] = mine;
    }
    const int live = __syncthreads_or(mine == 2);
    if (!live) {
        if (mine >= 0) {
            const int r = base + tid, b = r / T, t = r - b * T;
            const size_t o = static_cast<size_t>(b) * io.out_pitch + t;
            io.targets[o] = mine == 1 ? io.reward[static_cast<size_t>(b) * io.flag_pitch + t] : 0.0f;
            if (io.mask) io.mask[o] = mine ? 1.0f : 0.0f;
            if (io.agent_q)
                for (int n = 0; n < N; ++n) io.agent_q[o * N + n] = 0.0f;
        }
        return;
    }

    // 2. agent values and state rows
    for (int idx = tid; idx < TD_TM * N; idx += TD_NT) {
        const int i = idx / N, n = idx - i * N;
        float v = 0.0f;
        if (flags[i] == 2) {
            const int r = base + i, b = r / T;
            v = td_agent_value(io, b, r - b * T, n);
        }
        aq[i * RG_MAX_AGENTS + n] = v;
    }
    for (int i = wave; i < TD_TM; i += TD_NT / 64) {
        const bool on = flags[i] == 2;
        const int r = base + i, b = on ? r / T : 0, t = on ? r - b * T : 0;
        const float *src = io.obs + (static_cast<size_t>(b) * io.obs_pitch + t + 1) * S;
        for (int k = lane; k < sp; k += 64) st[i * sps + k] = (on && k < S) ? src[k] : 0.0f;
    }
    __syncthreads();

    // 3. the first layers: blocks `wave` and `wave + 3` of the six
    const int lr = lane & 31, lh = lane >> 5;
    {
        // Two chains per block, the k steps dealt out in turn and the chains added at the end: half the length of one fmaf chain
        // (the error of a chain grows with its length), and four independent accumulators for the matrix pipeline.
        f32x16 acc0 = {0}, acc1 = {0}, odd0 = {0}, odd1 = {0};
        const float *w0 = m.w_in + lh * TD_C1 + 32 * wave + lr, *w1 = w0 + 96;
        const float *arow = st + lr * sps + lh;
        for (int k = 0; k < sp; k += 4) {   // (sp is a multiple of 4: two k steps of the product at a time)
            const float av0 = arow[k], av1 = arow[k + 2];
            const float b00 = w0[static_cast<size_t>(k) * TD_C1], b10 = w1[static_cast<size_t>(k) * TD_C1];
            const float b01 = w0[static_cast<size_t>(k + 2) * TD_C1], b11 = w1[static_cast<size_t>(k + 2) * TD_C1];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, b00, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av0, b10, acc1, 0, 0, 0);
            odd0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, b01, odd0, 0, 0, 0);
            odd1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av1, b11, odd1, 0, 0, 0);
        }
        acc0 += odd0;
        acc1 += odd1;
        const int c0 = 32 * wave + lr, c1 = c0 + 96;
        const float bias0 = m.b_in[c0], bias1 = m.b_in[c1];
        const bool relu1 = c1 < TD_COL_B1;   // hyper_b_1 is one linear layer: no ReLU behind it (wave-uniform: a whole block)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int row = (j & 3) + 8 * (j >> 2) + 4 * lh;
            const float x0 = acc0[j] + bias0, x1 = acc1[j] + bias1;
            h1[row * TD_H1S + c0] = x0 > 0.0f ? x0 : (x0 != x0 ? x0 : 0.0f);
            h1[row * TD_H1S + c1] = !relu1 ? x1 : (x1 > 0.0f ? x1 : (x1 != x1 ? x1 : 0.0f));
        }
    }
    __syncthreads();   // h1 is complete, and every read of st is done

    // 4. the second layers: blocks 0 .. N - 1 are w1[:, n, :], block N is wf
    float *part = st, *wf = st + 3 * TD_TM * TD_PS;
    {
        f32x16 hid = {0};
        for (int blk = wave; blk <= N; blk += TD_NT / 64) {
            const bool is_w1 = blk < N;
            const int ldb = is_w1 ? N * TD_EMBED : TD_EMBED;
            const float *wb = (is_w1 ? m.w_w1 + blk * TD_EMBED : m.w_wf) + lh * ldb + lr;
            const float *arow = h1 + lr * TD_H1S + (is_w1 ? 0 : TD_COL_WF) + lh;
            f32x16 acc = {0}, odd = {0};   // two chains, as above
#pragma unroll 4
            for (int k = 0; k < TD_HYPER; k += 4) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[k], wb[static_cast<size_t>(k) * ldb], acc, 0, 0, 0);
                odd = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[k + 2], wb[static_cast<size_t>(k + 2) * ldb], odd, 0, 0, 0);
            }
            acc += odd;
            const float bias = is_w1 ? m.b_w1[blk * TD_EMBED + lr] : m.b_wf[lr];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int row = (j & 3) + 8 * (j >> 2) + 4 * lh;
                const float w = __builtin_fabsf(acc[j] + bias);
                if (is_w1) hid[j] = hid[j] + aq[row * RG_MAX_AGENTS + blk] * w;
                else wf[row * TD_PS + lr] = w;
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int row = (j & 3) + 8 * (j >> 2) + 4 * lh;
            part[(wave * TD_TM + row) * TD_PS + lr] = hid[j];
        }
    }
    __syncthreads();

    // 5. per row: elu, the product with wf, V's second layer, the sum over the 32 columns, the target
    for (int idx = tid; idx < TD_TM * TD_EMBED; idx += TD_NT) {   // (whole groups of 32 lanes: 192 and 1024 are multiples of 32)
        const int row = idx >> 5, e = idx & 31;
        float h = (part[row * TD_PS + e] + part[(TD_TM + row) * TD_PS + e]) + part[(2 * TD_TM + row) * TD_PS + e];
        h = h + h1[row * TD_H1S + TD_COL_B1 + e];
        h = h > 0.0f ? h : expm1f(h);
        float s = h * wf[row * TD_PS + e] + m.w_v[e] * h1[row * TD_H1S + TD_COL_V + e];
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) s += __shfl_xor(s, d, 32);
        const int flag = flags[row];
        if (flag < 0) continue;
        const int r = base + row, b = r / T, t = r - b * T;
        const size_t o = static_cast<size_t>(b) * io.out_pitch + t;
        if (e == 0) {
            const float reward = flag ? io.reward[static_cast<size_t>(b) * io.flag_pitch + t] : 0.0f;
            io.targets[o] = flag == 2 ? td_target(reward, io.gamma, s + m.b_v[0]) : reward;
            if (io.mask) io.mask[o] = flag ? 1.0f : 0.0f;
        }
        if (io.agent_q && e < N) io.agent_q[o * N + e] = aq[row * RG_MAX_AGENTS + e];
    }
}

}  // namespace rg
