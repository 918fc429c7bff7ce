// mixer_grad.h -- the rule of rg_mixer_forward / rg_mixer_backward (include/robogym_learn.h), stated once, and their kernels: the
// ONLINE mixer's pass of a Q-learner's training step WITH gradients -- chosen_action_qvals = mixer(gather(mac_out[:, :-1], actions),
// state[:, :-1]) and its backward pass -- in one launch each (instantiated by robogym_mixer_grad.hip).  DESIGN.md section 4
// "Trainable mixer" is the same rule.  The mixers are td_targets.h's (none / vdn / EPyMARL's QMixer with mixing_embed_dim 32,
// hypernet_layers 2, hypernet_embed 64), with the same limits: N <= RG_MAX_AGENTS, S padded to a multiple of 4 and at most 256,
// A <= 32.
//
// Inputs.
//   - q [B][q_pitch][N][A] f32: the online actor's output.
//   - actions [B][q_pitch][N] i32: the stored actions.
//   - obs [B][obs_pitch][N][D] f32: the state of row (b, t) is the S = N D contiguous floats of obs[b][t], row t itself.
//   - mask [B][out_pitch] f32.
//   - rows >= 2, with T = rows - 1.
//   - kind in {none, vdn, qmix} and the mixer's weights.
// Forward output.
//   - mixed [B][out_pitch] f32.  For `none` it is [B][out_pitch][N].
// For every b < B and t < T independently:
//   - Masked rows.  A row with mask == 0.0 gets mixed = 0.0.  None of its q, actions or obs rows is read, and every gradient of it
//     is zero.  Any other mask value makes the row live; terminal rows are live.
//   - Chosen values.  x_n = q[b][t][n][actions[b][t][n]].  An action outside [0, A) makes x_n NaN, and with it that row's mixed
//     (with `none`: that agent's), and reads or writes nothing out of bounds, forward or backward.
//   - Mixing.
//       - none: mixed[b][t][n] = x_n.
//       - vdn: mixed is the binary32 sum over n = 0 .. N-1 in that order: ((x_0 + x_1) + x_2) + ...
//       - qmix: EPyMARL's QMixer.forward on (x, state[b][t]):
//           a1 = W1a s + b1a, g1 = relu(a1), p1 = W1b g1 + b1b, w1 = |p1|, viewed [N][32].
//           b1 = Wb s + bb.
//           u = x w1 + b1, hidden = elu(u).
//           af = Wfa s + bfa, gf = relu(af), pf = Wfb gf + bfb, wf = |pf|, [32].
//           av = Va s + ba, gv = relu(av), v = Vb gv + bv.
//           y = hidden wf + v, and mixed = y.
// Backward, given d_mixed [B][out_pitch] ([B][out_pitch][N] for `none`), dy = d_mixed[b][t] of a live row, with torch's own
// convention at the kinks: relu'(0) = 0, and d|p|/dp = sign(p) with sign(0) = 0.
//   - none: dx_n = d_mixed[b][t][n].  vdn: dx_n = dy.
//   - qmix:
//       d_hidden = dy wf.  d_wf = dy hidden.  elu'(u) = 1 for u > 0, else hidden + 1.  du = d_hidden elu'(u).
//       dx_n = du . w1[n,:].  d_w1[n,:] = x_n du.  d_b1 = du.
//       dp1 = d_w1 sign(p1).  dpf = d_wf sign(pf).
//       dg1 = dp1 W1b and dgf = dpf Wfb, the second layers' weights untransposed.
//       da1 = dg1 [a1 > 0].  daf = dgf [af > 0].  dav = dy Vb [av > 0].
// Backward outputs.
//   - d_q [B][q_pitch][N][A]: dx_n at the chosen action, zero everywhere else in the rows t < T, zero in the whole of row T and
//     zero in masked rows.  An agent whose action is outside [0, A) has zeros alone.  The launch writes all rows t <= T.
//   - For qmix, per row, with aux_pitch >= rows rows per episode:
//       d_pre [B][aux_pitch][192] = (da1, daf, dav, d_b1), in the column order of w_in.
//       d_p2 [B][aux_pitch][N 32 + 32] = (dp1, dpf).
//       g [B][aux_pitch][160] = (g1, gf, gv).
//     Masked rows and row T hold zeros in all three.
//   - There is no gradient with respect to obs.
// The weight gradients are sums over all rows of products of these arrays, and are the caller's:
//   dW_in = d_pre^T state, dW1b = dp1^T g1, dWfb = dpf^T gf, dVb = sum dy gv, the biases as column sums (dbv = sum dy).
// Rows behind T of mixed, rows behind `rows` of every other output and the pitch padding are not touched.
// With none and vdn this fixes every bit.  The qmix arithmetic is float32 with a summation order of the kernels' choosing.
//
// The kernels.
//   none / vdn (mix_gather_forward_kernel, mix_gather_backward_kernel): one thread per (b, t) row, 256 rows per workgroup, as
//     td_gather_kernel; the backward one is the zero-filled scatter, and the thread of row T - 1 also zeroes row T.
//   qmix forward (mix_qmix_forward_kernel): td_qmix_kernel with three differences -- the gather is from row t of q / actions, the state
//     is row t, and y is stored as it is.  The same tile of 32 flat rows r = b T + t per workgroup of three wavefronts, the same
//     products on v_mfma_f32_32x32x2_f32, the same LDS (60 032 bytes: two workgroups per CU).  Two more differences, both for the
//     sake of the GRADIENTS' accuracy (an error of w1 is multiplied by x and by du on its way): every product is summed in FOUR
//     chains, not two, the k steps dealt out in turn and the chains added in pairs; and what lies BEHIND the matrix products -- u = x w1 + b1, elu, hidden wf + Vb gv, a few thousand operations per tile --
//     is done in binary64 and rounded once, here and in the backward kernel (du, dx_n likewise): the float32 error left is the
//     matrix products' own.
//     td_targets.h and this header share the tile's constants (mixer_tile.h); the forward and the backward kernel here share
//     mix_flags(), mix_first_layers() and mix_second_block().
//   qmix backward (mix_qmix_backward_kernel<NMAX>, NMAX = 8 or 16 agents): the same tile and workgroup.  It RECOMPUTES the forward
//     pass of its tile (steps 1-3 are the forward kernel's) instead of reading saved h1 / w1 / hidden: a forward pass is 0.48 ms for
//     4096 episodes, less than the traffic of saving N 32 + 192 + 32 words per row and reading them back.
//     4. The second-layer blocks store p1 and pf, SIGNED, to an LDS image (pw [32][32 NMAX + 1], over the state's image, dead by
//        then; pf [32][33]): w1 = |.| and sign(.) are both read off it, so sign(p1) needs no registers across the barrier and no
//        second pass over the blocks.  This is the choice the issue left open: registers would hold N / 3 blocks of 16 words per
//        lane across two barriers (up to 96 registers), a second pass would run the largest product twice.
//     5. 32 lanes per row: u in the forward kernel's order (three partial sums over the agents n = w, w + 3, .., added as
//        (p0 + p1) + p2, then + b1, in binary64: the forward kernel's hidden), elu, d_hidden, du (to LDS), dpf (over pf), dav and d_b1.
//     6. 32 lanes per (row, n): dx_n = sum_e du[e] |p1[n][e]| by a butterfly; dp1 = (x_n du) sign(p1) overwrites p1 in the image
//        and goes to d_p2.
//     7. dg1 = dp1 W1b (K = 32 N) and dgf = dpf Wfb (K = 32) on v_mfma_f32_32x32x2_f32 in four chains each: the A operand is the
//        image (odd row stride), the B operand torch's own [32 N][64] / [32][64] arrays, which are K-major for these products
//        (32 lanes contiguous).  Wavefronts 0 and 1 own the two column blocks of dg1, wavefront 2 both of dgf.  The ReLU masks come
//        from h1, and the results go to d_pre.
//     8. d_q: every word of the tile's rows, dx_n at the chosen action; g from h1; zeros for rows that are not live and for row T.
//   LDS of the backward kernel: NMAX = 8: 32 x 257 (state / p1 image) + 32 x 193 (h1) + 32 x 16 x 3 (x, dx, actions) + 2 x 32 x 33
//   (pf, du) + 32 x 3 (flags, dy, row offsets) words = 72 576 bytes: two workgroups per CU.  NMAX = 16: 32 x 513 for the image:
//   105 344 bytes: one workgroup per CU.  No scratch.  Six workgroup barriers.
//   A row's results depend on that row's inputs alone (an MFMA output element is a function of its A row and B column; every
//   butterfly stays inside the 32 lanes of one row), so a NaN stays in its row, and a row computes the same whatever tile it is in.
//   No cross-workgroup dependency, no device-wide synchronisation, no atomics: two calls give the same words.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/robogym_learn.h"
#include "mixer_tile.h"

namespace rg {

constexpr int MG_C_G = 160;               // columns of g: the three ReLU layers (a1, af, av)

struct MgArgs {
    rg_mixer_grad_weights w;
    rg_mixer_grad_io io;
    int32_t T;            // rows - 1
    int32_t total;        // B T flat rows
    int32_t sp;           // S padded to a multiple of 4 (qmix)
};

__device__ __forceinline__ bool mg_live(const rg_mixer_grad_io &io, int b, int t) {
    return io.mask[static_cast<size_t>(b) * io.out_pitch + t] != 0.0f;   // (a NaN is not 0.0: live)
}

// x_n of a live row (b, t): from row t of q and actions
__device__ __forceinline__ float mg_chosen(const rg_mixer_grad_io &io, int b, int t, int n) {
    const size_t an = (static_cast<size_t>(b) * io.q_pitch + t) * io.n_agents + n;
    const int a = io.actions[an];
    return static_cast<unsigned>(a) < static_cast<unsigned>(io.n_actions) ? io.q[an * io.n_actions + a] : __builtin_nanf("");
}

// none / vdn forward: one thread per row
__global__ __launch_bounds__(256) void mix_gather_forward_kernel(const MgArgs a) {
    const rg_mixer_grad_io &io = a.io;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.total) return;
    const int b = r / a.T, t = r - b * a.T, N = io.n_agents;
    const bool vdn = a.w.m.kind == RG_MIXER_VDN;
    const size_t o = static_cast<size_t>(b) * io.out_pitch + t;
    if (!mg_live(io, b, t)) {
        if (vdn) io.mixed[o] = 0.0f;
        else
            for (int n = 0; n < N; ++n) io.mixed[o * N + n] = 0.0f;
        return;
    }
    float y = 0.0f;
    for (int n = 0; n < N; ++n) {
        const float x = mg_chosen(io, b, t, n);
        if (!vdn) io.mixed[o * N + n] = x;
        y = n ? __fadd_rn(y, x) : x;
    }
    if (vdn) io.mixed[o] = y;
}

// none / vdn backward: the zero-filled scatter of row (b, t), and of row T by the thread of row T - 1
__global__ __launch_bounds__(256) void mix_gather_backward_kernel(const MgArgs a) {
    const rg_mixer_grad_io &io = a.io;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.total) return;
    const int b = r / a.T, t = r - b * a.T, N = io.n_agents, A = io.n_actions;
    const bool vdn = a.w.m.kind == RG_MIXER_VDN;
    const size_t o = static_cast<size_t>(b) * io.out_pitch + t;
    const bool live = mg_live(io, b, t);
    const size_t an = (static_cast<size_t>(b) * io.q_pitch + t) * N;
    const float dy = (live && vdn) ? io.d_mixed[o] : 0.0f;
    for (int n = 0; n < N; ++n) {
        const int act = live ? io.actions[an + n] : -1;
        const float d = !live ? 0.0f : (vdn ? dy : io.d_mixed[o * N + n]);
        float *dst = io.d_q + (an + n) * A;
        for (int c = 0; c < A; ++c) dst[c] = c == act ? d : 0.0f;
    }
    if (t == a.T - 1) {
        float *dst = io.d_q + (an + N) * A;   // row T
        for (int c = 0; c < N * A; ++c) dst[c] = 0.0f;
    }
}

// Steps 2 and 3 of td_qmix_kernel for a tile whose state rows are rows t: x and the state rows to LDS, then the first layers of the
// four hypernetworks to h1 (ReLU applied, hyper_b_1 linear).  flags[i] == 2: live.  Ends behind the barrier that completes h1 (and
// after which st is dead).  acts: where the tile's actions go as well, or null.
__device__ __forceinline__ void mix_first_layers(const MgArgs &a, const int *flags, float *st, float *h1, float *aq, int *acts) {
    const rg_mixer_grad_io &io = a.io;
    const rg_mixer_weights &m = a.w.m;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = io.n_agents, S = N * io.obs_dim, sp = a.sp, sps = sp + 1, T = a.T;
    const int base = blockIdx.x * TD_TM;
    for (int idx = tid; idx < TD_TM * N; idx += TD_NT) {
        const int i = idx / N, n = idx - i * N;
        float v = 0.0f;
        int act = -1;
        if (flags[i] == 2) {
            const int r = base + i, b = r / T, t = r - b * T;
            v = mg_chosen(io, b, t, n);
            if (acts) act = io.actions[(static_cast<size_t>(b) * io.q_pitch + t) * N + n];
        }
        aq[i * RG_MAX_AGENTS + n] = v;
        if (acts) acts[i * RG_MAX_AGENTS + n] = act;
    }
    for (int i = wave; i < TD_TM; i += TD_NT / 64) {
        const bool on = flags[i] == 2;
        const int r = base + i, b = on ? r / T : 0, t = on ? r - b * T : 0;
        const float *src = io.obs + (static_cast<size_t>(b) * io.obs_pitch + t) * S;
        for (int k = lane; k < sp; k += 64) st[i * sps + k] = (on && k < S) ? src[k] : 0.0f;
    }
    __syncthreads();

    // the first layers: blocks `wave` and `wave + 3` of the six (td_targets.h step 3), one after the other, each in FOUR chains, the
    // k steps dealt out in turn and the chains added in pairs at the end: a quarter of the length of one fmaf chain, and 64
    // accumulator registers at a time
    const int lr = lane & 31, lh = lane >> 5;
    const float *arow = st + lr * sps + lh;
#pragma nounroll
    for (int half = 0; half < 2; ++half) {
        const int col = 32 * wave + lr + 96 * half;
        const float *wk = m.w_in + lh * TD_C1 + col;
        f32x16 ch[4] = {{0}, {0}, {0}, {0}};
        int k = 0;
        for (; k + 8 <= sp; k += 8)
#pragma unroll
            for (int c = 0; c < 4; ++c) ch[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[k + 2 * c], wk[static_cast<size_t>(k + 2 * c) * TD_C1], ch[c], 0, 0, 0);
        if (k < sp)   // (sp is a multiple of 4: two k steps are left)
#pragma unroll
            for (int c = 0; c < 2; ++c) ch[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[k + 2 * c], wk[static_cast<size_t>(k + 2 * c) * TD_C1], ch[c], 0, 0, 0);
        const f32x16 acc = (ch[0] + ch[1]) + (ch[2] + ch[3]);
        const float bias = m.b_in[col];
        const bool relu = col < TD_COL_B1;   // hyper_b_1 is one linear layer: no ReLU behind it (wave-uniform: a whole block)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int row = (j & 3) + 8 * (j >> 2) + 4 * lh;
            const float x = acc[j] + bias;
            h1[row * TD_H1S + col] = (!relu || x > 0.0f) ? x : (x != x ? x : 0.0f);
        }
    }
    __syncthreads();   // h1 is complete, and every read of st is done
}

// One second-layer block [32 x 64] [64 x 32] + bias (td_targets.h step 4): block blk < N is p1[:, blk, :], block N is pf.
__device__ __forceinline__ f32x16 mix_second_block(const rg_mixer_weights &m, const float *h1, int blk, int N, int lr, int lh, float *bias) {
    const bool is_w1 = blk < N;
    const int ldb = is_w1 ? N * TD_EMBED : TD_EMBED;
    const float *wb = (is_w1 ? m.w_w1 + blk * TD_EMBED : m.w_wf) + lh * ldb + lr;
    const float *arow = h1 + lr * TD_H1S + (is_w1 ? 0 : TD_COL_WF) + lh;
    f32x16 ch[4] = {{0}, {0}, {0}, {0}};   // four chains, as the first layers
#pragma unroll 2
    for (int k = 0; k < TD_HYPER; k += 8)
#pragma unroll
        for (int c = 0; c < 4; ++c) ch[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[k + 2 * c], wb[static_cast<size_t>(k + 2 * c) * ldb], ch[c], 0, 0, 0);
    const f32x16 acc = (ch[0] + ch[1]) + (ch[2] + ch[3]);
    *bias = is_w1 ? m.b_w1[blk * TD_EMBED + lr] : m.b_wf[lr];
    return acc;
}

// elu in binary64 (what lies behind the matrix products is a few thousand operations per tile: it is done in binary64 and rounded once)
__device__ __forceinline__ double mix_elu(double u) { return u > 0.0 ? u : expm1(u); }

// the tile's row flags from the mask: -1 behind the last row, 0 masked, 2 live; returns whether the tile has a live row
__device__ __forceinline__ int mix_flags(const MgArgs &a, int *flags, int *mine_out) {
    const int tid = threadIdx.x, base = blockIdx.x * TD_TM;
    int mine = -1;
    if (tid < TD_TM) {
        const int r = base + tid;
        if (r < a.total) {
            const int b = r / a.T;
            mine = mg_live(a.io, b, r - b * a.T) ? 2 : 0;
        }
        flags[tid] = mine;
    }
    *mine_out = mine;
    return __syncthreads_or(mine == 2);
}

// qmix forward: one workgroup per tile of 32 rows
__global__ __launch_bounds__(TD_NT) void mix_qmix_forward_kernel(const MgArgs a) {
    // the state rows; from step 4 on the partial sums of u [3][32][33] in binary64 and wf [32][33]
    __shared__ __attribute__((aligned(16))) float st[TD_TM * (TD_MAX_SP + 1)];
    __shared__ float h1[TD_TM * TD_H1S];
    __shared__ float aq[TD_TM * RG_MAX_AGENTS];
    __shared__ int flags[TD_TM];
    static_assert((3 * TD_TM * TD_PS) * 2 + TD_TM * TD_PS <= TD_TM * (TD_MAX_SP + 1), "the partial sums and wf fit the state's image");
    const rg_mixer_grad_io &io = a.io;
    const rg_mixer_weights &m = a.w.m;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = io.n_agents, T = a.T;
    const int base = blockIdx.x * TD_TM;

    int mine;
    if (!mix_flags(a, flags, &mine)) {
        if (mine >= 0) {
            const int r = base + tid, b = r / T;
            io.mixed[static_cast<size_t>(b) * io.out_pitch + (r - b * T)] = 0.0f;
        }
        return;
    }
    mix_first_layers(a, flags, st, h1, aq, nullptr);

    const int lr = lane & 31, lh = lane >> 5;
    double *part = reinterpret_cast<double *>(st);
    float *wf = st + 2 * 3 * TD_TM * TD_PS;
    {
        double hid[16] = {0};
        for (int blk = wave; blk <= N; blk += TD_NT / 64) {
            float bias;
            const f32x16 acc = mix_second_block(m, h1, blk, N, lr, lh, &bias);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int row = (j & 3) + 8 * (j >> 2) + 4 * lh;
                const float w = __builtin_fabsf(acc[j] + bias);
                if (blk < N) hid[j] += static_cast<double>(aq[row * RG_MAX_AGENTS + blk]) * w;
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

    for (int idx = tid; idx < TD_TM * TD_EMBED; idx += TD_NT) {
        const int row = idx >> 5, e = idx & 31;
        double h = (part[row * TD_PS + e] + part[(TD_TM + row) * TD_PS + e]) + part[(2 * TD_TM + row) * TD_PS + e];
        h = mix_elu(h + h1[row * TD_H1S + TD_COL_B1 + e]);
        double s = h * wf[row * TD_PS + e] + static_cast<double>(m.w_v[e]) * h1[row * TD_H1S + TD_COL_V + e];
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) s += __shfl_xor(s, d, 32);
        const int flag = flags[row];
        if (flag < 0 || e != 0) continue;
        const int r = base + row, b = r / T;
        io.mixed[static_cast<size_t>(b) * io.out_pitch + (r - b * T)] = flag == 2 ? static_cast<float>(s + m.b_v[0]) : 0.0f;
    }
}

// qmix backward: one workgroup per tile of 32 rows, for up to NMAX agents
template <int NMAX>
__global__ __launch_bounds__(TD_NT) void mix_qmix_backward_kernel(const MgArgs a) {
    constexpr int PWS = TD_EMBED * NMAX + 1;        // row stride of the p1 image (odd); 32 NMAX + 1 >= TD_MAX_SP + 1 for NMAX >= 8
    static_assert(PWS >= TD_MAX_SP + 1, "the p1 image holds the state rows before it");
    __shared__ float pw[TD_TM * PWS];               // the state rows; from step 4 on p1 (signed), from step 6 on dp1
    __shared__ float h1[TD_TM * TD_H1S];
    __shared__ float aq[TD_TM * RG_MAX_AGENTS];     // x
    __shared__ float dxs[TD_TM * RG_MAX_AGENTS];    // dx
    __shared__ int acts[TD_TM * RG_MAX_AGENTS];     // the actions of the live rows (-1: the row is not live)
    __shared__ float pfs[TD_TM * TD_PS];            // pf (signed), from step 5 on dpf
    __shared__ float dus[TD_TM * TD_PS];            // du
    __shared__ int flags[TD_TM];
    __shared__ float dys[TD_TM];                    // dy of the live rows, 0.0 for the others
    __shared__ int aux[TD_TM];                      // b aux_pitch + t: the row in d_pre, d_p2 and g
    const rg_mixer_grad_io &io = a.io;
    const rg_mixer_weights &m = a.w.m;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = io.n_agents, A = io.n_actions, T = a.T, NE = N * TD_EMBED, P2 = NE + TD_EMBED;
    const int base = blockIdx.x * TD_TM;

    // 1. flags, dy, where the rows go
    int mine;
    const int live = mix_flags(a, flags, &mine);
    if (tid < TD_TM) {
        const int r = base + tid, b = mine >= 0 ? r / T : 0, t = r - b * T;
        dys[tid] = mine == 2 ? io.d_mixed[static_cast<size_t>(b) * io.out_pitch + t] : 0.0f;
        aux[tid] = mine >= 0 ? b * io.aux_pitch + t : -1;
    }
    if (!live) {
        __syncthreads();   // aux
        for (int i = 0; i < TD_TM; ++i) {
            const int ar = aux[i];
            if (ar < 0) break;
            const int r = base + i, b = r / T, t = r - b * T, both = t == T - 1 ? 2 : 1;   // (row T behind row T - 1: contiguous)
            float *dq = io.d_q + (static_cast<size_t>(b) * io.q_pitch + t) * N * A;
            for (int k = tid; k < both * N * A; k += TD_NT) dq[k] = 0.0f;
            for (int k = tid; k < both * TD_C1; k += TD_NT) io.d_pre[static_cast<size_t>(ar) * TD_C1 + k] = 0.0f;
            for (int k = tid; k < both * P2; k += TD_NT) io.d_p2[static_cast<size_t>(ar) * P2 + k] = 0.0f;
            for (int k = tid; k < both * MG_C_G; k += TD_NT) io.g[static_cast<size_t>(ar) * MG_C_G + k] = 0.0f;
        }
        return;
    }

    // 2., 3. as the forward kernel
    mix_first_layers(a, flags, pw, h1, aq, acts);

    // 4. the second layers, signed, to the image
    const int lr = lane & 31, lh = lane >> 5;
    for (int blk = wave; blk <= N; blk += TD_NT / 64) {
        float bias;
        const f32x16 acc = mix_second_block(m, h1, blk, N, lr, lh, &bias);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int row = (j & 3) + 8 * (j >> 2) + 4 * lh;
            const float p = acc[j] + bias;
            if (blk < N) pw[row * PWS + blk * TD_EMBED + lr] = p;
            else pfs[row * TD_PS + lr] = p;
        }
    }
    __syncthreads();

    // 5. per row: hidden as the forward kernel sums it, du, dpf, dav, d_b1
    for (int idx = tid; idx < TD_TM * TD_EMBED; idx += TD_NT) {
        const int row = idx >> 5, e = idx & 31;
        double part[3] = {0.0, 0.0, 0.0};
        for (int n0 = 0; n0 < N; n0 += 3)
#pragma unroll
            for (int w = 0; w < 3; ++w)
                if (n0 + w < N) part[w] += static_cast<double>(aq[row * RG_MAX_AGENTS + n0 + w]) * __builtin_fabsf(pw[row * PWS + (n0 + w) * TD_EMBED + e]);
        const double u = ((part[0] + part[1]) + part[2]) + h1[row * TD_H1S + TD_COL_B1 + e];
        const double hidden = mix_elu(u);
        const float pf = pfs[row * TD_PS + e], dy = dys[row];
        const double d_hidden = static_cast<double>(dy) * __builtin_fabsf(pf), d_wf = dy * hidden;
        const float du = static_cast<float>(d_hidden * (u > 0.0 ? 1.0 : hidden + 1.0));
        const float sf = pf > 0.0f ? 1.0f : (pf < 0.0f ? -1.0f : (pf != pf ? pf : 0.0f));
        const float dpf = static_cast<float>(d_wf) * sf;
        const bool on = flags[row] == 2;
        dus[row * TD_PS + e] = du;
        pfs[row * TD_PS + e] = on ? dpf : 0.0f;
        const int ar = aux[row];
        if (ar < 0) continue;
        const float gv = h1[row * TD_H1S + TD_COL_V + e];
        const float dav = gv > 0.0f ? dy * m.w_v[e] : (gv != gv ? gv : 0.0f);
        io.d_pre[static_cast<size_t>(ar) * TD_C1 + TD_COL_V + e] = on ? dav : 0.0f;
        io.d_pre[static_cast<size_t>(ar) * TD_C1 + TD_COL_B1 + e] = on ? du : 0.0f;
        io.d_p2[static_cast<size_t>(ar) * P2 + NE + e] = on ? dpf : 0.0f;
    }
    __syncthreads();

    // 6. per (row, n): dx_n, and dp1 over p1
    for (int idx = tid; idx < TD_TM * NE; idx += TD_NT) {   // (whole groups of 32 lanes)
        const int rn = idx >> 5, e = idx & 31, row = rn / N, n = rn - row * N;
        const float p = pw[row * PWS + n * TD_EMBED + e], du = dus[row * TD_PS + e], x = aq[row * RG_MAX_AGENTS + n];
        double s = static_cast<double>(du) * __builtin_fabsf(p);
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) s += __shfl_xor(s, d, 32);
        const float sg = p > 0.0f ? 1.0f : (p < 0.0f ? -1.0f : (p != p ? p : 0.0f));
        const bool on = flags[row] == 2;
        const float dp = on ? (x * du) * sg : 0.0f;
        pw[row * PWS + n * TD_EMBED + e] = dp;
        if (e == 0) dxs[row * RG_MAX_AGENTS + n] = static_cast<float>(s);
        const int ar = aux[row];
        if (ar >= 0) io.d_p2[static_cast<size_t>(ar) * P2 + n * TD_EMBED + e] = dp;
    }
    __syncthreads();

    // 7. dg1 = dp1 W1b (wavefronts 0, 1: one block of 32 columns each), dgf = dpf Wfb (wavefront 2: both blocks)
    for (int blk = (wave < 2 ? wave : 2); blk < (wave < 2 ? wave + 1 : 4); ++blk) {
        const bool is_w1 = blk < 2;
        const int K = is_w1 ? NE : TD_EMBED, cb = (blk & 1) * 32;
        const float *wb = (is_w1 ? a.w.w1b : a.w.wfb) + lh * TD_HYPER + cb + lr;
        const float *arow = (is_w1 ? pw + lr * PWS : pfs + lr * TD_PS) + lh;
        f32x16 ch[4] = {{0}, {0}, {0}, {0}};
        for (int k = 0; k < K; k += 8)   // (K is a multiple of 32)
#pragma unroll
            for (int c = 0; c < 4; ++c) ch[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[k + 2 * c], wb[static_cast<size_t>(k + 2 * c) * TD_HYPER], ch[c], 0, 0, 0);
        const f32x16 acc = (ch[0] + ch[1]) + (ch[2] + ch[3]);
        const int col = (is_w1 ? 0 : TD_COL_WF) + cb + lr;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int row = (j & 3) + 8 * (j >> 2) + 4 * lh;
            const int ar = aux[row];
            const float gg = h1[row * TD_H1S + col];
            const float da = gg > 0.0f ? acc[j] : (gg != gg ? gg : 0.0f);
            if (ar >= 0) io.d_pre[static_cast<size_t>(ar) * TD_C1 + col] = flags[row] == 2 ? da : 0.0f;
        }
    }

    // 8. d_q and g of the tile's rows, and the zeros of row T
    for (int i = 0; i < TD_TM; ++i) {
        const int ar = aux[i];
        if (ar < 0) break;
        const int r = base + i, b = r / T, t = r - b * T;
        const bool on = flags[i] == 2;
        float *dq = io.d_q + (static_cast<size_t>(b) * io.q_pitch + t) * N * A;
        for (int k = tid; k < N * A; k += TD_NT) {
            const int n = k / A, c = k - n * A;
            dq[k] = (on && c == acts[i * RG_MAX_AGENTS + n]) ? dxs[i * RG_MAX_AGENTS + n] : 0.0f;
        }
        for (int k = tid; k < MG_C_G; k += TD_NT) io.g[static_cast<size_t>(ar) * MG_C_G + k] = on ? h1[i * TD_H1S + k] : 0.0f;
        if (t == T - 1) {
            for (int k = tid; k < N * A; k += TD_NT) dq[N * A + k] = 0.0f;
            for (int k = tid; k < TD_C1; k += TD_NT) io.d_pre[static_cast<size_t>(ar + 1) * TD_C1 + k] = 0.0f;
            for (int k = tid; k < P2; k += TD_NT) io.d_p2[static_cast<size_t>(ar + 1) * P2 + k] = 0.0f;
            for (int k = tid; k < MG_C_G; k += TD_NT) io.g[static_cast<size_t>(ar + 1) * MG_C_G + k] = 0.0f;
        }
    }
}

}  // namespace rg
