// gru_scan.h -- the rule of rg_gru_scan_forward / rg_gru_scan_backward (include/robogym_learn.h), stated once, and their kernels: the
// sequential part of a recurrent actor's pass WITH gradients over a whole episode batch (instantiated by robogym_gru_scan.hip).
// DESIGN.md section 4 "Trainable actor" is the same rule.
//
// EPyMARL trains its actor with mac.forward(batch, t) for t = 0 .. L under autograd: `rows` x (fc1, GRUCell, fc2) launches forward,
// and the same chain replayed backwards.  Of that, fc1, the input half of the GRU (gi = relu(fc1(obs)) W_ih^T + b_ih), fc2 and
// every weight gradient are products over ALL B rows N rows at once, which the caller leaves to a GEMM library.  What is left is
// sequential in t, and is what these two launches compute.
//
// GRU scan rule.
//   torch.nn.GRUCell's recurrence, in float32 throughout, with H = hidden_dim in {64, 128} and the gates in torch's order r, z, n.
//   Flat row (b, n), agent n of episode b, is independent of every other flat row.  The weights are w_hh [A][3H][H] and b_hh
//   [A][3H] with A = 1 (every agent uses set 0) or A = N (agent n uses set n).
//   Forward.
//   - Inputs: gi [B][gi_pitch][N][3H]; hidden_in [B][N][H] or NULL, meaning zeros.  h_{-1} = hidden_in.
//   - For t = 0 .. rows-1 in order:
//       gh = h_{t-1} W_hh^T + b_hh
//       r = sigmoid(gi_r + gh_r)
//       z = sigmoid(gi_z + gh_z)
//       n = tanh(gi_n + r gh_n)
//       h_t = (1 - z) n + z h_{t-1}
//   - Outputs: h [B][save_pitch][N][H], every h_t; when gates is not NULL, gates [B][save_pitch][N][4H] = (r, z, n, gh_n) of every
//     step; when hidden_out is not NULL, hidden_out [B][N][H] = h_{rows-1}.
//   - There are no masks: every one of the rows steps is computed.  Row 0 is read as stored.
//   Backward.
//   - Inputs: the h and gates a forward launch saved, hidden_in as it was given to it, w_hh, dh_ext [B][grad_pitch][N][H] (the
//     gradient that reaches h_t from outside the recurrence), and d_hidden_out [B][N][H] or NULL, meaning zeros.
//   - carry = d_hidden_out.  For t = rows-1 .. 0 in order, with r, z, n, gh_n of step t and h_{t-1} (hidden_in at t = 0):
//       dh = dh_ext_t + carry
//       dn = dh (1 - z)
//       dz = dh (h_{t-1} - n)
//       da_n = dn (1 - n n)
//       da_r = (da_n gh_n) r (1 - r)
//       da_z = dz z (1 - z)
//       dgi_t = (da_r, da_z, da_n)
//       dghn_t = da_n r
//       carry = dh z + (da_r, da_z, dghn_t) W_hh
//   - Outputs: dgi [B][grad_pitch][N][3H]; dghn [B][grad_pitch][N][H] (the gradient of gh is (da_r, da_z, dghn): its r and z
//     thirds are dgi's); when d_hidden_in is not NULL, d_hidden_in [B][N][H] = the last carry.
//   Both.
//   - Every product with W_hh is a float32 sum in an order of the kernel's choosing, which is fixed: no atomics, so two calls give
//     the same words.  Every other operation is the single float32 operation written above, not contracted.
//   - sigmoid(x) = 1 / (1 + exp(-x)) and tanh(x) = sign(x) (-e / (2 + e)) with e = expm1(-2 |x|): neither overflows into a NaN, so
//     finite inputs give finite outputs.
//   - A row's results are a function of that row's inputs and its weight set alone: a NaN stays in its flat row, and a row
//     computes the same words whatever tile or neighbours it is computed with.
//   - Rows behind rows, and the pitch padding of every output, are not touched.
// End of the rule.
//
// The kernels.  One workgroup of H / 32 wavefronts owns a tile of 32 flat rows for the whole call -- with shared weights 32
// consecutive flat rows of [B N], with one weight set per agent 32 episodes of one agent (unroll_kernel's tiling) -- and walks the
// time steps; there are no cross-workgroup dependencies and no device-wide synchronisation.  Both products run on
// v_mfma_f32_32x32x2_f32 (the exact f32 matrix instruction: a k-ordered fmaf chain, a 32 x 32 block in 16 accumulator registers,
// ONE register per operand and k step), in several chains with the k steps dealt out in turn: the backward product in FOUR, added
// as (c0 + c1) + (c2 + c3) as nstep_returns.h does; each of the forward launch's three products in TWO (c0 + c1) -- six independent
// accumulators in flight, and with four chains per gate the twelve blocks beside the 3 H / 2 weight registers and the step's gi
// words no longer fit the register file (the compiler spilled 250 registers per lane at H = 128, 66 at H = 64).
//   Forward: wavefront w owns the hidden columns 32 w .. 32 w + 31 of ALL THREE gates, so the gate arithmetic happens on the
//   accumulators with no exchange: lane (lr, lh) holds column 32 w + lr of the tile rows (j & 3) + 8 (j >> 2) + 4 lh, j < 16.  Its
//   three [H x 32] blocks of W_hh^T sit IN REGISTERS for the whole call (3 H / 2 per lane: 192 at H = 128), gathered once from
//   torch's layout (or read from the transposed copy when the caller has one).  The A operand is the tile's h_{t-1} in LDS
//   ([32][H + 1]: the odd row stride keeps the 32 rows on 32 banks), double-buffered, so a step needs ONE barrier.  The step's gi
//   words are loaded at the head of the step and first used behind its 3 H / 2 matrix instructions.
//   Backward: the same ownership of columns.  The carry never leaves the accumulator layout (dh z is elementwise, and the product's
//   block lands where it is needed), so only (da_r, da_z, dghn) is staged, [32][3 H + 1] in LDS, double-buffered: ONE barrier per
//   step.  The B operand is W_hh as torch stores it (32 lanes read 32 consecutive words), 3 H / 2 registers per lane again.  The
//   words of step t - 1 (dh_ext, the four gates, h_{t-2}) are loaded under step t's matrix instructions.
//   A workgroup is one wavefront per SIMD with up to 512 registers per lane (vector + accumulator): one workgroup per CU.  The scan
//   is a latency chain -- 3 H / 2 dependent-rate matrix instructions per step and wavefront -- so occupancy would not help it.
//   Rows of a ragged tile behind its last row are computed on row 0's addresses and never stored.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/robogym_learn.h"

namespace rg {

constexpr int GS_TM = 32;   // flat rows of a tile

struct GsArgs {
    rg_gru_scan_weights w;
    rg_gru_scan_io io;
};

using gs_f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ int gs_acc_row(int j, int lh) { return (j & 3) + 8 * (j >> 2) + 4 * lh; }
__device__ __forceinline__ float gs_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float gs_tanh(float x) {
    const float e = expm1f(-2.0f * fabsf(x));   // in [-1, 0]
    return copysignf(-e / (2.0f + e), x);
}

// The tile of this workgroup: its weight set, and for tile row i < 32 the flat row r = b N + n and the row numbers of (b, t = 0, n)
// under the two pitches the kernel uses (rq[0], rq[1], rq[2]); a row behind the tile's last takes row 0's.  -> the valid rows
__device__ __forceinline__ int gs_tile(const rg_gru_scan_io &io, int n_sets, int pitch1, int pitch2, int (*rq)[GS_TM], int &set) {
    const int B = io.num_episodes, N = io.n_agents;
    const bool shared = n_sets == 1;
    int base;
    set = 0;
    if (shared) {
        base = blockIdx.x * GS_TM;
    } else {
        const int tiles_per_agent = (B + GS_TM - 1) / GS_TM;
        set = blockIdx.x / tiles_per_agent;
        base = (blockIdx.x - set * tiles_per_agent) * GS_TM;
    }
    const int left = (shared ? B * N : B) - base, nrows = left < GS_TM ? left : GS_TM;
    if (threadIdx.x < GS_TM) {
        const int i = static_cast<int>(threadIdx.x) < nrows ? threadIdx.x : 0;
        const int r = shared ? base + i : (base + i) * N + set, b = r / N, n = r - b * N;
        rq[0][threadIdx.x] = r;
        rq[1][threadIdx.x] = b * pitch1 * N + n;
        rq[2][threadIdx.x] = b * pitch2 * N + n;
    }
    return nrows;
}

template <int H>
__attribute__((amdgpu_waves_per_eu(1, 1)))   // one wavefront per SIMD: the whole register file
__global__ __launch_bounds__(2 * H) void gru_scan_forward_kernel(const GsArgs a) {
    constexpr int NT = 2 * H, HS = H + 1, KS = H / 2;   // threads, the LDS row stride, k steps of one gate's product
    __shared__ float hb[2][GS_TM * HS];                 // h_{t-1} and h_t of the tile
    __shared__ int rq[3][GS_TM];                        // flat row; row of (b, 0, n) in gi; in h and gates
    const rg_gru_scan_io &io = a.io;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, lh = lane >> 5, col = 32 * wave + lr;
    const int N = io.n_agents, rows = io.rows;
    int set;
    const int nrows = gs_tile(io, a.w.n_sets, io.gi_pitch, io.save_pitch, rq, set);

    // W_hh^T's three [H x 32] blocks of this wavefront: k step s of lane (lr, lh) is w_hh[g H + col][2 s + lh]
    float wr[3][KS], bias[3];
    {
        const size_t wset = static_cast<size_t>(set) * 3 * H * H;
        if (a.w.w_hh_t) {
            const float *wt = a.w.w_hh_t + wset;
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int s = 0; s < KS; ++s) wr[g][s] = wt[(2 * s + lh) * 3 * H + g * H + col];
        } else {
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                const float4 *row = reinterpret_cast<const float4 *>(a.w.w_hh + wset + static_cast<size_t>(g * H + col) * H);
#pragma unroll
                for (int q = 0; q < H / 4; ++q) {
                    const float4 v = row[q];
                    wr[g][2 * q] = lh ? v.y : v.x;
                    wr[g][2 * q + 1] = lh ? v.w : v.z;
                }
            }
        }
#pragma unroll
        for (int g = 0; g < 3; ++g) bias[g] = a.w.b_hh[set * 3 * H + g * H + col];
    }
    __syncthreads();   // rq
    for (int idx = tid; idx < GS_TM * H; idx += NT) {
        const int i = idx / H, k = idx - i * H;
        hb[0][i * HS + k] = (io.hidden_in && i < nrows) ? io.hidden_in[static_cast<size_t>(rq[0][i]) * H + k] : 0.0f;
    }
    __syncthreads();

    int cur = 0;
    for (int t = 0; t < rows; ++t) {
        const float *hc = hb[cur];
        float *hn = hb[cur ^ 1];
        // the step's gi words (first used behind the matrix instructions)
        float gr[16], gz[16], gn[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float *p = io.gi + static_cast<size_t>(rq[1][gs_acc_row(j, lh)] + t * N) * (3 * H) + col;
            gr[j] = p[0], gz[j] = p[H], gn[j] = p[2 * H];
        }
        gs_f32x16 acc[3];
        {
            const float *arow = hc + lr * HS + lh;
            gs_f32x16 c[3][2];
#pragma unroll
            for (int g = 0; g < 3; ++g) c[g][0] = c[g][1] = gs_f32x16{0};
#pragma unroll
            for (int s = 0; s < KS; s += 2) {
                const float a0 = arow[2 * s], a1 = arow[2 * s + 2];
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    c[g][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, wr[g][s], c[g][0], 0, 0, 0);
                    c[g][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, wr[g][s + 1], c[g][1], 0, 0, 0);
                }
            }
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[g] = c[g][0] + c[g][1];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int i = gs_acc_row(j, lh);
            const float r = gs_sigmoid(gr[j] + (acc[0][j] + bias[0]));
            const float z = gs_sigmoid(gz[j] + (acc[1][j] + bias[1]));
            const float ghn = acc[2][j] + bias[2];
            const float n = gs_tanh(gn[j] + r * ghn);
            const float hnew = (1.0f - z) * n + z * hc[i * HS + col];
            hn[i * HS + col] = hnew;
            if (i < nrows) {
                const size_t row = static_cast<size_t>(rq[2][i] + t * N);
                io.h[row * H + col] = hnew;
                if (io.gates) {
                    float *gp = io.gates + row * (4 * H) + col;
                    gp[0] = r, gp[H] = z, gp[2 * H] = n, gp[3 * H] = ghn;
                }
            }
        }
        __syncthreads();   // h_t is complete, and every read of h_{t-1} is done
        cur ^= 1;
    }
    if (io.hidden_out) {
        for (int idx = tid; idx < GS_TM * H; idx += NT) {
            const int i = idx / H, k = idx - i * H;
            if (i < nrows) io.hidden_out[static_cast<size_t>(rq[0][i]) * H + k] = hb[cur][i * HS + k];
        }
    }
}

template <int H>
__attribute__((amdgpu_waves_per_eu(1, 1)))
__global__ __launch_bounds__(2 * H) void gru_scan_backward_kernel(const GsArgs a) {
    constexpr int GS = 3 * H + 1, KS = 3 * H / 2;   // the LDS row stride, k steps of the product
    __shared__ float dg[2][GS_TM * GS];             // (da_r, da_z, dghn) of the tile, of this step and the one before
    __shared__ int rq[3][GS_TM];                    // flat row; row of (b, 0, n) in h and gates; in dh_ext, dgi and dghn
    const rg_gru_scan_io &io = a.io;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, lh = lane >> 5, col = 32 * wave + lr;
    const int N = io.n_agents, rows = io.rows;
    int set;
    const int nrows = gs_tile(io, a.w.n_sets, io.save_pitch, io.grad_pitch, rq, set);

    // W_hh's [3H x 32] block of this wavefront: k step s of lane (lr, lh) is w_hh[2 s + lh][col]
    float wr[KS];
    {
        const float *wb = a.w.w_hh + static_cast<size_t>(set) * 3 * H * H + lh * H + col;
#pragma unroll
        for (int s = 0; s < KS; ++s) wr[s] = wb[2 * s * H];
    }
    __syncthreads();   // rq

    float carry[16];
#pragma unroll
    for (int j = 0; j < 16; ++j)
        carry[j] = io.d_hidden_out ? io.d_hidden_out[static_cast<size_t>(rq[0][gs_acc_row(j, lh)]) * H + col] : 0.0f;

    // the words of one step in the accumulator layout: dh_ext, r, z, n, gh_n, h_{t-1}
    struct Step {
        float dhe[16], r[16], z[16], n[16], ghn[16], hp[16];
    };
    auto load = [&](int t, Step &s) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int i = gs_acc_row(j, lh);
            const size_t srow = static_cast<size_t>(rq[1][i] + t * N);
            s.dhe[j] = io.dh_ext[static_cast<size_t>(rq[2][i] + t * N) * H + col];
            const float *gp = io.gates + srow * (4 * H) + col;
            s.r[j] = gp[0], s.z[j] = gp[H], s.n[j] = gp[2 * H], s.ghn[j] = gp[3 * H];
        }
        // h_{t-1}: one uniform choice around the sixteen loads, not one per load
        const bool stored = t > 0 || io.hidden_in;
        const float *hsrc = t > 0 ? io.h : io.hidden_in;
#pragma unroll
        for (int j = 0; j < 16; ++j) s.hp[j] = 0.0f;
        if (stored) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int i = gs_acc_row(j, lh);
                const size_t row = t > 0 ? static_cast<size_t>(rq[1][i] + (t - 1) * N) : static_cast<size_t>(rq[0][i]);
                s.hp[j] = hsrc[row * H + col];
            }
        }
    };
    Step now;
    load(rows - 1, now);
    for (int t = rows - 1; t >= 0; --t) {
        float *buf = dg[t & 1];
        float cz[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int i = gs_acc_row(j, lh);
            const float r = now.r[j], z = now.z[j], n = now.n[j];
            const float dh = now.dhe[j] + carry[j];
            const float dn = dh * (1.0f - z);
            const float dz = dh * (now.hp[j] - n);
            const float da_n = dn * (1.0f - n * n);
            const float da_r = ((da_n * now.ghn[j]) * r) * (1.0f - r);
            const float da_z = (dz * z) * (1.0f - z);
            const float dghn = da_n * r;
            cz[j] = dh * z;
            buf[i * GS + col] = da_r, buf[i * GS + H + col] = da_z, buf[i * GS + 2 * H + col] = dghn;
            if (i < nrows) {
                const size_t row = static_cast<size_t>(rq[2][i] + t * N);
                float *gp = io.dgi + row * (3 * H) + col;
                gp[0] = da_r, gp[H] = da_z, gp[2 * H] = da_n;
                io.dghn[row * H + col] = dghn;
            }
        }
        __syncthreads();   // the step's staging block is complete (the one before is read no more: a step later than its product)
        Step next;
        if (t > 0) load(t - 1, next);
        else next = now;
        {
            const float *arow = buf + lr * GS + lh;
            gs_f32x16 c0 = {0}, c1 = {0}, c2 = {0}, c3 = {0};
#pragma unroll
            for (int s = 0; s < KS; s += 4) {
                c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * s], wr[s], c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * s + 2], wr[s + 1], c1, 0, 0, 0);
                c2 = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * s + 4], wr[s + 2], c2, 0, 0, 0);
                c3 = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * s + 6], wr[s + 3], c3, 0, 0, 0);
            }
            const gs_f32x16 acc = (c0 + c1) + (c2 + c3);
#pragma unroll
            for (int j = 0; j < 16; ++j) carry[j] = cz[j] + acc[j];
        }
        now = next;
    }
    if (io.d_hidden_in) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int i = gs_acc_row(j, lh);
            if (i < nrows) io.d_hidden_in[static_cast<size_t>(rq[0][i]) * H + col] = carry[j];
        }
    }
}

}  // namespace rg
