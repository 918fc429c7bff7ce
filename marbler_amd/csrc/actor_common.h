// actor_common.h -- what the actor's tile computation (actor_body.inc) needs around it: the MFMA operand types, the plane splits,
// the LDS swizzles, the gate nonlinearities and the argument block.  Shared by actor_mfma.hip and policy_rollout.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/robogym.h"
#include "probes/actor_diag.h"   // RG_ASTAMP* / RG_AKEEP*: phase stamps of the diagnostic builds, nothing in the shipped one

namespace rg {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- float32 carried as three bfloat16 planes (gru_packed == 2; round 4).
// v_mfma_f32_32x32x2_f32 costs 64 cycles for K = 2; v_mfma_f32_32x32x16_bf16 costs 32 cycles for K = 16: 16 x the rate.  A
// float32 value is EXACTLY hi + mid + lo with hi = the top 16 bits of x (a bfloat16 by truncation), mid = the top 16 bits of
// x - hi, lo = the top 16 bits of x - hi - mid (what is dropped is below 2^-24 |x|).  A product x w is then the sum of nine
// plane products, of which the six of order >= 2^-16 are computed -- hh, hm, mh, hl, lh, mm, each exact in the MFMA's float32
// accumulator -- and the three of order 2^-24 are left out: 6 / 16 of the float32 MFMA time for an error BELOW that of a
// float32 dot product's own roundings (measured on 4096 x 128 x 384 random operands: 3.6e-7 against the exact product, a
// float32 GEMM 2.5e-6).  Same exponent range as float32: nothing can overflow or flush that float32 would not.
// split8: eight consecutive k values of one row -> the three planes as MFMA operands (element e of a plane = k0 + e)
__device__ __forceinline__ void split8(const float4 &lo4, const float4 &hi4, bf16x8 &ph, bf16x8 &pm, bf16x8 &pl) {
    const float x[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
    uint32_t bh[8], bm[8], bl[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        bh[e] = __builtin_bit_cast(uint32_t, x[e]) & 0xFFFF0000u;
        const float r1 = x[e] - __builtin_bit_cast(float, bh[e]);   // exact
        bm[e] = __builtin_bit_cast(uint32_t, r1) & 0xFFFF0000u;
        const float r2 = r1 - __builtin_bit_cast(float, bm[e]);     // exact
        bl[e] = __builtin_bit_cast(uint32_t, r2);                    // (truncated by the packing below)
    }
    u32x4 h, m, l;
#pragma unroll
    for (int q = 0; q < 4; ++q) {   // two bfloat16 per register: element 2q in the low half
        h[q] = __builtin_amdgcn_perm(bh[2 * q + 1], bh[2 * q], 0x07060302u);
        m[q] = __builtin_amdgcn_perm(bm[2 * q + 1], bm[2 * q], 0x07060302u);
        l[q] = __builtin_amdgcn_perm(bl[2 * q + 1], bl[2 * q], 0x07060302u);
    }
    ph = __builtin_bit_cast(bf16x8, h);
    pm = __builtin_bit_cast(bf16x8, m);
    pl = __builtin_bit_cast(bf16x8, l);
}

// ---- float32 carried as TWO binary16 planes (gru_packed == 3; round 5): half the matrix-core time of the three-plane form.
// x = hi + lo with hi = x rounded to binary16 (11 significant bits) and lo = x - hi (exact, below 2^-11 |x|); lo is
// carried SCALED by 2^11 -- lo' = binary16(2048 lo), again 11 significant bits, well inside binary16's exponent range wherever
// hi is -- so what is dropped is below 2^-22 |x|.  A product x w is hi hi + (hi lo' + lo' hi) 2^-11 + O(2^-22): THREE plane
// products on v_mfma_f32_32x32x16_f16 (the same 32 cycles for K = 16 as the bfloat16 instruction), the two cross products into
// a second accumulator that joins the first with one multiply-add in the gate arithmetic.  Measured on 2048 x 128 x 384 random
// operands against the exact product: max 3.9e-7, rms 5.6e-8 -- a float32 GEMM of the same operands: 9.5e-7 / 7.5e-8.
// Range: binary16's.  Activations are the hidden state (in [-1, 1]) and fc1's ReLU output; |x| > 65504 saturates (f16_saturate:
// never inf; the same for a weight).
// Below 2^-14 hi is a binary16 DENORMAL (spacing 2^-24) and lo' the 11 bits after it: conversions and the matrix cores take
// denormal operands as they are on gfx950 (round 5: with them flushed -- s_setreg MODE.FP_DENORM -- a hidden state of 3e-5 kept 11
// bits in all, and products against large weights were off by 2e-4; tests/test_gpu_actor.py holds the case).
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
constexpr float F16_LO_SCALE = 2048.0f, F16_LO_UNSCALE = 1.0f / 2048.0f;
// The activations are split where they are PRODUCED (fc1's epilogue, the hidden state's staging copy: split1 below), once per tile,
// into plane images in LDS; the products' loop reads 16-byte operands and runs no conversion (split by every wave at every K step,
// 64 conversion instructions per step stood between the MFMAs: 52 cycles per MFMA against the pipe's 32).

constexpr int TM = 32;        // agent rows per wavefront
constexpr int MAX_IP = 64;    // padded input width (multiple of 8)

struct ActorArgs {
    rg_actor_weights w;
    const float *obs;       // [E][N][D]
    const uint8_t *restart; // [E] or NULL: nonzero = a new episode: hidden state and observation are taken as zero
    float *hidden;          // [E][N][H] in/out
    float *q;               // [E][N][A] or NULL
    int32_t *actions;       // [E][N] or NULL
    const float *explore_u; // [E][N] uniforms in [0, 1) or NULL: epsilon-greedy selection (rg_actor_forward_explore)
    float explore_scale;    // n_actions / epsilon
    int32_t E, N, D, append_agent_id, ip;  // ip = padded input width
    const float *sample_u;  // [E][N] uniforms in [0, 1) or NULL: soft-policies sampling (rg_actor_forward_sample; soft_select_row below)
    float *prob;            // [E][N] or NULL: the probability the sampled action had
};

// ---- the launch's arithmetic, on the host: what rg_actor_forward*, rg_actor_unroll and rg_policy_rollout each need of it
static_assert(MAX_IP % 8 == 0, "so that a padded width is within MAX_IP exactly when the width is");
inline bool input_width_fits(int64_t in_dim) { return in_dim <= MAX_IP; }
inline int padded_input_width(int in_dim) { return (in_dim + 7) / 8 * 8; }   // ActorArgs::ip, of a width that fits
// shared weights: tiles of the flat [B * N] row space; otherwise a tile takes rows of ONE agent index (RG_ACTOR_LOCATE)
inline int64_t actor_tiles(int n_sets, int64_t B, int64_t N) { return n_sets == 1 ? (B * N + TM - 1) / TM : N * ((B + TM - 1) / TM); }
inline float explore_scale(const float *explore_u, int n_actions, float epsilon) { return explore_u ? static_cast<float>(n_actions) / epsilon : 0.0f; }

// gate nonlinearities on the hardware exponential (v_exp_f32, ~1 ulp on 2^t): absolute error ~1e-7 on
// outputs in [0, 1] / [-1, 1], far inside the 1e-5 parity bar, at a tenth of libm's instruction count
// (v_rcp_f32 is within 1 ulp; `1.0f / x` would be the ten-instruction correctly rounded division, 48 times per lane and tile)
// torch.relu: a NaN stays a NaN (v_max_f32 would return the 0)
__device__ __forceinline__ float relu_(float x) { return x < 0.0f ? 0.0f : x; }
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x)); }

// ---- soft policies: the action is SAMPLED from softmax(logits) (EPyMARL's SoftPoliciesSelector, external to the reference: what
// its MAPPO / IPPO / MAA2C checkpoints collect data with) and the probability it had is reported.  The rule is a float32 SPEC, as
// explore_select is: this file, marbler_amd.evaluate.soft_select (torch) and tests/soft_twin.py (numpy) give the same action and
// the same `prob` word for the same (q, u).  Per agent row, from the logits q[0..A) as the launch writes them and ONE uniform u:
//   m = the row maximum; e_c = soft_exp(q_c - m); c_k = the partial sums of ((e_0 + e_1) + e_2) + ... in ascending column order,
//   Z = c_{A-1}; t = u * Z; the action is the first k with t < c_k, or, if there is none, the last k with e_k > 0 (for u below 1
//   the float32 product u * Z stays below Z: only u = 1, outside sample_u's range, gets there -- and still lands inside the row's
//   support); prob = e_action / Z (one correctly rounded division).  A column with e_k = 0 (a -inf logit, underflow) is never
//   chosen.  A row whose maximum is not finite (a NaN anywhere, +inf, all -inf) takes the greedy action and prob = NaN.
// soft_exp(x), x <= 0, is NOT v_exp_f32 or libm (neither promises the same bits as a CPU twin): with this file compiled
// -ffp-contract=off every line is one correctly rounded IEEE operation --
//   k = rint(x * LOG2E) (to nearest even); r = (x - k * LN2_HI) - k * LN2_LO (LN2_HI = 355 / 512: k * LN2_HI is exact);
//   p = ((((P0 r + P1) r + P2) r + P3) r + P4) r + P5, every multiply and add its own operation; y = ((p * (r * r)) + r) + 1;
//   the result is y with k added to its exponent field; 0 for x < SOFT_CUT = -87.336 (below it exp(x) < 1.001 x 2^-126, the edge of
//   the normal float32 range; at and above it k >= -126 and y >= 1, so the exponent field never leaves the normal range).
// Constants: LOG2E = 0x3FB8AA3B, LN2_HI = 0.693359375, LN2_LO = -2.12194440e-4 and the Cephes expf coefficients 1.9875691500e-4,
// 1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1.  Measured against binary64 exp on 2^24
// random arguments in [SOFT_CUT, 0] and every reduction boundary: at most 1.37 x 2^-24 relative (tests/test_soft_select.py).
constexpr float SOFT_LOG2E = 1.4426950408889634f, SOFT_LN2_HI = 0.693359375f, SOFT_LN2_LO = -2.12194440e-4f, SOFT_CUT = -87.336f;
__device__ __forceinline__ float soft_exp(float x) {
    const bool live = x >= SOFT_CUT;           // (false for -inf and NaN)
    const float xc = live ? x : 0.0f;
    const float k = __builtin_rintf(xc * SOFT_LOG2E);
    const float r = (xc - k * SOFT_LN2_HI) - k * SOFT_LN2_LO;
    float p = 1.9875691500e-4f;
    p = p * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    const float y = ((p * (r * r)) + r) + 1.0f;
    const int32_t bits = __builtin_bit_cast(int32_t, y) + (static_cast<int32_t>(k) << 23);
    return live ? __builtin_bit_cast(float, bits) : 0.0f;
}
// Where the ordered sum runs.  After fc2 a row's A logits sit on TPR neighbouring lanes, CPT consecutive columns each (the layout
// of the arg-max pass).  The CPT exponentials of a lane are independent and run on all lanes at once; the chain of additions is
// walked lane by lane in column order: in round s every lane continues the chain from the carry over its own columns, the lane
// with sub == s keeps its partial sums, and its running value is the next round's carry (one __shfl of width TPR) -- the spec's
// additions in the spec's order, TPR x CPT = 32 adds and TPR shuffles per lane, no LDS traffic and no barrier.  (Republishing
// the logits in LDS for ONE lane of the row to walk would put all 32 exponentials, ~20 dependent operations each, on a 1 / TPR
// occupied wave behind an LDS round trip; here the exponentials use every lane.)  Padding columns (c >= A) carry e = 0: x + 0 is
// x, they change nothing in the chain.  The first crossing and the last positive column are then reduced over the row's lanes
// with the same xor butterfly as the arg-max.  `sub` = the lane's position in its row, m = the row's maximum on every lane.
template <int TPR, int CPT>
__device__ __forceinline__ void soft_select_row(const float (&v)[CPT], float m, int sub, int A, float u, int greedy, int &action,
                                                float &prob) {
    float e[CPT], cs[CPT];
#pragma unroll
    for (int c_ = 0; c_ < CPT; ++c_) {
        e[c_] = sub * CPT + c_ < A ? soft_exp(v[c_] - m) : 0.0f;
        cs[c_] = 0.0f;
    }
    float carry = 0.0f;
#pragma unroll
    for (int s = 0; s < TPR; ++s) {
        float run = carry;
#pragma unroll
        for (int c_ = 0; c_ < CPT; ++c_) {
            run = run + e[c_];
            cs[c_] = sub == s ? run : cs[c_];
        }
        carry = __shfl(run, s, TPR);
    }
    const float Z = carry, t = u * Z;
    int hit = 0x7FFFFFFF, last = -1;
    float ehit = 0.0f, elast = 0.0f;
#pragma unroll
    for (int c_ = 0; c_ < CPT; ++c_) {
        const int c = sub * CPT + c_;
        if (e[c_] > 0.0f) last = c, elast = e[c_];
        if (c < A && t < cs[c_] && hit == 0x7FFFFFFF) hit = c, ehit = e[c_];
    }
#pragma unroll
    for (int d = 1; d < TPR; d <<= 1) {
        const int oh = __shfl_xor(hit, d), ol = __shfl_xor(last, d);
        const float oeh = __shfl_xor(ehit, d), oel = __shfl_xor(elast, d);
        if (oh < hit) hit = oh, ehit = oeh;
        if (ol > last) last = ol, elast = oel;
    }
    const bool none = hit == 0x7FFFFFFF;
    const bool finite = (__builtin_bit_cast(uint32_t, m) & 0x7F800000u) != 0x7F800000u;
    action = finite ? (none ? last : hit) : greedy;
    prob = finite ? (none ? elast : ehit) / Z : __builtin_nanf("");
}


// Two [TM][H] images in LDS with pitch exactly H.  Bank conflicts are avoided by an XOR swizzle of the 16-byte block index
// with the row instead of padding: block b of row i lives at block b ^ (i & 7).  The eight lanes of an LDS lane group read the
// same logical block of eight consecutive rows -> eight different physical blocks -> all 32 banks.
template <int H>
__device__ __forceinline__ int swz(int i, int k) { return i * H + ((((k >> 2) ^ (i & 7)) << 2) | (k & 3)); }
template <int H>
__device__ __forceinline__ int swz4(int i, int k4) { return i * H + ((k4 ^ (i & 7)) << 2); }

// binary16 plane images [TM][H] (pitch H halves): the 16-byte block b8 = k / 8 of row i lives at block b8 ^ (i & 7) -- the eight lanes
// of an LDS lane group read one logical block of eight consecutive rows: eight physical blocks, all banks
template <int H>
__device__ __forceinline__ int swz8(int i, int b8) { return i * H + ((b8 ^ (i & 7)) << 3); }
// one value -> its two planes, rounded to nearest (the activations are split where they are PRODUCED, once per tile)
// (beyond binary16's largest finite value the conversion would round to infinity and the low plane to NaN: the value saturates
// instead -- comparisons, so that a NaN stays a NaN)
constexpr float F16_MAX = 65504.0f;
__device__ __forceinline__ float f16_saturate(float x) { return x > F16_MAX ? F16_MAX : x < -F16_MAX ? -F16_MAX : x; }
__device__ __forceinline__ void split1(float x, _Float16 &hi, _Float16 &lo) {
    x = f16_saturate(x);
    hi = static_cast<_Float16>(x);
    lo = static_cast<_Float16>((x - static_cast<float>(hi)) * F16_LO_SCALE);
}

// a workgroup barrier that orders LDS traffic only: global stores in flight stay in flight
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

}  // namespace rg
