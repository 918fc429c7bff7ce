// actor_mfma.hip -- the EPyMARL recurrent actor (utilities/rnn_agent.py:5-29: fc1 -> ReLU -> GRUCell ->
// fc2, or rnn_ns_agent.py:5-36 with one such network per agent) for all E x N agents of a batch in
// ONE launch: policy inference for on-device evaluation rollouts.
//
// This is the one dense contraction on the path, so it runs on the matrix cores.  One workgroup of H/32 wavefronts owns a
// tile of 32 agent rows and carries it through the whole network, wavefront w computing the 32 hidden columns
// [32 w, 32 w + 32) of every layer:
//     X [32 x I]  --fc1-->  Y [32 x H]  --GRU (6 gate tiles per 32 hidden columns)-->  h' [32 x H]  --fc2--> q [32 x A]
// * The GRU -- 96 % of the arithmetic -- has three forms.  gru_packed == 3 (rg_actor_pack_gru_f16x2, the default of
//   marbler_amd/evaluate.py since round 5): every float32 value is carried as TWO binary16 planes (hi, 2^11 lo) and a float32
//   product becomes three plane products on v_mfma_f32_32x32x16_f16, the cross terms in a second accumulator; the activations are
//   split where they are produced, into plane images in LDS (see "two binary16 planes" below).  gru_packed == 2
//   (rg_actor_pack_gru_bf16x3, round 4): THREE bfloat16 planes (split8 below), six plane products on v_mfma_f32_32x32x16_bf16
//   (32 cycles for K = 16), float32's exponent range, an error below a float32 dot product's own roundings.  gru_packed == 0 / 1:
//   f32-input MFMA (v_mfma_f32_32x32x2_f32, 64 cycles for K = 2), exact float32 products.  At 4096 x 4 rows, hidden 128:
//   19-20 / 24-26 / 44-50 us per launch.
// * A operands (activations) are read from LDS; B operands of the GRU (weights) stream from L2 in the order a pack routine
//   wrote them (1 KB per load instruction), a ring of groups ahead of the MFMAs, held in place by scheduling fences.  fc1's
//   small ragged operands are fetched once per tile, coalesced, and staged in LDS (inputs up to 32 wide; wider ones are read
//   as they lie by a ROLLED loop: unrolled, the layer was ~600 instructions of cold code at the head of every launch).
// * Two [32][H] float32 LDS images with an XOR swizzle instead of padding (a third, of binary16 planes, in the two-plane form:
//   48 KB per tile at hidden 128), and 256 registers per lane (amdgpu_waves_per_eu): TWO tiles per CU, one wave of each per SIMD.
//   (Rounds 1-3 ran one tile per CU -- 352 registers per lane; LDS was never the limit: hipOccupancyMaxActiveBlocksPerMultiprocessor
//   reckons with 64 KB of LDS per CU, the hardware has 160.)
// * Memory traffic is ordered by hand: the head requests the restart flag, fc1's staged operands and then the hidden state (the
//   vector-memory counter retires in order: the wait in front of the staging stores leaves the hidden state in flight); the GRU's
//   first weight groups go out ahead of fc1's epilogue; the new hidden state is stored right after the gates and drains under fc2
//   and the arg-max, whose barriers order LDS only (lds_barrier).
// * Layer outputs come out of the MFMA with the column on the lane and 16 rows in registers (C/D map: col = lane & 31,
//   row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)); the gate arithmetic is elementwise in that layout and one LDS write turns it
//   into the next layer's A image.  fc2's K range is split over the tile's wavefronts, the partial tiles meet in LDS, and all
//   threads take part in the bias / arg-max / q stores.  Non-shared actors: a tile takes the rows of ONE agent index (stride N),
//   so the whole tile uses one weight set.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/robogym.h"
#include "actor_common.h"
#include "host_checks.h"

namespace rg {

// tile blockIdx.x of the whole batch (shared: rows 32 b .. 32 b + 31 of the flat [E*N] row space; otherwise agent
// b / tiles_per_agent, envs 32 (b % tiles_per_agent) ..), the hidden state read and written in memory
#define RG_ACTOR_LOCATE(shared, E, set, base)                 \
    if (shared) {                                             \
        base = blockIdx.x * TM;                               \
    } else {                                                  \
        const int tiles_per_agent = (E + TM - 1) / TM;        \
        set = blockIdx.x / tiles_per_agent;                   \
        base = (blockIdx.x - set * tiles_per_agent) * TM;     \
    }
#define RG_ACTOR_HIDDEN_LOAD(r, k4) *reinterpret_cast<const float4 *>(a.hidden + static_cast<size_t>(r) * H + 4 * (k4))
#define RG_ACTOR_HIDDEN_STORE(r, j, v) a.hidden[static_cast<size_t>(r) * H + (j)] = (v)

template <int H, int SPLIT>   // SPLIT: the GRU's products on 1: three bfloat16 planes (gru_packed == 2), 2: two binary16 planes (gru_packed == 3)
__attribute__((amdgpu_waves_per_eu(2, 2)))   // 256 registers (VGPR + AGPR): two tiles per CU, one's serial phases under the other's MFMAs
__global__ __launch_bounds__(64 * (H / 32)) void actor_kernel(const ActorArgs a) {
#define RG_ACTOR_SAMPLING(a) false
#include "actor_body.inc"
#undef RG_ACTOR_SAMPLING
}

// The same tile computation with the soft-policies epilogue (rg_actor_forward_sample; actor_common.h soft_select_row).  A kernel of
// its own, not a run-time branch in actor_kernel: the selector is a compile-time constant of the body, so the greedy /
// epsilon-greedy kernels keep the instruction stream they had before the rule existed.
template <int H, int SPLIT>
__attribute__((amdgpu_waves_per_eu(2, 2)))
__global__ __launch_bounds__(64 * (H / 32)) void actor_sample_kernel(const ActorArgs a) {
#define RG_ACTOR_SAMPLING(a) true
#include "actor_body.inc"
#undef RG_ACTOR_SAMPLING
}
#undef RG_ACTOR_LOCATE
#undef RG_ACTOR_HIDDEN_LOAD
#undef RG_ACTOR_HIDDEN_STORE

// torch layout [S][3H][H] -> the kernel's streaming order [S][cb][chunk][gate][q4][lane = (half, col)][4]
__global__ void pack_gru_kernel(const float *src, float *dst, int n_sets, int H) {
    const int nch = (H / 2) / 32, ncb = H / 32;
    const size_t total = static_cast<size_t>(n_sets) * 3 * H * H;
    for (size_t o = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; o < total;
         o += static_cast<size_t>(gridDim.x) * blockDim.x) {
        size_t r = o;
        const int f = r % 4; r /= 4;
        const int lane = r % 64; r /= 64;
        const int q4 = r % 8; r /= 8;
        const int g = r % 3; r /= 3;
        const int chunk = r % nch; r /= nch;
        const int cb = r % ncb; r /= ncb;
        const int s = static_cast<int>(r);
        const int half = lane >> 5, col = lane & 31;
        const int row = g * H + cb * 32 + col, k = half * (H / 2) + chunk * 32 + q4 * 4 + f;
        dst[o] = src[(static_cast<size_t>(s) * 3 * H + row) * H + k];
    }
}

// torch layout [S][3H][H] float32 -> three bfloat16 planes in the SPLIT kernel's streaming order
// [S][cb][ks][gate][plane][lane = (half, col)][8]: 6 bytes per weight
__global__ void pack_gru_bf16x3_kernel(const float *src, uint16_t *dst, int n_sets, int H) {
    const int nks = H / 16, ncb = H / 32;
    const size_t total = static_cast<size_t>(n_sets) * 3 * H * H;   // (set, cb, ks, gate, lane, e) tuples = weights
    for (size_t o = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; o < total;
         o += static_cast<size_t>(gridDim.x) * blockDim.x) {
        size_t r = o;
        const int e = r % 8; r /= 8;
        const int lane = r % 64; r /= 64;
        const int g = r % 3; r /= 3;
        const int ks = r % nks; r /= nks;
        const int cb = r % ncb; r /= ncb;
        const int s = static_cast<int>(r);
        const int half = lane >> 5, col = lane & 31;
        const int row = g * H + cb * 32 + col, k = ks * 16 + half * 8 + e;
        const float w = src[(static_cast<size_t>(s) * 3 * H + row) * H + k];
        const uint32_t bh = __builtin_bit_cast(uint32_t, w) & 0xFFFF0000u;
        const float r1 = w - __builtin_bit_cast(float, bh);
        const uint32_t bm = __builtin_bit_cast(uint32_t, r1) & 0xFFFF0000u;
        const float r2 = r1 - __builtin_bit_cast(float, bm);
        const uint32_t bl = __builtin_bit_cast(uint32_t, r2);
        const size_t base = ((((static_cast<size_t>(s) * ncb + cb) * nks + ks) * 3 + g) * 3) * 64 * 8 + static_cast<size_t>(lane) * 8 + e;
        dst[base] = static_cast<uint16_t>(bh >> 16);
        dst[base + 64 * 8] = static_cast<uint16_t>(bm >> 16);
        dst[base + 2 * 64 * 8] = static_cast<uint16_t>(bl >> 16);
    }
}

// torch layout [S][3H][H] float32 -> two binary16 planes (hi, 2^11 lo: see split1) in the streaming order
// [S][cb][ks][gate][plane][lane = (half, col)][8]: 4 bytes per weight.  Round to nearest here (the weights are split once).
__global__ void pack_gru_f16x2_kernel(const float *src, uint16_t *dst, int n_sets, int H) {
    const int nks = H / 16, ncb = H / 32;
    const size_t total = static_cast<size_t>(n_sets) * 3 * H * H;
    for (size_t o = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; o < total;
         o += static_cast<size_t>(gridDim.x) * blockDim.x) {
        size_t r = o;
        const int e = r % 8; r /= 8;
        const int lane = r % 64; r /= 64;
        const int g = r % 3; r /= 3;
        const int ks = r % nks; r /= nks;
        const int cb = r % ncb; r /= ncb;
        const int s = static_cast<int>(r);
        const int half = lane >> 5, col = lane & 31;
        const int row = g * H + cb * 32 + col, k = ks * 16 + half * 8 + e;
        const float w = f16_saturate(src[(static_cast<size_t>(s) * 3 * H + row) * H + k]);
        const _Float16 hi = static_cast<_Float16>(w);
        const float rest = (w - static_cast<float>(hi)) * F16_LO_SCALE;
        const _Float16 lo = static_cast<_Float16>(rest);
        const size_t base = ((((static_cast<size_t>(s) * ncb + cb) * nks + ks) * 3 + g) * 2) * 64 * 8 + static_cast<size_t>(lane) * 8 + e;
        dst[base] = __builtin_bit_cast(uint16_t, hi);
        dst[base + 64 * 8] = __builtin_bit_cast(uint16_t, lo);
    }
}

}  // namespace rg

static thread_local char g_actor_err[256] = "";

// the three pack entries: one check (rg_actor_pack_gru's float32 order takes any dst: align 1), one launch
template <class T>
static int pack_gru(const char *entry, void (*kernel)(const float *, T *, int, int), size_t align, const float *src, int32_t n_sets,
                    int32_t hidden_dim, void *dst, void *hip_stream) {
    const rg::Fail fail{g_actor_err, sizeof(g_actor_err), entry};
    if (!src || !dst || n_sets < 1 || (hidden_dim != 64 && hidden_dim != 128)) return fail(-1, "NULL array, n_sets < 1 or hidden_dim not 64 / 128");
    if (!rg::all_aligned(align, dst)) return fail(-9, "dst must be 16-byte aligned");
    hipLaunchKernelGGL(kernel, dim3(256), dim3(256), 0, static_cast<hipStream_t>(hip_stream), src, static_cast<T *>(dst), n_sets, hidden_dim);
    return hipGetLastError() == hipSuccess ? 0 : -30;
}

extern "C" int rg_actor_pack_gru_f16x2(const float *src, int32_t n_sets, int32_t hidden_dim, void *dst, void *hip_stream) {
    return pack_gru("rg_actor_pack_gru_f16x2", rg::pack_gru_f16x2_kernel, 16, src, n_sets, hidden_dim, dst, hip_stream);
}

extern "C" int rg_actor_pack_gru_bf16x3(const float *src, int32_t n_sets, int32_t hidden_dim, void *dst, void *hip_stream) {
    return pack_gru("rg_actor_pack_gru_bf16x3", rg::pack_gru_bf16x3_kernel, 16, src, n_sets, hidden_dim, dst, hip_stream);
}

extern "C" int rg_actor_pack_gru(const float *src, int32_t n_sets, int32_t hidden_dim, float *dst, void *hip_stream) {
    return pack_gru("rg_actor_pack_gru", rg::pack_gru_kernel, 1, src, n_sets, hidden_dim, dst, hip_stream);
}

extern "C" const char *rg_actor_last_error(void) { return g_actor_err; }

RG_ACTOR_DIAG_ENTRY   // (diagnostic builds: rg_actor_occupancy)

// (hidden_dim, split, sampling), each checked by the caller -> the kernel's template arguments, as integral constants
template <class F>
static void for_actor_kernel(int hidden_dim, int split, bool sampling, F &&f) {
    using std::integral_constant;
    auto with = [&](auto h, auto s) { sampling ? f(h, s, std::true_type()) : f(h, s, std::false_type()); };
    switch (hidden_dim * 4 + split) {
        case 64 * 4 + 0: return with(integral_constant<int, 64>(), integral_constant<int, 0>());
        case 64 * 4 + 1: return with(integral_constant<int, 64>(), integral_constant<int, 1>());
        case 64 * 4 + 2: return with(integral_constant<int, 64>(), integral_constant<int, 2>());
        case 128 * 4 + 0: return with(integral_constant<int, 128>(), integral_constant<int, 0>());
        case 128 * 4 + 1: return with(integral_constant<int, 128>(), integral_constant<int, 1>());
        case 128 * 4 + 2: return with(integral_constant<int, 128>(), integral_constant<int, 2>());
    }
}

static int actor_forward(const rg_actor_weights *w, int32_t num_envs, int32_t n_agents, const float *obs,
                         int32_t obs_dim, int32_t append_agent_id, const uint8_t *restart, float *hidden,
                         float *q, int32_t *actions, const float *explore_u, float epsilon, void *hip_stream,
                         const float *sample_u = nullptr, float *prob = nullptr) {
    const rg::Fail fail{g_actor_err, sizeof(g_actor_err), nullptr};
    if (!w || !obs || !hidden) return fail(-1, "weights, obs or hidden is NULL");
    if (!w->w1 || !w->b1 || !w->wih || !w->bih || !w->w2 || !w->b2) return fail(-2, "a weight array is NULL");
    if (w->use_rnn && (!w->whh || !w->bhh)) return fail(-2, "GRU weights whh / bhh are NULL");
    if (w->hidden_dim != 64 && w->hidden_dim != 128) return fail(-3, "hidden_dim must be 64 or 128 (the reference's actors)");
    if (w->n_actions < 1 || w->n_actions > 32) return fail(-4, "n_actions must be in 1..32");
    if (w->gru_packed < 0 || w->gru_packed > 3) return fail(-10, "gru_packed must be 0 (torch layout), 1 (rg_actor_pack_gru), 2 (rg_actor_pack_gru_bf16x3) or 3 (rg_actor_pack_gru_f16x2)");
    if (w->n_sets != 1 && w->n_sets != n_agents) return fail(-5, "n_sets must be 1 (shared) or n_agents");
    if (num_envs < 1 || n_agents < 1 || obs_dim < 1) return fail(-6, "num_envs, n_agents, obs_dim must be >= 1");
    if (explore_u && !(epsilon >= 1e-6f && epsilon <= 1.0f)) return fail(-11, "epsilon must be in [1e-6, 1] when explore_u is given");
    if (explore_u && !actions) return fail(-11, "explore_u without an actions array");
    const int in_dim = obs_dim + (append_agent_id ? n_agents : 0);
    if (in_dim != w->input_dim) return fail(-7, "obs_dim (+ n_agents with append_agent_id) != the actor's input_dim");
    if (!rg::input_width_fits(in_dim)) return fail(-8, "input_dim above 64 is not supported");
    if (!rg::all_aligned(16, hidden, w->w1, w->wih, w->whh, w->w2)) return fail(-9, "hidden, w1, wih, whh and w2 must be 16-byte aligned");
    rg::ActorArgs a;
    a.w = *w;
    a.obs = obs;
    a.restart = restart;
    a.hidden = hidden;
    a.q = q;
    a.actions = actions;
    a.explore_u = explore_u;
    a.explore_scale = rg::explore_scale(explore_u, w->n_actions, epsilon);
    a.sample_u = sample_u;
    a.prob = prob;
    a.E = num_envs;
    a.N = n_agents;
    a.D = obs_dim;
    a.append_agent_id = append_agent_id;
    a.ip = rg::padded_input_width(in_dim);
    const dim3 tiles(static_cast<uint32_t>(rg::actor_tiles(w->n_sets, num_envs, n_agents)));
    const int split = !w->use_rnn ? 0 : w->gru_packed == 2 ? 1 : w->gru_packed == 3 ? 2 : 0;
    for_actor_kernel(w->hidden_dim, split, sample_u != nullptr, [&](auto h, auto s, auto sampling) {
        constexpr int H = decltype(h)::value, SPLIT = decltype(s)::value;
        if constexpr (decltype(sampling)::value) hipLaunchKernelGGL((rg::actor_sample_kernel<H, SPLIT>), tiles, dim3(64 * (H / 32)), 0, static_cast<hipStream_t>(hip_stream), a);
        else hipLaunchKernelGGL((rg::actor_kernel<H, SPLIT>), tiles, dim3(64 * (H / 32)), 0, static_cast<hipStream_t>(hip_stream), a);
    });
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return fail(-30, hipGetErrorString(err));
    return 0;
}

extern "C" int rg_actor_forward(const rg_actor_weights *w, int32_t num_envs, int32_t n_agents, const float *obs,
                                int32_t obs_dim, int32_t append_agent_id, const uint8_t *restart, float *hidden,
                                float *q, int32_t *actions, void *hip_stream) {
    return actor_forward(w, num_envs, n_agents, obs, obs_dim, append_agent_id, restart, hidden, q, actions, nullptr, 0.0f,
                         hip_stream);
}

extern "C" int rg_actor_forward_explore(const rg_actor_weights *w, int32_t num_envs, int32_t n_agents, const float *obs,
                                        int32_t obs_dim, int32_t append_agent_id, const uint8_t *restart, float *hidden,
                                        float *q, int32_t *actions, const float *explore_u, float epsilon,
                                        void *hip_stream) {
    return actor_forward(w, num_envs, n_agents, obs, obs_dim, append_agent_id, restart, hidden, q, actions, explore_u, epsilon,
                         hip_stream);
}

extern "C" int rg_actor_forward_sample(const rg_actor_weights *w, int32_t num_envs, int32_t n_agents, const float *obs,
                                       int32_t obs_dim, int32_t append_agent_id, const uint8_t *restart, float *hidden,
                                       float *q, int32_t *actions, const float *sample_u, float *prob, void *hip_stream) {
    const rg::Fail fail{g_actor_err, sizeof(g_actor_err), "rg_actor_forward_sample"};
    if (!sample_u) return fail(-12, "sample_u is NULL");
    if (!actions) return fail(-12, "sample_u without an actions array");
    return actor_forward(w, num_envs, n_agents, obs, obs_dim, append_agent_id, restart, hidden, q, actions, nullptr, 0.0f,
                         hip_stream, sample_u, prob);
}
