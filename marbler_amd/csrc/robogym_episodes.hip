// robogym_episodes.hip -- rg_episodes_append: a collector's time-major stream into episode-major slots, one launch per collection
// (include/robogym.h; the rule: episodes.h).
//
// The traffic is the rows: every obs row of the stream is read once and written once (N D floats; 256 B at PredatorCapturePrey
// x 4), the action / prob rows likewise, and the flags are a byte per (t, e).  ONE wave owns an env for the whole call:
//   * per chunk of 64 time steps lane l loads the flags and the reward of step t0 + l (consecutive envs of a step lie side by
//     side, so the four waves of a work-group read neighbouring bytes) and two ballots turn them into the chunk's start and
//     termination masks.  Where an episode begins and ends in the chunk is then scalar bit arithmetic on the two masks and the
//     env's cursor: no serial walk over T, no divergence -- every value that steers the wave is wave-uniform.
//   * an episode's part of the chunk is a run of consecutive stream rows that go to consecutive slot rows: the destination is ONE
//     contiguous block, the source rows lie E N D floats apart.  The 64 lanes copy it together, a lane a 16-byte piece (8 or 4
//     bytes where N D or a base is not a multiple of 16 bytes: the host picks the kernel), COPY_UNROLL pieces in flight, so a
//     wave instruction covers 1 KiB of the destination and whole 256-B runs of the source.
//   * the episodes of a chunk are written one after the other by the same wave, in order, with a wave-scope fence between them:
//     an env that wraps its ring inside a call overwrites its own older slot exactly as the sequential rule says, and nothing
//     else in the launch touches that env's slots.
// E waves of 64 lanes: 4096 waves at 4096 envs, half of the wave slots of the chip, each with 4 KiB in flight.
//
// The host entry is handle-free and keeps its own last-error text (as robogym_render.hip does): every argument check comes
// before the first HIP call, so the refusals can be exercised without a device.
#include <hip/hip_runtime.h>

#include "episodes.h"
#include "host_checks.h"

namespace rg {
namespace episodes {

#ifndef RG_EPISODES_HOST_ONLY   // (the sanitized host build, build.py build_host_sanitized: the argument checks without the kernel)
typedef float F4 __attribute__((ext_vector_type(4)));
typedef float F2 __attribute__((ext_vector_type(2)));
template <int VW> struct Piece;
template <> struct Piece<4> { using type = F4; };
template <> struct Piece<2> { using type = F2; };
template <> struct Piece<1> { using type = float; };

// where lane `lane` starts in a block of rows of `per_row` pieces, and how 64 pieces further on moves it
struct Walk {
    int row, col, d_row, d_col;
};
__device__ __forceinline__ Walk walk_of(int lane, int per_row) {
    Walk w;
    w.row = lane / per_row;
    w.col = lane - w.row * per_row;
    w.d_row = 64 / per_row;
    w.d_col = 64 - w.d_row * per_row;
    return w;
}

// `items` = rows * per_row pieces: piece (row, col) of the source, whose rows lie `src_stride` pieces apart, goes to piece
// row * per_row + col of the contiguous destination.  The whole wave calls it; lane `lane` takes pieces lane, lane + 64, ...
template <typename V>
__device__ __forceinline__ void copy_rows(const V *__restrict__ src, size_t src_stride, V *__restrict__ dst, int items, int per_row,
                                          Walk w, int lane) {
    for (int i = lane; i < items; i += 64 * COPY_UNROLL) {
        V v[COPY_UNROLL];
#pragma unroll
        for (int u = 0; u < COPY_UNROLL; ++u) {
            v[u] = i + 64 * u < items ? src[static_cast<size_t>(w.row) * src_stride + w.col] : V(0);
            w.col += w.d_col;
            w.row += w.d_row;
            if (w.col >= per_row) {
                w.col -= per_row;
                ++w.row;
            }
        }
#pragma unroll
        for (int u = 0; u < COPY_UNROLL; ++u)
            if (i + 64 * u < items) dst[i + 64 * u] = v[u];
    }
}

// what one lane wrote, another lane of the wave may overwrite: order the two (a wave's memory operations execute in order; the
// fence keeps the compiler from moving them)
__device__ __forceinline__ void wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int VW>
__global__ __launch_bounds__(BLOCK) void episodes_append_kernel(const Args a) {
    using V = typename Piece<VW>::type;
    const int lane = static_cast<int>(threadIdx.x) & 63;
    const int e = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * ENVS_PER_BLOCK + (static_cast<int>(threadIdx.x) >> 6));
    const int E = a.b.num_envs, R = a.b.slots_per_env, L = a.b.episode_limit, N = a.b.n_agents, T = a.s.T;
    if (e >= E) return;
    const int ND = N * a.b.obs_dim, per_row = ND / VW;
    const Walk w_obs = walk_of(lane, per_row), w_act = walk_of(lane, N);
    const bool with_prob = a.b.prob != nullptr;

    int32_t *cursor = a.b.cursor + static_cast<size_t>(e) * CUR_WORDS;
    int open = cursor[CUR_OPEN], pos = cursor[CUR_POS], opened = cursor[CUR_OPENED], overflow = cursor[CUR_OVERFLOW];
    float ret = open >= 0 ? a.b.episode_return[open] : 0.0f;

    for (int t0 = 0; t0 < T; t0 += 64) {
        const int n_in = T - t0 < 64 ? T - t0 : 64;
        const bool in = lane < n_in;
        const size_t at = static_cast<size_t>(t0 + lane) * E + e;
        const bool starts = in && a.s.episode_start[at] != 0, ends = in && a.s.terminated[at] != 0;
        const float rw = in ? a.s.reward[at] : 0.0f;
        const uint64_t S = __ballot(starts), M = __ballot(ends);

        int cur = 0;
        while (cur < n_in) {
            if ((S >> cur) & 1) {           // rule 1
                if (open >= 0) --opened;    // abandoned: the new episode takes its slot
                const int slot = e * R + opened % R;
                const size_t row0 = static_cast<size_t>(slot) * (L + 1);
                for (int r = lane; r <= L; r += 64) {
                    a.b.filled[row0 + r] = 0;
                    a.b.terminated[row0 + r] = 0;
                    a.b.reward[row0 + r] = 0.0f;
                }
                if (lane == 0) {
                    a.b.length[slot] = 0;
                    a.b.episode_return[slot] = 0.0f;
                    a.b.complete[slot] = 0;
                    a.b.fresh[slot] = 0;
                    a.b.episode_index[slot] = opened;
                }
                wave_order();
                open = slot;
                pos = 0;
                ret = 0.0f;
                ++opened;
            }
            // the steps up to the next start belong to this episode (or to none)
            const uint64_t later = cur < 63 ? S & (~0ull << (cur + 1)) : 0;
            const int seg_end = later ? __builtin_ctzll(later) : n_in;
            if (open < 0) {                 // rule 2
                cur = seg_end;
                continue;
            }
            int n = seg_end - cur;          // transitions the episode takes here: up to its end
            bool closes = false, overflows = false;
            const uint64_t ends_here = M & (~0ull << cur) & (seg_end < 64 ? (1ull << seg_end) - 1 : ~0ull);
            if (ends_here) {                // rule 4
                n = __builtin_ctzll(ends_here) - cur + 1;
                closes = true;
            }
            if (L - pos < n) {              // rule 5: the slot is full before that
                n = L - pos;
                closes = overflows = true;
            } else if (L - pos == n && !closes) {
                closes = overflows = true;
            }
            const size_t row = static_cast<size_t>(open) * (L + 1) + pos;       // slot row of the first transition
            const size_t src_row = static_cast<size_t>(t0 + cur) * E + e;      // its (t, e)
            // rule 3 (and the last-data row of rule 4): n + closes obs rows, n action / prob rows
            copy_rows<V>(reinterpret_cast<const V *>(a.s.obs) + src_row * per_row, static_cast<size_t>(E) * per_row,
                         reinterpret_cast<V *>(a.b.obs) + row * per_row, (n + (closes ? 1 : 0)) * per_row, per_row, w_obs, lane);
            copy_rows<int32_t>(a.s.actions + src_row * N, static_cast<size_t>(E) * N, a.b.actions + row * N, n * N, N, w_act, lane);
            if (with_prob) copy_rows<float>(a.s.prob + src_row * N, static_cast<size_t>(E) * N, a.b.prob + row * N, n * N, N, w_act, lane);
            const int j = lane - cur;
            if (j >= 0 && j < n) {
                a.b.reward[row + j] = rw;
                a.b.terminated[row + j] = ends ? 1 : 0;
                a.b.filled[row + j] = 1;
            }
            for (int k = 0; k < n; ++k)     // one binary32 addition per step, in step order
                ret = ret + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rw), cur + k));
            if (lane == 0) {
                a.b.episode_return[open] = ret;
                if (closes) {
                    a.b.filled[row + n] = 1;
                    a.b.length[open] = pos + n;
                    a.b.complete[open] = 1;
                    a.b.fresh[open] = 1;
                }
            }
            wave_order();
            if (closes) {
                overflow += overflows ? 1 : 0;
                open = -1;
            } else {
                pos += n;
            }
            cur = seg_end;
        }
    }
    if (lane == 0) {
        cursor[CUR_OPEN] = open;
        cursor[CUR_POS] = open >= 0 ? pos : 0;
        cursor[CUR_OPENED] = opened;
        cursor[CUR_OVERFLOW] = overflow;
    }
}

static bool launch(const Args &a, int vw, void *hip_stream) {
    const dim3 grid((static_cast<uint32_t>(a.b.num_envs) + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK), block(BLOCK);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (vw == 4)
        hipLaunchKernelGGL(episodes_append_kernel<4>, grid, block, 0, stream, a);
    else if (vw == 2)
        hipLaunchKernelGGL(episodes_append_kernel<2>, grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL(episodes_append_kernel<1>, grid, block, 0, stream, a);
    return hipGetLastError() == hipSuccess;
}
#else
static bool launch(const Args &, int, void *) { return false; }
#endif

}  // namespace episodes
}  // namespace rg

static thread_local char g_episodes_err[256] = "";

extern "C" const char *rg_episodes_last_error(void) { return g_episodes_err; }
extern "C" int rg_sizeof_episode_buffer(void) { return static_cast<int>(sizeof(rg_episode_buffer)); }
extern "C" int rg_sizeof_episode_stream(void) { return static_cast<int>(sizeof(rg_episode_stream)); }

extern "C" int rg_episodes_append(const rg_episode_buffer *buffer, const rg_episode_stream *stream, void *hip_stream) {
    using namespace rg::episodes;
    const rg::Fail fail{g_episodes_err, sizeof(g_episodes_err), "rg_episodes_append"};
    if (!buffer) return fail(-1, "buffer", "is NULL");
    if (!stream) return fail(-2, "stream", "is NULL");
    const rg_episode_buffer &b = *buffer;
    const rg_episode_stream &s = *stream;
    if (b.num_envs < 1) return fail(-110, "buffer.num_envs", "must be >= 1");
    if (b.slots_per_env < 1) return fail(-111, "buffer.slots_per_env", "must be >= 1");
    if (b.episode_limit < 1) return fail(-112, "buffer.episode_limit", "must be >= 1");
    if (b.n_agents < 1) return fail(-113, "buffer.n_agents", "must be >= 1");
    if (b.obs_dim < 1) return fail(-114, "buffer.obs_dim", "must be >= 1");
    if (s.T < 1) return fail(-115, "stream.T", "must be >= 1");
    // the largest arrays are the obs ones
    if (!rg::elements_fit(b.num_envs, b.slots_per_env, static_cast<int64_t>(b.episode_limit) + 1, b.n_agents, b.obs_dim))
        return fail(-116, "buffer.num_envs * slots_per_env * (episode_limit + 1) * n_agents * obs_dim", "exceeds 2^31 - 1 elements");
    if (!rg::elements_fit(static_cast<int64_t>(s.T) + 1, b.num_envs, b.n_agents, b.obs_dim))
        return fail(-117, "(stream.T + 1) * buffer.num_envs * n_agents * obs_dim", "exceeds 2^31 - 1 elements");
    const rg::NamedPtr fields[] = {{b.obs, "buffer.obs", 4},
                                   {b.actions, "buffer.actions", 4},
                                   {b.reward, "buffer.reward", 4},
                                   {b.terminated, "buffer.terminated", 1},
                                   {b.filled, "buffer.filled", 1},
                                   {b.length, "buffer.length", 4},
                                   {b.episode_return, "buffer.episode_return", 4},
                                   {b.complete, "buffer.complete", 1},
                                   {b.fresh, "buffer.fresh", 1},
                                   {b.episode_index, "buffer.episode_index", 4},
                                   {b.cursor, "buffer.cursor", 4},
                                   {s.obs, "stream.obs", 4},
                                   {s.actions, "stream.actions", 4},
                                   {s.reward, "stream.reward", 4},
                                   {s.terminated, "stream.terminated", 1},
                                   {s.episode_start, "stream.episode_start", 1},
                                   {b.prob, "buffer.prob", 4},   // (the 16 above are required; the two prob arrays: both or neither)
                                   {s.prob, "stream.prob", 4}};
    if (const rg::NamedPtr *f = rg::first_null(fields, 16)) return fail(-120 - static_cast<int>(f - fields), f->name, "is NULL");
    if (b.prob && !s.prob) return fail(-136, "stream.prob", "is NULL, but buffer.prob is not: the buffer keeps prob, the stream has none");
    if (s.prob && !b.prob) return fail(-137, "buffer.prob", "is NULL, but stream.prob is not: the stream has prob, the buffer keeps none");
    if (const rg::NamedPtr *f = rg::first_misaligned(fields)) return fail(-150 - static_cast<int>(f - fields), f->name, "must be 4-byte aligned");

    // the widest piece that divides a row and keeps every row of both obs arrays aligned
    const int nd = b.n_agents * b.obs_dim;
    const uintptr_t bases = reinterpret_cast<uintptr_t>(b.obs) | reinterpret_cast<uintptr_t>(s.obs);
    const int vw = (nd % 4 == 0 && (bases & 15u) == 0) ? 4 : (nd % 2 == 0 && (bases & 7u) == 0) ? 2 : 1;
    Args a;
    a.b = b;
    a.s = s;
    if (!launch(a, vw, hip_stream)) return fail(-30, "the launch", "failed");
    return 0;
}
