// policy_rollout.h -- rg_policy_rollout: T time steps of "actor -> action -> env step" in ONE launch (instantiated by
// robogym_policy_h64.hip and robogym_policy_h128.hip, one file per hidden size so that the two compile side by side).
//
// A workgroup is the actor's H / 32 wavefronts and owns the envs of one step wavefront (64 / GW envs, at most 64 agent rows: two
// actor tiles of 32 rows; a non-shared actor takes one tile per agent index).  Envs are independent, so there is no device-wide
// synchronisation between time steps (as in rg_rollout).  Per time step:
//   1. every wavefront runs the actor's tiles of the workgroup's rows (actor_body.inc: the arithmetic of actor_kernel<H, 2>, the
//      two-binary16-plane GRU); the hidden state stays in LDS for the whole launch and is written back once at the end;
//   2. the greedy or epsilon-greedy action goes to the caller's actions[t] (global memory, read back by the same workgroup);
//   3. wavefront 0 runs one env step (step_once, gymma block compiled in, AHEAD = false as in rg_rollout) with WaveSync: every
//      barrier inside it is wave scope, the other wavefronts wait at the next uniform workgroup barrier;
//   4. the observation and the episode-end flags it wrote are the next time step's actor inputs (workgroup-scope release /
//      acquire of that barrier).
// The only workgroup barriers are the uniform ones between the phases and those inside the actor's tiles, which every wavefront
// runs.  LDS: the actor's three [32][H] images (48 KB at H = 128), the resident hidden state [64][H] float32 (32 KB) and the
// step's Lds<GW> (7.5 KB): 88 KB at H = 128, 48 KB at H = 64, within the CU's 160 KB.
#pragma once
#include <string.h>

#include "actor_common.h"
#include "step_group.h"

namespace rg {

struct PolicyArgs {
    KernelArgs k;            // the env: state, the step's output slots (rg_step_io), auto_reset, seed; envs_per_wave = 64 / GW
    ActorArgs act;           // the actor: weights, N, D, append_agent_id, ip, explore_scale (per-step pointers set in the kernel)
    rg_policy_io io;
    int32_t T;
};

// the hidden state of flat row r lives at row r - row0 of the workgroup's resident block (rows outside the tile read row 0)
constexpr int POLICY_ROWS = 64;

// One actor tile of the workgroup's rows: `a.E` is the end of the workgroup's envs (the body's row bound), hres the resident
// hidden state of rows row0 .. row0 + 63.
template <int H>
__device__ __forceinline__ void policy_tile(const ActorArgs &a, float *hres, int row0, int t_set, int t_base) {
    constexpr int SPLIT = 2;
#define RG_ACTOR_LOCATE(shared, E, set, base) \
    set = t_set;                              \
    base = t_base
#define RG_ACTOR_HIDDEN_LOAD(r, k4) \
    *reinterpret_cast<const float4 *>(&hres[(static_cast<unsigned>((r) - row0) < POLICY_ROWS ? (r) - row0 : 0) * H + 4 * (k4)])
#define RG_ACTOR_HIDDEN_STORE(r, j, v) hres[((r) - row0) * H + (j)] = (v)
#include "actor_body.inc"
#undef RG_ACTOR_LOCATE
#undef RG_ACTOR_HIDDEN_LOAD
#undef RG_ACTOR_HIDDEN_STORE
}

template <int SCN, int GW, int H>
__global__ __launch_bounds__(64 * (H / 32)) void policy_rollout_kernel(const PolicyArgs pa_in) {
    constexpr int NTHREADS = 64 * (H / 32), EPW = WAVE / GW;
    __shared__ __attribute__((aligned(16))) float hres[POLICY_ROWS * H];
    __shared__ Lds<GW> lds;
    const PolicyArgs &pa = pa_in;
    const KernelArgs &a = pa.k;
    const rg_policy_io &io = pa.io;
    const int tid = threadIdx.x;
    const int E = a.E, N = a.p.n_agents, D = a.p.obs_dim, T = pa.T;
    const size_t EN = static_cast<size_t>(E) * N;
    const int e0 = xcd_chunk(gridDim.x) * EPW;   // the envs step_once gives this workgroup's wavefront 0
    const int e_end = e0 + EPW < E ? e0 + EPW : E;
    const int row0 = e0 * N, nrows = (e_end - e0) * N;
    const bool shared = pa.act.w.n_sets == 1;

    for (int i = tid; i < nrows * (H / 4); i += NTHREADS)
        reinterpret_cast<float4 *>(hres)[i] = reinterpret_cast<const float4 *>(io.hidden + static_cast<size_t>(row0) * H)[i];
    // wavefront 0's lane -> (env, agent) of step_once, for the distance sums
    const int ag = tid & (GW - 1), e = e0 + tid / GW;
    const bool lane_ok = tid < WAVE && e < e_end && ag < N;
    float dist = (lane_ok && io.dist_sum) ? io.dist_sum[static_cast<size_t>(e) * N + ag] : 0.0f;
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        // The argument block is re-addressed every time step (an opaque copy of the kernel-argument segment's address; the block is
        // the kernel's only argument, at offset 0): left loop-invariant, the compiler hoists every kernel-argument load of the actor
        // AND of the env step out of the time loop and holds all of them across both phases -- the whole register file and hundreds
        // of spilled values.  (Not `&pa_in`: taking the argument's address makes the compiler copy it to scratch.)
        typedef const __attribute__((address_space(4))) PolicyArgs *ArgPtr;
        ArgPtr pp = (ArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(pp));
        const PolicyArgs &pa = *(const PolicyArgs *)pp;
        const KernelArgs &a = pa.k;
        const rg_policy_io &io = pa.io;
        int32_t *act_t = io.actions + static_cast<size_t>(t) * EN;
        ActorArgs ac = pa.act;
        ac.E = e_end;
        ac.obs = io.obs ? io.obs + static_cast<size_t>(t) * EN * D : a.io.obs;
        ac.restart = t == 0 ? io.restart
                            : io.restart_on_done ? a.io.done : (io.ended ? io.ended + static_cast<size_t>(t - 1) * E : a.io.ended);
        ac.actions = act_t;
        ac.q = nullptr;
        ac.explore_u = io.explore_u ? io.explore_u + static_cast<size_t>(t) * EN : nullptr;
        if (shared) {
            for (int tb = 0; tb < nrows; tb += TM) {
                if (tb) __syncthreads();   // the previous tile's last LDS reads
                policy_tile<H>(ac, hres, row0, 0, row0 + tb);
            }
        } else {
            for (int s = 0; s < N; ++s) {
                if (s) __syncthreads();
                policy_tile<H>(ac, hres, row0, s, e0);
            }
        }
        __syncthreads();   // the actions are in memory; the actor's LDS is free
        if (tid < WAVE) {
            StepView sv = step_view(a, 0, N, D);
            sv.actions = act_t;
            sv.io.obs = io.obs ? io.obs + static_cast<size_t>(t + 1) * EN * D : a.io.obs;
            if (io.reward_sum) sv.io.reward_sum = io.reward_sum + static_cast<size_t>(t) * E;
            if (io.ended) sv.io.ended = io.ended + static_cast<size_t>(t) * E;
            step_once<SCN, GW, false, 0, false, true, 0, void, WaveSync>(a, lds, sv, static_cast<void *>(nullptr));
            // run_eval's `dist.add_(env.dist_travelled)`: float32 adds in step order (this lane stored the value itself)
            if (lane_ok && io.dist_sum) dist = dist + sv.io.dist_travelled[static_cast<size_t>(e) * N + ag];
        }
        __syncthreads();   // the step's outputs are the next time step's inputs
    }
    for (int i = tid; i < nrows * (H / 4); i += NTHREADS)
        reinterpret_cast<float4 *>(io.hidden + static_cast<size_t>(row0) * H)[i] = reinterpret_cast<const float4 *>(hres)[i];
    if (lane_ok && io.dist_sum) io.dist_sum[static_cast<size_t>(e) * N + ag] = dist;
}

template <int SCN, int H>
static hipError_t launch_policy_scn(const PolicyArgs &pa_in, hipStream_t stream) {
    PolicyArgs pa = pa_in;
    const int gw = SCN == RG_SCN_ARCTIC_TRANSPORT ? 4 : group_width(pa.k.p.n_agents);
    pa.k.envs_per_wave = WAVE / gw;
    const int grid = (pa.k.E + WAVE / gw - 1) / (WAVE / gw);
    const dim3 block(64 * (H / 32));
    if (gw == 4) hipLaunchKernelGGL((policy_rollout_kernel<SCN, 4, H>), dim3(grid), block, 0, stream, pa);
    else if constexpr (SCN != RG_SCN_ARCTIC_TRANSPORT) {
        if (gw == 8) hipLaunchKernelGGL((policy_rollout_kernel<SCN, 8, H>), dim3(grid), block, 0, stream, pa);
        else hipLaunchKernelGGL((policy_rollout_kernel<SCN, 16, H>), dim3(grid), block, 0, stream, pa);
    }
    return hipGetLastError();
}

// every argument validated by rg_policy_rollout (robogym_capi.hip)
template <int H>
static hipError_t launch_policy_h(const KernelArgs &k, const rg_actor_weights &w, const rg_policy_io &io, int32_t T,
                                  hipStream_t stream) {
    PolicyArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.k = k;
    pa.io = io;
    pa.T = T;
    pa.act.w = w;
    pa.act.N = k.p.n_agents;
    pa.act.D = k.p.obs_dim;
    pa.act.append_agent_id = io.append_agent_id;
    pa.act.ip = (w.input_dim + 7) / 8 * 8;
    pa.act.explore_scale = io.explore_u ? static_cast<float>(w.n_actions) / io.epsilon : 0.0f;
    switch (k.p.scenario) {
        case RG_SCN_PREDATOR_CAPTURE_PREY: return launch_policy_scn<RG_SCN_PREDATOR_CAPTURE_PREY, H>(pa, stream);
        case RG_SCN_WAREHOUSE: return launch_policy_scn<RG_SCN_WAREHOUSE, H>(pa, stream);
        case RG_SCN_MATERIAL_TRANSPORT: return launch_policy_scn<RG_SCN_MATERIAL_TRANSPORT, H>(pa, stream);
        case RG_SCN_SIMPLE: return launch_policy_scn<RG_SCN_SIMPLE, H>(pa, stream);
        case RG_SCN_ARCTIC_TRANSPORT: return launch_policy_scn<RG_SCN_ARCTIC_TRANSPORT, H>(pa, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rg
