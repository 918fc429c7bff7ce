// policy_rollout.h -- rg_policy_rollout: T time steps of "actor -> action -> env step" in ONE launch (instantiated by
// robogym_policy_unit.hip, compiled once per hidden size and selector so that they compile side by side).
//
// A workgroup is the actor's H / 32 wavefronts and owns the envs of one step wavefront (64 / GW envs, at most 64 agent rows: two
// actor tiles of 32 rows; a non-shared actor takes one tile per agent index).  Envs are independent, so there is no device-wide
// synchronisation between time steps (as in rg_rollout).  Per time step:
//   1. every wavefront runs the actor's tiles of the workgroup's rows (actor_body.inc: the arithmetic of actor_kernel<H, 2>, the
//      two-binary16-plane GRU); the hidden state stays in LDS for the whole launch and is written back once at the end;
//   2. the greedy, epsilon-greedy or (rg_policy_rollout_sample) sampled action goes to the caller's actions[t] (global memory, read
//      back by the same workgroup); the sampling rule is the actor launch's (actor_common.h soft_select_row), in kernels of its own
//      (policy_rollout_sample_kernel: the same body, policy_body.inc, with the selector a compile-time constant);
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
    ActorArgs act;           // the actor: weights, N, D, append_agent_id, ip, explore_scale; sample_u / prob: the [T][E][N] arrays of
                             // rg_policy_sample or NULL (the other per-step pointers are set in the kernel)
    rg_policy_io io;
    int32_t T;
};

// the hidden state of flat row r lives at row r - row0 of the workgroup's resident block (rows outside the tile read row 0)
constexpr int POLICY_ROWS = 64;

// One actor tile of the workgroup's rows: `a.E` is the end of the workgroup's envs (the body's row bound), hres the resident
// hidden state of rows row0 .. row0 + 63.
template <int H, bool SAMPLE>
__device__ __forceinline__ void policy_tile(const ActorArgs &a, float *hres, int row0, int t_set, int t_base) {
    constexpr int SPLIT = 2;
#define RG_ACTOR_LOCATE(shared, E, set, base) \
    set = t_set;                              \
    base = t_base
#define RG_ACTOR_HIDDEN_LOAD(r, k4) \
    *reinterpret_cast<const float4 *>(&hres[(static_cast<unsigned>((r) - row0) < POLICY_ROWS ? (r) - row0 : 0) * H + 4 * (k4)])
#define RG_ACTOR_HIDDEN_STORE(r, j, v) hres[((r) - row0) * H + (j)] = (v)
#define RG_ACTOR_SAMPLING(a) SAMPLE
#include "actor_body.inc"
#undef RG_ACTOR_SAMPLING
#undef RG_ACTOR_LOCATE
#undef RG_ACTOR_HIDDEN_LOAD
#undef RG_ACTOR_HIDDEN_STORE
}

template <int SCN, int GW, int H>
__global__ __launch_bounds__(64 * (H / 32)) void policy_rollout_kernel(const PolicyArgs pa_in) {
#define RG_POLICY_SAMPLE false
#include "policy_body.inc"
#undef RG_POLICY_SAMPLE
}

// rg_policy_rollout_sample: the same launch with the soft-policies epilogue in the actor's tiles.  A kernel of its own: a run-time
// selector in the shared body measured 1.6 % on the greedy rollout at hidden 128 (1812 -> 1840 us per 64 steps at 4096 x 4),
// eight times the parent's run-to-run spread.
template <int SCN, int GW, int H>
__global__ __launch_bounds__(64 * (H / 32)) void policy_rollout_sample_kernel(const PolicyArgs pa_in) {
#define RG_POLICY_SAMPLE true
#include "policy_body.inc"
#undef RG_POLICY_SAMPLE
}

#define RG_POLICY_LAUNCH(gw_)                                                                                        \
    do {                                                                                                             \
        if constexpr (SAMPLE) hipLaunchKernelGGL((policy_rollout_sample_kernel<SCN, gw_, H>), dim3(grid), block, 0, stream, pa); \
        else hipLaunchKernelGGL((policy_rollout_kernel<SCN, gw_, H>), dim3(grid), block, 0, stream, pa);                        \
    } while (0)
template <int SCN, int H, bool SAMPLE>
static hipError_t launch_policy_scn(const PolicyArgs &pa_in, hipStream_t stream) {
    PolicyArgs pa = pa_in;
    const int gw = group_width(pa.k.p.n_agents);
    pa.k.envs_per_wave = WAVE / gw;
    const int grid = (pa.k.E + WAVE / gw - 1) / (WAVE / gw);
    const dim3 block(64 * (H / 32));
    if (gw == 4) RG_POLICY_LAUNCH(4);
    else if constexpr (SCN != RG_SCN_ARCTIC_TRANSPORT) {
        if (gw == 8) RG_POLICY_LAUNCH(8);
        else RG_POLICY_LAUNCH(16);
    }
    return hipGetLastError();
}
#undef RG_POLICY_LAUNCH

// every argument validated by rg_policy_rollout (robogym_capi.hip)
template <int H, bool SAMPLE = false>
static hipError_t launch_policy_h(const KernelArgs &k, const rg_actor_weights &w, const rg_policy_io &io, int32_t T,
                                  hipStream_t stream, const rg_policy_sample *sample = nullptr) {
    PolicyArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.k = k;
    pa.io = io;
    pa.T = T;
    pa.act.w = w;
    pa.act.N = k.p.n_agents;
    pa.act.D = k.p.obs_dim;
    pa.act.append_agent_id = io.append_agent_id;
    pa.act.ip = padded_input_width(w.input_dim);
    pa.act.explore_scale = explore_scale(io.explore_u, w.n_actions, io.epsilon);
    pa.act.sample_u = sample ? sample->sample_u : nullptr;
    pa.act.prob = sample ? sample->prob : nullptr;
    return for_scenario(k.p.scenario, [&](auto scn) { return launch_policy_scn<decltype(scn)::value, H, SAMPLE>(pa, stream); });
}

}  // namespace rg
