// policy_body.inc -- the body of rg_policy_rollout's kernels (policy_rollout.h describes it), included INSIDE the two kernels that
// differ in the action selector only: policy_rollout_kernel (RG_POLICY_SAMPLE false: greedy / epsilon-greedy, the token stream it
// had before the sampling rule existed) and policy_rollout_sample_kernel (true: soft policies, actor_common.h soft_select_row).
// The including kernel provides its argument `pa_in` and the template parameters SCN, GW, H.
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
        // The argument block is re-addressed every time step (device_common.h kernarg_block): left loop-invariant, the compiler
        // hoists every kernel-argument load of the actor AND of the env step out of the time loop and holds all of them across
        // both phases -- the whole register file and hundreds of spilled values.
        const PolicyArgs &pa = *(const PolicyArgs *)kernarg_block<PolicyArgs>();
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
        if constexpr (RG_POLICY_SAMPLE) {
            ac.sample_u = pa.act.sample_u + static_cast<size_t>(t) * EN;
            ac.prob = pa.act.prob ? pa.act.prob + static_cast<size_t>(t) * EN : nullptr;
        }
        if (shared) {
            for (int tb = 0; tb < nrows; tb += TM) {
                if (tb) __syncthreads();   // the previous tile's last LDS reads
                policy_tile<H, RG_POLICY_SAMPLE>(ac, hres, row0, 0, row0 + tb);
            }
        } else {
            for (int s = 0; s < N; ++s) {
                if (s) __syncthreads();
                policy_tile<H, RG_POLICY_SAMPLE>(ac, hres, row0, s, e0);
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
