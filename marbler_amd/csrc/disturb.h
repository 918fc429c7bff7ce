// disturb.h -- the pose disturbance (rg_set_disturbance, include/robogym.h rg_disturbance_params): a bounded, zero-mean,
// near-Gaussian pose error applied to every agent's stored pose as the first thing of an env step.
// Out of parity scope by construction (the reference has no such thing); every value is held to the float32 oracle stepped
// from the pose displaced by the NumPy twin (tests/disturb_twin.py).
//
// Spec (DESIGN.md "Pose disturbance").  Env e (global index ge = env_offset + e), agent a < N, running episode
// ep = reset_count[e] - 1, at step s = episode_steps[e] as read at the start of the step:
//   draw      (w0, w1, w2, w3) = philox4x32_10(counter (ge_lo, ge_hi, ep, 0x40000000 | ((s & 0x3FFFFFF) << 4) | a),
//                                              key (seed_lo, seed_hi) of the step's seed)
//             -- the reset sampler's stream family at blocks no other draw reaches (the sampler: blocks <= 32; the team
//             draw: 0x80000000)
//   variates  c_j = sum_i ((w_i >> 10 j) & 1023) - 2046 for j = 0 (x), 1 (y), 2 (theta), in integers: the sum of four
//             uniforms on 0..1023, so c_j lies in [-2046, 2046], its variance is exactly (2^20 - 1) / 3, and the variate is
//             bounded at +-3.46 sigma
//   scale     k = binary32(double(sigma) * sqrt(3.0 / 1048575.0)), computed on the host in binary64 (kernel_args.h
//             disturb_scale, by rg_set_disturbance); k = 0 leaves that part of the pose alone
//   update    x' = x + k_xy * float(c_0), y' = y + k_xy * float(c_1), theta' = wrap_spec(theta + k_theta * float(c_2)),
//             every operation rounded to binary32, no contraction
// Only `poses` is displaced; everything the step reads afterwards (the goal, the controller, the barrier QP, integration,
// distance travelled, tracking, rewards, observations, the violation tests) reads the displaced pose.  The draw adds no
// state and does not depend on batch size, sharding, kernel form or rollout length.  rg_get_obs applies nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "device_common.h"

namespace rg {

// the disturbance kernels' argument block: the step's own and the two scales (kernel_args.h DisturbScale), side by side (the other kernels never see the latter)
struct DisturbArgs {
    KernelArgs k;
    DisturbScale ds;
};

// Philox block of the draw of step s, agent a: above every block of the reset sampler, below the team draw's
constexpr uint32_t DISTURB_BLOCK = 0x40000000u;

// c_0, c_1, c_2 of (ge, ep, s, a): integers in [-2046, 2046]
__device__ __forceinline__ void disturb_draw(uint64_t ge, int32_t ep, int32_t s, int a, uint64_t seed, int (&c)[3]) {
    const uint32_t blk = DISTURB_BLOCK | ((static_cast<uint32_t>(s) & 0x3FFFFFFu) << 4) | static_cast<uint32_t>(a);
    uint32_t w[4];
    philox4x32_10(static_cast<uint32_t>(ge), static_cast<uint32_t>(ge >> 32), static_cast<uint32_t>(ep), blk,
                  static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), w);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        uint32_t sum = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) sum += (w[i] >> (10 * j)) & 1023u;
        c[j] = static_cast<int>(sum) - 2046;
    }
}

// the update of one agent's pose
__device__ __forceinline__ void disturb_pose(float k_xy, float k_theta, const int (&c)[3], float &x, float &y, float &th) {
    x = x + k_xy * static_cast<float>(c[0]);
    y = y + k_xy * static_cast<float>(c[1]);
    th = wrap_spec(th + k_theta * static_cast<float>(c[2]));
}

}  // namespace rg
