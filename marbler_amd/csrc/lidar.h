// lidar.h -- the opt-in range observation (rg_set_lidar, include/robogym.h rg_lidar_params): R rays per agent, appended to the
// agent's observation row after the scenario's own columns.  Out of parity scope by construction (the reference has no lidar).
//
// Spec (DESIGN.md "Lidar"): ray k of agent i at post-step pose (x, y, th) points along (cos th, sin th) rotated by the host's
// table dir[k] = binary32(cos, sin of 2 pi k / R).  Its range t is the smallest positive distance from the robot's centre to
// the disk (radius robot_diameter / 2) of another robot of the env, or to a wall of the arena rectangle; the stored value is
// min(t, L) / L -- exactly 1 when nothing lies within L, 0 when the centre lies inside another robot's disk, and 0 on every ray
// of an agent whose centre lies outside the arena.
//
// Mapping: the lane-group kernel's (one lane per agent).  Partner positions come from the wave's LDS rows the scenario's own
// observation builder staged (own[][0..1], or ax / ay for MaterialTransport's step).  Rays go in chunks of four (four running minima
// live, one 16-byte store per chunk where the row allows it), partners are the inner loop, a partner farther than L + rho is
// culled.  The square root and the reciprocal are the hardware's (v_sqrt_f32, v_rcp_f32: 1 ulp): the values are reproducible
// bit for bit on the GPU across every path that writes them (they are the same instructions), not on a CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"

namespace rg {

// the lidar kernels' argument block: the step's own and the lidar's, side by side (the existing kernels never see the latter)
struct LidarArgs {
    KernelArgs k;
    rg_lidar_params lid;
};

template <int SCN, int GW, bool OBS_ONLY, typename Sync>
__device__ __forceinline__ void write_lidar(const rg_lidar_params &lp, const KernelArgs &a, Lds<GW> &lds, int lane, int gbase, int N,
                                            int ag, bool lane_ok, float x, float y, float th, float *obs_row) {
    constexpr bool MT = SCN == RG_SCN_MATERIAL_TRANSPORT;
    // MaterialTransport's step stages x, y in ax / ay for its reward replay; its observation-only launch stages nothing and
    // uses no LDS at all otherwise: 512 bytes of its own there instead of the whole step block
    __shared__ float2 xy_stage[(MT && OBS_ONLY) ? WAVE : 1];
    if constexpr (MT && OBS_ONLY) {
        xy_stage[lane] = make_float2(x, y);
        Sync::sync();
    }
    const Consts &k = a.k;
    const float L = lp.range, inv_L = lp.inv_range;
    const float rho = 0.5f * a.p.robot_diameter, rho2 = rho * rho;
    const float cull = L + rho, cull2 = cull * cull;
    const bool outside = (x < k.xmin) | (x > k.xmax) | (y < k.ymin) | (y > k.ymax);
    // distances to the four walls (>= 0 inside the arena, +0 on a wall)
    const float w_xhi = k.xmax - x, w_xlo = x - k.xmin, w_yhi = k.ymax - y, w_ylo = y - k.ymin;
    float s, c;
    sincos_spec(th, s, c);
    const int R = lp.rays;
    float *dst = obs_row + lp.offset;
    const bool wide = ((a.p.obs_dim | lp.offset) & 3) == 0;   // every row's block 16-byte aligned (obs is, rg_step checks it)
    for (int r0 = 0; r0 < R; r0 += 4) {
        float ux[4], uy[4], tm[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float ck = lp.dir[r0 + t][0], sk = lp.dir[r0 + t][1];
            ux[t] = c * ck - s * sk;
            uy[t] = s * ck + c * sk;
            // the nearer wall along the ray: wx / |ux| against wy / |uy|, compared without dividing
            const float ax = __builtin_fabsf(ux[t]), ay = __builtin_fabsf(uy[t]);
            const float wx = ux[t] > 0.0f ? w_xhi : w_xlo, wy = uy[t] > 0.0f ? w_yhi : w_ylo;
            const bool use_x = (ay == 0.0f) | (wx * ay < wy * ax);
            tm[t] = (use_x ? wx : wy) * __builtin_amdgcn_rcpf(use_x ? ax : ay);
        }
        for (int j = 0; j < N; ++j) {
            float px, py;
            if constexpr (MT && OBS_ONLY) {
                const float2 q = xy_stage[gbase + j];
                px = q.x;
                py = q.y;
            } else if constexpr (MT) {
                px = lds.ax[gbase + j];
                py = lds.ay[gbase + j];
            } else {
                const float2 q = *reinterpret_cast<const float2 *>(&lds.own[gbase + j][0]);
                px = q.x;
                py = q.y;
            }
            const float dx = px - x, dy = py - y;
            const float d2 = dx * dx + dy * dy;
            if ((j != ag) & (d2 <= cull2)) {
                const float cc = d2 - rho2;   // <= 0: this centre lies inside the partner's disk
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    // b along the ray, p across it: the discriminant b^2 - cc = rho^2 - p^2 from the small terms (b^2 and cc
                    // are up to ~10 m^2, their rounding would swamp a grazing ray's discriminant)
                    const float b = dx * ux[t] + dy * uy[t];
                    const float pr = dx * uy[t] - dy * ux[t];
                    const float disc = rho2 - pr * pr;
                    const float th_ = b - __builtin_amdgcn_sqrtf(disc > 0.0f ? disc : 0.0f);
                    const bool hit = (b > 0.0f) & (disc >= 0.0f) & (th_ < tm[t]);
                    tm[t] = cc <= 0.0f ? 0.0f : hit ? th_ : tm[t];
                }
            }
        }
        float v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = outside ? 0.0f : tm[t] >= L ? 1.0f : tm[t] * inv_L;
        if (lane_ok) {
            if (wide) {
                *reinterpret_cast<float4 *>(dst + r0) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) dst[r0 + t] = v[t];
            }
        }
    }
}

}  // namespace rg
