// step_group.h -- the fused env-step kernel for gfx950 (MI355X, CDNA4), lane-group mapping.
// (Templates only: the step, its kernels in four families -- plain, lidar, team pool, pose disturbance -- and their one launch
// dispatcher.  Instantiated by robogym_group_unit.hip, compiled once per (family, solver mode, single launch or rollout), and by
// robogym_kernels.hip, robogym_team.hip and robogym_resident*.hip: kernel_args.h RG_GROUP_ENTRIES.)
//
// One launch = one env step for E envs: goal generation, U sim sub-iterations (controller with
// the barrier-certificate QP every 15th, collision/boundary validation, Euler integration),
// then the scenario's tracking / observation / reward / termination, and the reset of envs that
// finished -- all with the env's state in registers.  HBM traffic is the algorithmic I/O only
// (measured with rocprofv3 FETCH_SIZE / WRITE_SIZE in profiles/).
//
// Mapping: a lane GROUP of GW lanes (GW = 4, 8 or 16 >= N) owns one env, one lane per agent; a
// 64-lane wavefront carries 64/GW envs; one wavefront per workgroup (no cross-wave sync
// anywhere).  The O(N^2) pair work (collision scan, QP constraint sweeps) runs as GW-1
// "rounds": in round k lane a is paired with lane a^k, a 1-factorisation of the complete graph
// on the group -- disjoint pairs, so a Gauss-Seidel sweep over the QP constraints in this
// order is pair-parallel yet identical to the sequential sweep of the CPU oracle.  Partner
// data moves by DPP (row-local lane permutes on the VALU), never through memory; per-env
// reductions are DPP butterflies or one wave ballot; the per-env prey block and the agents'
// own-observation rows are staged in LDS.
//
// No MFMA: there is no dense contraction on this path.  At the benchmark size (4096 envs =
// 512 wavefronts on 1024 SIMDs) the kernel is a latency-bound dependent chain per wavefront, so
// the design goal is the shortest per-lane instruction chain with independent work interleaved
// (sub-steps are processed in chunks of 5 for ILP), not bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "device_common.h"
#include "ipm_qp.h"
#include "lidar.h"
#include "team.h"
#include "disturb.h"
#include "probes/diag.h"   // diagnostic hooks: every RG_* macro below expands to nothing in the shipped build

namespace rg {

// Output stores (observation rows, rewards, distances): plain stores (non-temporal ones were tried: NOTEBOOK.md section 4.4)
__device__ __forceinline__ void out_store4(float *p, float a, float b, float c, float d) {
    *reinterpret_cast<float4 *>(p) = make_float4(a, b, c, d);
}
__device__ __forceinline__ void out_store1(float *p, float a) {
    *p = a;
}

// sub-steps validated together (ILP across independent test chains).  The controller periods of the
// reference's configurations are 15 and 14 sub-steps: three chunks of 5, or two and a remainder chunk of 4.
constexpr int CHUNK = RG_CHUNK;
static_assert(CHUNK >= 1 && CHUNK <= 5, "the sparse collision pre-test covers sub-steps 0..2 and 3..4 of a chunk: longer chunks would go untested");

// ------------------------------------------------------------------ controller (a3..a8)
// utilities/controller.py:20-24 over the restated rps closures,
// followed by Robotarium.set_velocities' clipping.  Called in wave-uniform control flow.
// QPM: how the certificate's QP is evaluated (include/robogym.h RG_QP_*): 0 the exact projection by the Hildreth sweeps below,
// 1 cvxopt's interior-point iterate (ipm_qp.h; qp = the wave's LDS of that mode: one record per lane, one workspace per env).
// SPAN (16-lane rows, step_once): the pair constants are split between the group and its replica (below); the sweeps run in
// the group, and the replica takes the result over.
template <int GW, int QPM = 0, typename QpLds = void, bool SPAN = false>
__device__ __forceinline__ int controller(const rg_scenario_params &p, const Consts &k, int N, int ag, bool lane_ok,
                                          bool upd, float x, float y, float c, float s, float gx, float gy, float &v,
                                          float &w, QpLds *qp RG_CTRL_TICKS_PARAM) {
    RG_CTRL_BEGIN(x, y, c, s)
    // a4 uni_to_si_states, a5 si_position_controller (gain 1, |dxi| <= 0.15)
    const float xix = x + k.pd * c, xiy = y + k.pd * s;
    float ux = gx - xix, uy = gy - xiy;
    {
        const float nrm = norm2_spec(ux, uy);
        const float sc = k.pvl / nrm;
        const bool clip = nrm > k.pvl;
        ux = clip ? ux * sc : ux;
        uy = clip ? uy * sc : uy;
    }
    if constexpr (QPM == RG_QP_CVXOPT) {
        // a6 as the reference's stack evaluates it: "threshold control inputs before QP" (decided on squares, as below), then the
        // env's records gathered in LDS and the interior-point iteration of ipm_qp.h, the same in every lane of the group
        {
            const float n2u = ux * ux + uy * uy;
            const bool clip = n2u > k.bml * k.bml;
            if (__any(clip)) {
                const float sc = k.bml / __builtin_sqrtf(n2u);
                ux = clip ? ux * sc : ux;
                uy = clip ? uy * sc : uy;
            }
        }
        const int lane_ = threadIdx.x;
        qp->rec[lane_] = make_float4(xix, xiy, ux, uy);
        __syncthreads();   // (one wave per workgroup: the records are visible)
        int iters = 0;
        if (upd) iters = ipm::solve_qp_n<GW>(N, ipm::make_consts(p), qp->rec + (lane_ & ~(GW - 1)), qp->ws[lane_ / GW], ag);
        __syncthreads();
        const float4 r = qp->rec[lane_];
        ux = r.z;
        uy = r.w;
        RG_CTRL_TICK(1);
        float vv = c * ux + s * uy;
        float ww = k.inv_pd * (-s * ux + c * uy);
        ww = ww > k.wlim ? k.wlim : ww;
        ww = ww < -k.wlim ? -k.wlim : ww;
        vv = vv > k.vmax ? k.vmax : vv;
        vv = vv < -k.vmax ? -k.vmax : vv;
        ww = ww > k.wmax ? k.wmax : ww;
        ww = ww < -k.wmax ? -k.wmax : ww;
        v = upd ? vv : v;
        w = upd ? ww : w;
        RG_CTRL_TICK(2);
        return iters;
    }
    // a6 barrier certificate: rows e_ij.(u_j - u_i) <= beta_ij, one per round; the exact projection
    // by Hildreth sweeps with vector-extrapolation restarts (algorithm and derivation: oracle/oracle_core.h
    // barrier_qp).  Per round: f = e/n2, bp = beta/n2, emax = max(|ex|, |ey|); absent pairs have
    // f = bp = emax = 0 and mu = 0, which makes every update of theirs an exact no-op.
    const float bgain = p.barrier_gain, ugain = p.unsafe_barrier_gain, qp_rtol = p.qp_rtol;
    const int qp_cap = p.qp_max_sweeps;
    const bool has_unsafe = p.barrier_has_unsafe_gain != 0;
    float ex[GW - 1], ey[GW - 1], fx[GW - 1], fy[GW - 1], bp[GW - 1], emax[GW - 1];
    float mu[GW - 1], dmu[GW - 1];  // dmu: the change of mu over sweep 2 (d1), then over sweep 3 (d2), of a block of four sweeps
    // the constants of the pair (this lane's agent, agent ag ^ K) from the partner's (pxi, pyi) into slot i of the arrays
    auto pair_consts = [&](float pxi, float pyi, int K, int i) {
        const float dx = xix - pxi, dy = xiy - pyi;
        const float ee = dx * dx + dy * dy;
        const float h = ee - k.r2;
        const float gain = ((h >= 0.0f) | !has_unsafe) ? bgain : ugain;
        const float b = gain * ((h * h) * h);
        const float n2 = 2.0f * ee;
        const bool ok = lane_ok & ((ag ^ K) < N) & (n2 > 0.0f);
        const float rn2 = ok ? 1.0f / n2 : 0.0f;
        ex[i] = dx;
        ey[i] = dy;
        fx[i] = dx * rn2;
        fy[i] = dy * rn2;
        bp[i] = (0.5f * b) * rn2;
        emax[i] = ok ? fmaxf(__builtin_fabsf(dx), __builtin_fabsf(dy)) : 0.0f;
    };
    const bool helper = SPAN && (threadIdx.x & GW) != 0;
    if constexpr (SPAN) {
        // Four rounds' worth of work instead of seven.  The replica's partner values are mirrored first (lane 8 + a holds agent
        // a ^ 7), so that ONE quad permute xor S pairs the group's lane a with agent a ^ S (rounds 1..3) and the replica's lane
        // 8 + a with agent a ^ S ^ 7 (rounds 6, 5, 4); "S = 0" is round 7 in the replica (and an absent pair in the group).
        // Slot S keeps its result in array slot 7 - S - 1 for now; the group then fetches the replica's rounds 4..7 across
        // the row, one row_ror:8 move per value.  The same operations on the same operands as the seven rounds: same bits.
        static_assert(GW == 8, "16-lane rows of two 8-lane halves");
        const float mx = mirror_upper_half(xix), my = mirror_upper_half(xiy);
        static_for<0, 4>([&](auto SS) {
            constexpr int S = decltype(SS)::value;
            const int K = helper ? S ^ 7 : S;
            if constexpr (S == 0) pair_consts(mx, my, K, 6);
            else pair_consts(xor_lane<S>(mx), xor_lane<S>(my), K, (S ^ 7) - 1);
        });
        static_for<1, 4>([&](auto SS) {   // the group: rounds 1..3 its own, 4..6 and 7 (already in place) from the replica
            constexpr int S = decltype(SS)::value, J = (S ^ 7) - 1;
            ex[S - 1] = ex[J];
            ey[S - 1] = ey[J];
            fx[S - 1] = fx[J];
            fy[S - 1] = fy[J];
            bp[S - 1] = bp[J];
            emax[S - 1] = emax[J];
        });
        static_for<3, 7>([&](auto JJ) {
            constexpr int J = decltype(JJ)::value;
            // (both halves swap: the replica's own slots J are dead from here on -- it runs no sweep -- and a move that kept
            // them would be tied to the values just copied to slots 0..2: one register copy per move)
            auto cross = [](float v) { return RG_ROW_SWAP_HALVES ? swap_halves(v) : to_lower_half(v); };
            ex[J] = cross(ex[J]);
            ey[J] = cross(ey[J]);
            fx[J] = cross(fx[J]);
            fy[J] = cross(fy[J]);
            bp[J] = cross(bp[J]);
            emax[J] = cross(emax[J]);
        });
    } else {
        static_for<1, GW>([&](auto KK) {
            constexpr int K = decltype(KK)::value;
            pair_consts(xor_lane<K>(xix), xor_lane<K>(xiy), K, K - 1);
        });
    }
    static_for<0, GW - 1>([&](auto KK) { mu[decltype(KK)::value] = dmu[decltype(KK)::value] = 0.0f; });
    RG_CTRL_PIN_ROUNDS(GW, fx, bp, emax)
    RG_CTRL_TICK(0);  // position controller + pair constants
    {   // "Threshold control inputs before QP": decided on squares; never taken after the 0.15 clip
        const float n2u = ux * ux + uy * uy;
        const bool clip = n2u > k.bml * k.bml;
        if (__any(clip)) {
            const float sc = k.bml / __builtin_sqrtf(n2u);
            ux = clip ? ux * sc : ux;
            uy = clip ? uy * sc : uy;
        }
    }
    const float uhx = ux, uhy = uy;
    // A group drops out when converged (its lanes are exec-masked for the whole sweep body: groups
    // are uniform, so an active lane never reads a masked partner); the wave loops while any group
    // is active.
    bool active = upd & !helper;   // (SPAN: the replica holds rounds of its own in the arrays; it takes the group's result below)
    int sweeps = 0, my_sweeps = 0;
    // one sweep over the GW-1 rounds + the convergence test; PHASE = sweep number mod 4 selects the
    // restart bookkeeping: d1 and d2 of oracle_core.h (the changes of the multipliers over sweeps 2 and 3 of a block of four)
    // are these sweeps' own deltas -- nothing touches mu between them -- so sweep 2 records its delta, sweep 3 forms the two
    // inner products <d2 - d1, d2>, <d2 - d1, d2 - d1> while it runs (independent of its dependent chain: free issue slots)
    // and leaves d2 in place of d1 for the restart
    auto sweep = [&](auto PH) {
        constexpr int PHASE = decltype(PH)::value;
        ++sweeps;
        if (active) {
            float chg = 0.0f, pa = 0.0f, pb = 0.0f;
            static_for<1, GW>([&](auto KK) {
                constexpr int K = decltype(KK)::value;
                const float pux = xor_lane<K>(ux), puy = xor_lane<K>(uy);
                const float c0 = mu[K - 1] - bp[K - 1];
                const float t = __builtin_fmaf(fy[K - 1], puy - uy, c0);
                float mn = __builtin_fmaf(fx[K - 1], pux - ux, t);
                mn = (mn > 0.0f) ? mn : 0.0f;
                const float delta = mn - mu[K - 1];
                mu[K - 1] = mn;
                ux = __builtin_fmaf(delta, ex[K - 1], ux);
                uy = __builtin_fmaf(delta, ey[K - 1], uy);
                chg = fmaxf(chg, __builtin_fabsf(delta) * emax[K - 1]);
                if constexpr (PHASE == 2) dmu[K - 1] = delta;
                if constexpr (PHASE == 3) {
                    const float dd = delta - dmu[K - 1];
                    pa = __builtin_fmaf(dd, delta, pa);
                    pb = __builtin_fmaf(dd, dd, pb);
                    dmu[K - 1] = delta;
                }
            });
            my_sweeps = sweeps;
            const float um = lane_ok ? fmaxf(__builtin_fabsf(ux), __builtin_fabsf(uy)) : 0.0f;
            const float gchg = group_max_nonneg<GW>(chg);
            const float gum = fmaxf(k.bml, group_max_nonneg<GW>(um));
            active = (gchg > qp_rtol * gum) & (sweeps < qp_cap);
            if constexpr (PHASE == 3) {
                if (active) {  // restart: the multipliers extrapolated along their last change, u rebuilt from them
                    const float ga = group_sum<GW>(pa), gb = group_sum<GW>(pb);
                    const bool ok = (gb > 0.0f) & (ga < 0.0f) & (-ga < 32.0f * gb);
                    const float gam = ok ? ga / gb : 0.0f;  // the one division of a restart
                    float sx = uhx, sy = uhy;
                    static_for<1, GW>([&](auto KK) {
                        constexpr int K = decltype(KK)::value;
                        float m = __builtin_fmaf(-gam, dmu[K - 1], mu[K - 1]);
                        m = (m > 0.0f) ? m : 0.0f;
                        mu[K - 1] = m;
                        sx = __builtin_fmaf(m, ex[K - 1], sx);
                        sy = __builtin_fmaf(m, ey[K - 1], sy);
                    });
                    ux = sx;
                    uy = sy;
                }
            }
        }
    };
    if constexpr (SPAN) {
        // The rows' loop is a DIVERGENT one: an env leaves it with its own verdict, and the sweeps that follow run for the envs still
        // in it.  The verdict's compare is then the exec mask of the next sweep -- one scalar and, one saveexec, one branch on "no
        // env left" -- where the wave-uniform loop below makes the compiler turn the flags into a register and back twice per
        // sweep and copy the multipliers from sweep to sweep.  The envs of a wave still step through the phases together (an env
        // that has left is masked, not behind), so `sweeps` stays the wave's count and every env sees the sweeps, the restarts
        // and the cap it saw before.
        while (active) {
            sweep(std::integral_constant<int, 1>{});
            if (!active) break;
            sweep(std::integral_constant<int, 2>{});
            if (!active) break;
            sweep(std::integral_constant<int, 3>{});
            if (!active) break;
            sweep(std::integral_constant<int, 0>{});
        }
    } else {
        while (__any(active)) {
            sweep(std::integral_constant<int, 1>{});
            if (!__any(active)) break;
            sweep(std::integral_constant<int, 2>{});
            if (!__any(active)) break;
            sweep(std::integral_constant<int, 3>{});
            if (!__any(active)) break;
            sweep(std::integral_constant<int, 0>{});
        }
    }
    if constexpr (SPAN) {
        ux = to_upper_half(ux);
        uy = to_upper_half(uy);
    }
    RG_CTRL_PIN2(ux, uy);
    RG_CTRL_TICK(1);  // sweeps
    // a7 si_to_uni_dyn, a8 set_velocities
    float vv = c * ux + s * uy;
    float ww = k.inv_pd * (-s * ux + c * uy);
    ww = ww > k.wlim ? k.wlim : ww;
    ww = ww < -k.wlim ? -k.wlim : ww;
    vv = vv > k.vmax ? k.vmax : vv;
    vv = vv < -k.vmax ? -k.vmax : vv;
    ww = ww > k.wmax ? k.wmax : ww;
    ww = ww < -k.wmax ? -k.wmax : ww;
    v = upd ? vv : v;
    w = upd ? ww : w;
    RG_CTRL_PIN2(v, w);
    RG_CTRL_COUNT_SWEEPS(sweeps);
    RG_CTRL_TICK(2);  // si -> uni, clips
    return my_sweeps;
}

// ------------------------------------------------------------------ neighbour observations
// K nearest neighbours' own-observation rows (staged in LDS) into obs slots 1..K: ascending
// squared distance, ties -> lower index (the canonical order for misc.py:20-25); K >= N-1: all
// others in index order.  Partner rows come from LDS by address, so -- unlike the DPP rounds of the
// controller -- the partners need not be the XOR partners: agent a visits (a + r) mod N, r = 1..N-1.
// With the agent count a compile-time constant (NT) that is N-1 slots and (N-1)(N-2)/2 comparisons
// instead of GW-1 and (GW-1)(GW-2)/2 (N = 5 in groups of 8: 4 and 6 instead of 7 and 21).
// SPAN (16-lane rows; `lane_ok` then covers both halves of the row, and `gbase` is the row's first lane): the M partner slots
// are split between the halves -- the group half owns r < S = (M + 1) / 2, the replica the rest (with M odd its last slot is
// absent).  Each half reads and keys its own partners, fetches the other half's keys across the row (row_ror:8, one move per
// word), ranks its own slots against all M keys and stores only its own slots' rows: the replica stores into the agent's obs_row.
// A slot's rank is the number of keys below its own, whichever half holds them, so every row lands where the one-half form puts it.
template <int GW, int OD, int NT, bool SPAN = false>
__device__ __forceinline__ void write_neighbour_obs(Lds<GW> &lds, int N, int Knb, int ag, int gbase, bool lane_ok,
                                                    float x, float y, float *obs_row) {
    constexpr int M = NT > 0 ? NT - 1 : GW - 1;  // partner slots
    constexpr int S = SPAN ? (M + 1) / 2 : M;    // ... of this lane: slots r0 .. r0 + S - 1 (SPAN: r0 = S in the replica)
    const int r0 = SPAN && (threadIdx.x & GW) != 0 ? S : 0;
    // 64-bit sort keys: (bits of the squared distance, partner index) -- non-negative floats order
    // like their bit patterns, so one unsigned 64-bit compare is the (distance, index) lexicographic
    // test.  Absent partners get keys above every real one.
    unsigned long long key[S > 0 ? S : 1], okey[S > 0 ? S : 1];  // okey (SPAN): the other half's keys
    bool ok[S > 0 ? S : 1];
    int rank[S > 0 ? S : 1], who[S > 0 ? S : 1];
    static_for<0, S>([&](auto RR) {
        constexpr int l = decltype(RR)::value;
        const int r = r0 + l;
        int j = ag + r + 1;
        j = j >= N ? j - N : j;
        j = j & (GW - 1);  // idle lanes (ag >= N) and the replica's absent slot stay inside the group's rows
        who[l] = j;
        const float2 pxy = *reinterpret_cast<const float2 *>(&lds.own[gbase + j][0]);  // partner's (x, y)
        const float dx = pxy.x - x, dy = pxy.y - y;
        const float d2 = dx * dx + dy * dy;
        ok[l] = lane_ok & (r + 1 < N);
        if constexpr (SPAN) ok[l] &= r < M;
        const unsigned int hi = ok[l] ? __builtin_bit_cast(unsigned int, d2) : 0xFFFFFFFFu;
        key[l] = (static_cast<unsigned long long>(hi) << 32) | static_cast<unsigned int>(j);
        if constexpr (SPAN) {  // both words by a move: recomputing j from ag and the other half's r costs three instructions
            const unsigned int ohi = static_cast<unsigned int>(xor_lane_i<8>(static_cast<int>(hi)));
            okey[l] = (static_cast<unsigned long long>(ohi) << 32) | static_cast<unsigned int>(xor_lane_i<8>(j));
        }
        rank[l] = S - 1 - l;  // own pairs in which this slot is the first element; each lost comparison adds one below
    });
    const bool all_others = Knb >= N - 1;
    // rank of a partner = number of partners ahead of it: one comparison per unordered pair (q < k) of this lane's slots
    static_for<1, S>([&](auto KK) {
        constexpr int k = decltype(KK)::value;
        static_for<0, k>([&](auto QQ) {
            constexpr int q = decltype(QQ)::value;
            const int q_first = key[q] < key[k] ? 1 : 0;
            rank[k] += q_first;
            rank[q] -= q_first;
        });
    });
    if constexpr (SPAN) {  // ... and the other half's slots ahead of each of mine
        static_for<0, S>([&](auto LL) {
            constexpr int l = decltype(LL)::value;
            static_for<0, S>([&](auto QQ) { rank[l] += okey[decltype(QQ)::value] < key[l] ? 1 : 0; });
        });
    }
    // the rows first (independent LDS reads in flight together), then the predicated stores
    float row[S > 0 ? S : 1][OD];
    static_for<0, S>([&](auto RR) {
        constexpr int r = decltype(RR)::value;
        const float *src = &lds.own[gbase + who[r]][0];
        if constexpr (OD == 4) {
            const float4 v = *reinterpret_cast<const float4 *>(src);
            row[r][0] = v.x;
            row[r][1] = v.y;
            row[r][2] = v.z;
            row[r][3] = v.w;
        } else {
#pragma unroll
            for (int c = 0; c < OD; ++c) row[r][c] = src[c];
        }
    });
    static_for<0, S>([&](auto RR) {
        constexpr int r = decltype(RR)::value;
        const int j = who[r];
        const int slot = all_others ? (j < ag ? j : j - 1) : rank[r];
        if (ok[r] & (all_others | (slot < Knb))) {
            float *o = obs_row + (slot + 1) * OD;
            if constexpr (OD == 4) {
                out_store4(o, row[r][0], row[r][1], row[r][2], row[r][3]);
            } else {
#pragma unroll
                for (int c = 0; c < OD; ++c) o[c] = row[r][c];
            }
        }
    });
}

// ------------------------------------------------------------------ the step kernel
// The lane predicates of the row kernels' sub-step loop as wave masks (device_common.h lane_mask; step_once PM): the envs of the
// launch and their agents' lanes; the envs still running (env & !dead) and their agents' lanes (lane & !dead); the envs that ended
// in this controller period (died_now); the lanes whose env cannot use the sparse pre-test in this period (lane & !sparse_ok).
struct RowMasks {
    lane_mask env, lane, alive, live, died, dense;
};
struct NoRowMasks {   // (every other kernel: nothing to hold; the names exist for the dead side of `PM ? ... : ...`)
    static constexpr lane_mask env = 0, lane = 0, alive = 0, live = 0, died = 0, dense = 0;
};
// NT: the agent count when it is a compile-time constant (instantiated for GW = 8: 5..8), 0 = read
// it from the parameter block.  One env step of the wave's envs; `sv` = this step's slice of the
// action and output arrays.
// AHEAD: use (and keep filled) the drawn-ahead initial states of rg_state.next_init.  Off in the multi-step launch: there
// the launch costs the MEAN wavefront, and drawing ahead moves the sampler's work without removing any.
// GYM: the gymma block of rg_step_io (gym's TimeLimit + reductions) is compiled in.  Its own instantiations (generic agent
// count, single-step launch): the benchmark kernels carry none of it.
// Sync: how the wave's lanes meet (device_common.h): WgSync in the step kernels (one-wave workgroups), WaveSync where the step
// runs on one wave of a larger workgroup (policy_rollout.h): every barrier below sits under the wave's own control flow.
// LIDAR: the range block of `lid` (lidar.h) goes after the scenario's own columns.  Its own instantiations (lidar_step_kernel).
// TEAM: the agents' capabilities come from set team_index[e] of the pool `tm` (team.h), and an episode that starts here draws
// the env's next index.  Its own instantiations (team_step_kernel).
// SPAN: an env owns a whole 16-lane DPP row (GW = 8): lanes 8..15 of the row (the "helper" half) run a bit-identical replica of
// lanes 0..7 -- same loads, same code, same votes -- and take over part of the env's order-free work (the sparse and dense
// collision pre-tests, whose result is a minimum over pairs and sub-steps; in the epilogue prey 4..7 of PredatorCapturePrey's prey
// pass and the upper half of the neighbour slots).  The replica makes ONE kind of global store: the neighbour rows of the slots it
// owns, into its agent's own obs_row (write_neighbour_obs); every other store is the group half's.  Every DPP exchange and
// reduction at GW = 8 stays inside its 8-lane half (quad permutes, row_half_mirror), so no value mixes the two halves except
// where a result is brought across on purpose (row_ror:8, xor_lane_i<8>).
// NOISE: the pose disturbance of `nz` (disturb.h): the step begins by displacing the poses it has just loaded.  Its own
// instantiations (disturb_step_kernel).
// SH: the members of the parameter block that are compile-time constants here (kernel_args.h Shape; NoShape: none).  The
// resident form's reference shapes only (robogym_resident_shapes.hip); the host launches such a kernel for a handle whose
// block holds exactly these values (match_shape).
template <int SCN, int GW, bool OBS_ONLY, int NT, bool AHEAD, bool GYM, int QPM = 0, typename QpLds = void, typename Sync = WgSync,
          bool LIDAR = false, bool TEAM = false, bool SPAN = false, bool NOISE = false, bool RES = false, class SH = NoShape>
__device__ __forceinline__ void step_once(const KernelArgs &a, Lds<GW> &lds, const StepView &sv, QpLds *qp_lds = nullptr,
                                          const rg_lidar_params *lid = nullptr, const rg_team_params *tm = nullptr,
                                          const DisturbScale *nz = nullptr) {
    static_assert(!SPAN || (GW == 8 && QPM == 0 && !GYM && !LIDAR && !TEAM && !NOISE), "the 16-lane rows: exact mode, GW = 8, no side blocks");
    static_assert(!NOISE || !OBS_ONLY, "an observation-only launch displaces nothing");
    static_assert(!RES || (SPAN && RG_ROW_ARG_REGS != 0), "the resident form: the 16-lane rows, arguments in vector registers");
    static_assert(RES || std::is_same<SH, NoShape>::value, "shapes: the resident form only");
    constexpr int RW = SPAN ? 2 * GW : GW;  // lanes per env
    constexpr int EPW = WAVE / RW;  // envs per wave
    RG_STAMPS_BEGIN()
    const rg_scenario_params &p = a.p;
    const Consts &k = a.k;
    // SPAN: the argument block a second time, in four vector registers (device_common.h load_arg_regs), requested before anything
    // else.  Everything behind the sub-step loop reads its arguments from them: RG_ARG(a.x) / RG_OUT(x) below are one or two
    // v_readlane_b32 there, and the plain a.x / sv.io.x in every other kernel (a single-step launch: sv.io is a.io).
    // RG_ARG_OR(a.x, q): the same for an argument the prologue holds as q.  (Macros, and a conditional on a constant, of which
    // the compiler emits the live side only: every other kernel is compiled from the plain member access, as before.)
    constexpr bool ARGV = SPAN && RG_ROW_ARG_REGS != 0;
    constexpr bool SCHED = SPAN && RG_SHAPE_SCHEDULE != 0 && SH::U > 0 && SH::PERIOD > 0;   // the chunk schedule from the shape (below, at run_chunk)
    // PM: the lane predicates of the sub-step loop as wave masks (below, at `dead`).  The resident row kernels: the ones a handle
    // runs; the by-value row kernels (a handle without an image, RG_STEP_RESIDENT=0) stay as they were.
    constexpr bool PM = SPAN && RES && RG_ROW_PRED_MASKS != 0;
    // RES (the resident form, kernel_args.h): `a` is the handle's image, read like the kernel arguments, and the per-call arguments
    // come through `sv`; in the registers they are the fifth (device_common.h resident_arg_off).
    int av[ARG_REGS] = {0, 0, 0, 0, 0};
    if constexpr (RES) load_arg_regs_resident(a, threadIdx.x, av);
    else if constexpr (ARGV) load_arg_regs(a, threadIdx.x, av);
#define RG_ARG_BLOCK_OFF(f) static_cast<unsigned>(reinterpret_cast<const char *>(&(f)) - reinterpret_cast<const char *>(&a))
#define RG_ARG_OFF(f) (RES ? resident_arg_off(RG_ARG_BLOCK_OFF(f)) : RG_ARG_BLOCK_OFF(f))
#define RG_ARG(f) (ARGV ? arg_reg<std::decay_t<decltype(f)>>(av, RG_ARG_OFF(f)) : (f))
#define RG_ARG_OR(f, q) (ARGV ? arg_reg<std::decay_t<decltype(q)>>(av, RG_ARG_OFF(f)) : (q))
#define RG_OUT(m) (ARGV ? arg_reg<std::decay_t<decltype(sv.io.m)>>(av, RG_ARG_OFF(a.io.m)) : (sv.io.m))
    // RG_SHAPED(F, x): the shape's constant for field F where it has one, the run-time value x where not (NoShape: always x)
#define RG_SHAPED(F, x) (SH::F >= 0 ? SH::F : (x))
    auto arg_elem = [&](const auto &array, int i) {   // element i of an int array of the block that lies in one register (ARGV only)
        const unsigned off = static_cast<unsigned>(reinterpret_cast<const char *>(&array) - reinterpret_cast<const char *>(&a));
        return __builtin_amdgcn_readlane(av[off >> 8], static_cast<int>((off >> 2) & 63) + i);
    };
    static_assert(offsetof(KernelArgs, p.torque) / 256 == (offsetof(KernelArgs, p.torque) + sizeof(rg_scenario_params::torque) - 1) / 256,
                  "arg_elem(p.torque, j): the table lies in one of the argument registers");
    // RG_IMG(ptr): a pointer read from the block with scalar loads.  Of one that was a kernel argument the compiler knows that it
    // is a global one; of one read from the resident image it has to be told, or every access through it is a flat one.
#define RG_IMG(ptr) (RES ? as_global(ptr) : (ptr))
    // RG_SAMPLER_ARGS: the block as the sampler's calls get it.  The image through an address the compiler cannot see through: it
    // would otherwise merge the sampler's loads of the state pointers with the prologue's, keep those values across the whole
    // kernel, and -- at the scalar-register limit -- fetch them again inside the sub-step loop.  (Kernel arguments become loads too
    // late for that merge.)
#define RG_SAMPLER_ARGS (RES ? reopened_image(a) : (a))
    // ---- kernel arguments first: every pointer and scalar the loads below need, fetched TOGETHER.  Left to itself
    // the compiler fetches each kernarg field where it is first used: five dependent scalar-memory round trips, the
    // state loads issued in between and waited for one group at a time -- 3.3 k of a wave's 24 k cycles went by
    // before the first controller (tools/stamp_probe.py).  The empty asm makes all of them live here: one trip.
    const float *q_poses = RG_IMG(a.st.poses), *q_carry = RG_IMG(a.st.carry_dist), *q_ret = RG_IMG(a.st.ep_return), *q_sum = RG_IMG(a.st.done_return_sum);
    const int32_t *q_steps = RG_IMG(a.st.episode_steps), *q_act = sv.actions, *q_cnt = RG_IMG(a.st.done_count), *q_stp = RG_IMG(a.st.done_steps_sum);
    int32_t *q_el = GYM ? sv.io.elapsed : nullptr;  // gymma block (gym TimeLimit's counter)
    const int q_tl = GYM ? sv.io.time_limit : 0;
    const int32_t *q_rc = RG_IMG(a.st.reset_count), *q_nep = AHEAD ? RG_IMG(a.st.next_episode) : nullptr;
    const float *q_nin = AHEAD ? RG_IMG(a.st.next_init) : nullptr;
    const int q_nst = AHEAD ? a.next_stride : 0;
    const int q_E = a.E, q_epw = a.envs_per_wave, q_P = RG_SHAPED(P, p.num_prey), q_N = p.n_agents, q_G = RES ? sv.grid : gridDim.x;
    if constexpr (SH::P < 0)
    asm volatile("" ::"s"(q_poses), "s"(q_carry), "s"(q_ret), "s"(q_sum), "s"(q_steps), "s"(q_act), "s"(q_cnt), "s"(q_stp),
                 "s"(q_E), "s"(q_epw), "s"(q_P), "s"(q_N), "s"(q_G), "s"(q_rc));
    else   // (q_P is a constant: nothing to fetch)
    asm volatile("" ::"s"(q_poses), "s"(q_carry), "s"(q_ret), "s"(q_sum), "s"(q_steps), "s"(q_act), "s"(q_cnt), "s"(q_stp),
                 "s"(q_E), "s"(q_epw), "s"(q_N), "s"(q_G), "s"(q_rc));
    if constexpr (GYM) asm volatile("" ::"s"(q_el), "s"(q_tl));
    if constexpr (AHEAD) asm volatile("" ::"s"(q_nep), "s"(q_nin), "s"(q_nst));
    const float *q_prey = RG_IMG(a.st.prey_loc);
    const uint8_t *q_sen = RG_IMG(a.st.prey_sensed), *q_cap = RG_IMG(a.st.prey_captured), *q_loaded = RG_IMG(a.st.loaded), *q_grid = RG_IMG(a.st.grid);
    const uint8_t *q_pix = RG_IMG(a.st.pixel_type), *q_reached = RG_IMG(a.st.reached_goal);
    const int32_t *q_gcol = RG_IMG(a.st.goal_col), *q_msg = RG_IMG(a.st.messages), *q_zone = RG_IMG(a.st.zone_load), *q_load = RG_IMG(a.st.load);
    if constexpr (SCN == RG_SCN_PREDATOR_CAPTURE_PREY) asm volatile("" ::"s"(q_prey), "s"(q_sen), "s"(q_cap));
    else if constexpr (SCN == RG_SCN_WAREHOUSE) asm volatile("" ::"s"(q_loaded));
    else if constexpr (SCN == RG_SCN_SIMPLE) asm volatile("" ::"s"(q_prey));
    else if constexpr (SCN == RG_SCN_ARCTIC_TRANSPORT) asm volatile("" ::"s"(q_grid), "s"(q_pix), "s"(q_reached), "s"(q_gcol));
    else asm volatile("" ::"s"(q_msg), "s"(q_zone), "s"(q_load));
    int32_t *q_tidx = TEAM ? tm->team_index : nullptr;
    const float *q_tstep = TEAM ? tm->agent_step : nullptr, *q_tsr = TEAM ? tm->sensing_radius : nullptr;
    const float *q_tcr = TEAM ? tm->capture_radius : nullptr;
    const int32_t *q_ttq = TEAM ? tm->torque : nullptr;
    const int q_tC = TEAM ? tm->n_sets : 1;
    if constexpr (TEAM) {
        asm volatile("" ::"s"(q_tidx), "s"(q_tstep), "s"(q_tC));
        if constexpr (SCN == RG_SCN_PREDATOR_CAPTURE_PREY) asm volatile("" ::"s"(q_tsr), "s"(q_tcr));
        else if constexpr (SCN == RG_SCN_MATERIAL_TRANSPORT) asm volatile("" ::"s"(q_ttq));
    }

    // NOISE: the draw's key and the scales, with the rest (read where the poses arrive: no scalar-memory trip there)
    const uint64_t q_seed = NOISE ? a.seed : 0;
    const int64_t q_off = NOISE ? a.env_offset : 0;
    const float q_kxy = NOISE ? nz->k_xy : 0.0f, q_kth = NOISE ? nz->k_theta : 0.0f;
    if constexpr (NOISE) asm volatile("" ::"s"(q_seed), "s"(q_off), "s"(q_kxy), "s"(q_kth));

    const int N = NT > 0 ? NT : q_N;
    const int lane = threadIdx.x;
    const int ag = lane & (GW - 1);
    const int g = lane / RW;
    const int gbase = lane & ~(RW - 1);   // (with SPAN, group reads of LDS rows and ballots see the lower half of the row)
    const bool helper = SPAN && (lane & GW) != 0;
    const int epw = q_epw > 0 ? q_epw : EPW;
    const int chunk = xcd_chunk(q_G);
    const int e = chunk * epw + g;
    const bool env_ok = (g < epw) & (e < q_E);
    const bool lane_ok = env_ok && ag < N;
    const bool env_st = env_ok & !helper, lane_st = lane_ok & !helper;   // the lanes that store
    std::conditional_t<PM, RowMasks, NoRowMasks> rm;                     // PM: env_ok, lane_ok as wave masks (below, at `dead`)
    if constexpr (PM) {
        rm.env = mask_of(g < epw) & mask_of(e < q_E);
        rm.lane = rm.env & mask_of(ag < N);
    }
    const bool lane_nb = SPAN ? lane_ok : lane_st;                       // ... the neighbour rows (write_neighbour_obs)
    const size_t eN = static_cast<size_t>(e) * N;

    // ---- loads, ALL issued before anything waits for one of them (coalesced: a wave covers EPW consecutive
    // envs = one contiguous span per array).  What the first controller needs comes first (loads return in
    // order); what only the epilogue needs is fetched raw and decoded there, so its latency hides behind the
    // sub-step loop (RG_LATE pins the first use of such a value to where it is decoded).
#define RG_LATE(v) asm volatile("" : "+v"(v))
    float x = 0.0f, y = 0.0f, th = 0.0f, carry = 0.0f;
    int act = 4;
    int steps_raw = 0;
    float agent_step = 0.0f, sr = 0.0f, cr = 0.0f;
    float st_ret = 0.0f, st_sum = 0.0f;
    int st_cnt = 0, st_steps = 0;
    const bool stats = (!OBS_ONLY) && q_ret != nullptr;
    int pix = 0, reached = 0;  // ArcticTransport (pix feeds this step's goals)
    int team_raw = 0, tq_raw = 0;  // TEAM: the env's set index (fetched first: the pool loads below depend on it); own torque
    if constexpr (TEAM) {
        if (env_ok) team_raw = q_tidx[e];
    }
    // NOISE: what the draw is keyed by (the env's episode and step), requested before the poses, with everything else
    int nz_rc = 0, nz_steps = 0;
    if constexpr (NOISE) {
        if (env_ok) {
            nz_rc = q_rc[e];
            nz_steps = q_steps[e];
        }
    }
    if (lane_ok) {
        const float *X = q_poses + eN * 3;
        x = X[ag];
        y = X[N + ag];
        th = X[2 * N + ag];
        if constexpr (!OBS_ONLY) act = q_act[eN + ag];
        if constexpr (SCN == RG_SCN_ARCTIC_TRANSPORT) pix = q_pix[eN + ag];
        if constexpr (!TEAM) {
        agent_step = p.agent_step[ag];
        if constexpr (SCN == RG_SCN_PREDATOR_CAPTURE_PREY) {
            sr = p.sensing_radius[ag];
            cr = p.capture_radius[ag];
        }
        }
        if constexpr (!OBS_ONLY) carry = q_carry[eN + ag];
        if constexpr (TEAM) {
            // the lane's row of the env's set, behind the state loads above (they do not wait for the index); the step
            // length feeds the goal, the rest (radii, torque) only the epilogue, where RG_LATE pins their first use
            const size_t ti = static_cast<size_t>(team_clamp(team_raw, q_tC)) * N + ag;
            agent_step = q_tstep[ti];
            if constexpr (SCN == RG_SCN_PREDATOR_CAPTURE_PREY) {
                sr = q_tsr[ti];
                cr = q_tcr[ti];
            }
            if constexpr (SCN == RG_SCN_MATERIAL_TRANSPORT) tq_raw = q_ttq[ti];
        }
    }
    int rc_raw = -1;  // reset_count, for the fused reset of an env that finishes in this launch
    // The env's NEXT initial state, drawn ahead of time into its block of next_init (device_common.h ResetDst) at the
    // end of an earlier launch: fetched now with everything else, so that an env that finishes in this launch -- as a
    // rule the slowest wavefront's, a near-collision env -- starts its next episode with a handful of stores instead of
    // the sampler (Philox, Fisher-Yates through LDS: ~2 k cycles at the very end of the launch's critical path).
    // Only the block's tag is fetched here (4 bytes per env); the block itself is fetched for the few envs that end
    // (load_next below), early enough to hide its latency behind the epilogue.
    const bool ahead = AHEAD && (!OBS_ONLY) && q_nst > 0 && *sv.auto_reset;
    int nx_tag = -2;                               // episode the block was drawn for
    float nx_pose[3] = {0.0f, 0.0f, 0.0f};         // this lane's agent
    float nx_a = 0.0f, nx_b = 0.0f;                // PCP / Simple: prey `ag` (x, y); MaterialTransport: zone load `ag` (bits)
    uint32_t nx_grid[7] = {0, 0, 0, 0, 0, 0, 0};   // ArcticTransport: this lane's 6 terrain dwords + the goal column
    auto load_next = [&](bool want) {              // this lane's share of the env's drawn-ahead block
        if (want) {
            const auto nb = RG_ARG_OR(a.st.next_init, q_nin) + static_cast<size_t>(e) * RG_ARG_OR(a.next_stride, q_nst);
            if (ag < N) {
                nx_pose[0] = nb[ag];
                nx_pose[1] = nb[N + ag];
                nx_pose[2] = nb[2 * N + ag];
            }
            if constexpr (SCN == RG_SCN_PREDATOR_CAPTURE_PREY || SCN == RG_SCN_SIMPLE) {
                if (ag < RG_SHAPED(P, RG_ARG_OR(p.num_prey, q_P))) {
                    nx_a = nb[3 * N + 2 * ag];
                    nx_b = nb[3 * N + 2 * ag + 1];
                }
            } else if constexpr (SCN == RG_SCN_MATERIAL_TRANSPORT) {
                if (ag < 2) nx_a = nb[3 * N + ag];
            } else if constexpr (SCN == RG_SCN_ARCTIC_TRANSPORT) {
                const uint32_t *gb = reinterpret_cast<const uint32_t *>(nb + 3 * N);
#pragma unroll
                for (int t = 0; t < 6; ++t) nx_grid[t] = gb[ag * 6 + t];
                nx_grid[6] = gb[24];
            }
        }
    };
    int el_raw = 0;
    if (env_ok) {
        steps_raw = q_steps[e];
        if (!OBS_ONLY && *sv.auto_reset) rc_raw = q_rc[e];
        if constexpr (GYM) el_raw = q_el[e];
        if (ahead) nx_tag = q_nep[e];
        if (stats && ag == 0) {
            st_ret = q_ret[e];
            st_sum = q_sum[e];
            st_cnt = q_cnt[e];
            st_steps = q_stp[e];
        }
    }
    // scenario state
    uint32_t sen_lo = 0, sen_hi = 0, cap_lo = 0, cap_hi = 0;  // PCP prey flags as bit masks (P <= 64)
    int flag_raw[4] = {0, 0, 0, 0};                          // PCP, P <= 8: this lane's flag bytes, decoded in the epilogue
    int loaded = 0;                                          // Warehouse
    float goal_x = 0.0f, goal_y = 0.0f;                      // Simple
    uint32_t grid_pre[6] = {0, 0, 0, 0, 0, 0};               // ArcticTransport
    int goal_col = 1;
    int load = 0, zone0 = 0, zone1 = 0;                      // MaterialTransport
    int msg[4] = {0, 0, 0, 0};
    // PCP: up to 8 prey (the reference's configurations: 6) go straight into registers now -- every lane
    // of the group loads the same 8 points, one request per group -- so the load latency hides behind
    // the sub-step loop and the epilogue needs no LDS staging; larger prey counts are staged in LDS.
    float2 prey_r[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) prey_r[t] = make_float2(0.0f, 0.0f);
    static_assert(SCN != RG_SCN_ARCTIC_TRANSPORT || GW == 4, "ArcticTransport is a 4-agent scenario");
    if constexpr (SCN == RG_SCN_PREDATOR_CAPTURE_PREY) {
        const int P = q_P;
        if (P <= 8) {
            if (env_ok) {
                const float2 *src = reinterpret_cast<const float2 *>(q_prey) + static_cast<size_t>(e) * P;
                if constexpr (SPAN) {  // each half of the row holds the four prey it scans: 0..3 the group, 4..7 the replica
                    const int t0 = helper ? 4 : 0;
#pragma unroll
                    for (int t = 0; t < 4; ++t) prey_r[t] = src[t0 + t < P ? t0 + t : P - 1];
                } else {
#pragma unroll
                for (int t = 0; t < 8; ++t) prey_r[t] = src[t < P ? t : P - 1];
                }
                if (ag < P) {
                    flag_raw[0] = q_sen[static_cast<size_t>(e) * P + ag];
                    flag_raw[1] = q_cap[static_cast<size_t>(e) * P + ag];
                }
                if constexpr (GW < 8)
                    if (ag + GW < P) {
                        flag_raw[2] = q_sen[static_cast<size_t>(e) * P + ag + GW];
                        flag_raw[3] = q_cap[static_cast<size_t>(e) * P + ag + GW];
                    }
            }
        } else {
            if (env_ok) {
                for (int i = ag; i < 2 * P; i += GW) lds.prey[g][i] = q_prey[static_cast<size_t>(e) * 2 * P + i];
                for (int i = ag; i < P; i += GW) {
                    const uint32_t sb = q_sen[static_cast<size_t>(e) * P + i] != 0;
                    const uint32_t cb = q_cap[static_cast<size_t>(e) * P + i] != 0;
                    if (i < 32) {
                        sen_lo |= sb << i;
                        cap_lo |= cb << i;
                    } else {
                        sen_hi |= sb << (i - 32);
                        cap_hi |= cb << (i - 32);
                    }
                }
            }
            sen_lo = group_or<GW>(sen_lo);
            cap_lo = group_or<GW>(cap_lo);
            if (P > 32) {
                sen_hi = group_or<GW>(sen_hi);
                cap_hi = group_or<GW>(cap_hi);
            }
        }
    } else if constexpr (SCN == RG_SCN_WAREHOUSE) {
        if (lane_ok) loaded = q_loaded[eN + ag];
    } else if constexpr (SCN == RG_SCN_SIMPLE) {
        if (env_ok) {
            goal_x = q_prey[static_cast<size_t>(e) * 2];
            goal_y = q_prey[static_cast<size_t>(e) * 2 + 1];
        }
    } else if constexpr (SCN == RG_SCN_ARCTIC_TRANSPORT) {
        if (env_ok) {
            // 96 terrain bytes = 24 dwords: 6 per lane of the group (GW = 4)
            const uint32_t *gsrc = reinterpret_cast<const uint32_t *>(q_grid + static_cast<size_t>(e) * 96);
#pragma unroll
            for (int t = 0; t < 6; ++t) grid_pre[t] = gsrc[ag * 6 + t];
            goal_col = q_gcol[e];
        }
        if (lane_ok) reached = q_reached[eN + ag];
    } else {
        if (env_ok) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {  // raw: the `% 4` of MaterialTransport.py:119-120 happens in the epilogue
                if (OBS_ONLY || i >= N) msg[i] = q_msg[4 * e + i];
                else msg[i] = q_act[eN + i];
            }
            zone0 = q_zone[2 * e];
            zone1 = q_zone[2 * e + 1];
        }
        if (lane_ok) load = q_load[eN + ag];
    }

    if constexpr (NOISE) {
        // The pose the rest of the step reads: displaced before its first use (disturb.h).  The draw is integer work on the two
        // early loads, pinned HERE, behind every request of the prologue: left free, its first multiply moves up to the two
        // loads and waits for them before the poses are requested -- a second memory round trip on the step's chain.  Pinned,
        // the chain grows by the Philox rounds alone.  (They do not overlap the loads' latency: the requests sit in divergent
        // blocks, behind which a wait for the oldest load is a wait for all of them.)
        RG_LATE(nz_rc);
        RG_LATE(nz_steps);
        int nz_c[3];
        disturb_draw(static_cast<uint64_t>(q_off + e), nz_rc - 1, nz_steps, ag, q_seed, nz_c);
        float dx = x, dy = y, dth = th;
        disturb_pose(q_kxy, q_kth, nz_c, dx, dy, dth);
        x = lane_ok ? dx : x;
        y = lane_ok ? dy : y;
        th = lane_ok ? dth : th;
    }

    int viol = 0, max_sweeps = 0;
    bool replayed = false;  // wave-uniform: some chunk of this step went through the exact-test replay
    float dist = 0.0f;
    if constexpr (!OBS_ONLY) {
        RG_PIN5(x, y, th, carry, act);
        RG_STAMP(0);  // inputs loaded
        // ---- a1 goal generation (agent.py:48-76, warehouse.py:19-45, MaterialTransport.py:19-46)
        float gx = x, gy = y;
        {
            const int mv = (SCN == RG_SCN_MATERIAL_TRANSPORT) ? act / 4 : act;
            float sd = agent_step;
            if constexpr (SCN == RG_SCN_ARCTIC_TRANSPORT) {  // agent.py:89-113: drones 0,1; ice 2; water 3
                const float nrm_s = p.arctic_normal_step, slow_s = p.arctic_slow_step, fast_s = p.arctic_fast_step;
                const float water = pix == 1 ? slow_s : pix == 2 ? fast_s : nrm_s;
                const float ice = pix == 1 ? fast_s : pix == 2 ? slow_s : nrm_s;
                sd = ag < 2 ? fast_s : ag == 3 ? water : ice;
            }
            const float cgx = clamp_spec(gx, p.left, p.right), cgy = clamp_spec(gy, p.up, p.down);
            const float lft = (gx - sd) > p.left ? (gx - sd) : p.left;
            const float rgt = (gx + sd) < p.right ? (gx + sd) : p.right;
            const float upw = (gy - sd) > p.up ? (gy - sd) : p.up;
            const float dwn = (gy + sd) < p.down ? (gy + sd) : p.down;
            gx = mv == 0 ? lft : mv == 1 ? rgt : cgx;
            gy = mv == 2 ? upw : mv == 3 ? dwn : cgy;
        }
        // ---- a2 roboEnv.step (utilities/roboEnv.py:52-94), float spec of oracle/oracle_core.h, one
        // CONTROLLER PERIOD (<= 15 sub-steps with v, w held) at a time: theta and dist_travelled
        // advance once per period by fma; inside the period only x, y and (cos, sin) move.
        //
        // _validate every sub-step: the exact test (GW-1 DPP rounds of float math) runs only in a
        // rare wave-uniform branch.  The common path is a conservative pre-test (kernel_args.h): the
        // collision points rounded to binary16 pairs -- per pair round one DPP + v_pk_add_f16 +
        // v_dot2_f32_f16 -- against a threshold widened by the rounding bound, and one boundary test
        // per chunk on the chunk's first position widened by the chunk's travel.  Absent lanes /
        // finished envs sit on far-apart ghost points.  CHUNK sub-steps are advanced and tested
        // together: their test chains are independent, which is the only ILP a single wavefront has here.
        const int thr_pre = __builtin_bit_cast(int, k.thr_pre);  // non-negative floats order like their bit patterns
        const int ghost_q = __builtin_bit_cast(int, __builtin_amdgcn_cvt_pkrtz(1000.0f + 32.0f * ag, -1000.0f));
        float v = 0.0f, w = 0.0f, s = 0.0f, c = 1.0f;
        RG_CHUNK_LOCALS()
        RG_CTRL_LOCALS()
        float acc = carry, last = 0.0f;  // dist incl. the pending sub-step; length of the last sub-step
        bool dead = false;               // group-uniform: the env hit a violation (roboEnv.py:92-94)
        // PM (the resident row kernels): `dead` and every predicate formed from it as wave masks in scalar registers (device_common.h
        // lane_mask; RowMasks above) -- a bool that is carried around the period and chunk loops and assigned in the replay reaches
        // its uses as an integer in a vector register, turned back into a mask by each of them.  The masks change in the replay
        // alone.  (Every use is under `if constexpr (PM)` or the live side of `PM ? ... : ...`: the other kernels are compiled from
        // the statements they had, and stay instruction-identical.)
        if constexpr (PM) {
            rm.alive = rm.env;
            rm.live = rm.lane;
        }
        float fin_x = 0.0f, fin_y = 0.0f;
        // x, y = period base (bx, by) + displacement since the period began (ox, oy): a sub-step adds
        // dt*v*(cos, sin) to the small displacement and the position is the single rounding bx + ox, so the
        // roundings of the 29..74 Euler updates do not pile up in x, y (float spec, oracle/oracle_core.h)
        float bx = x, by = y, ox = 0.0f, oy = 0.0f;
        const bool penalize = RG_SHAPED(PENALIZE, p.penalize_violations) != 0;
        const int U = RG_SHAPED(U, p.update_frequency), period = RG_SHAPED(PERIOD, p.controller_period);
        for (int it0 = 0; it0 < U; it0 += period) {
            const int n = (U - it0) < period ? (U - it0) : period;
            RG_HEADING_SINCOS(th, s, c);
            const int sw = controller<GW, QPM, QpLds, SPAN>(p, k, N, ag, lane_ok, PM ? mask_lane(rm.alive) : env_ok & !dead, x, y, c, s, gx, gy, v, w, qp_lds RG_CTRL_TICKS_ARG);
            max_sweeps = sw > max_sweeps ? sw : max_sweeps;
            const float dtv = k.dt * v, dtw = k.dt * w;
            float sd, cd;
            sincos_small_spec(dtw, sd, cd);
            if (__any(__builtin_fabsf(dtw) > 0.25f)) {  // only with non-rps time steps / velocity limits
                float sd2, cd2;
                sincos_spec(dtw, sd2, cd2);
                const bool big = __builtin_fabsf(dtw) > 0.25f;
                sd = big ? sd2 : sd;
                cd = big ? cd2 : cd;
            }
            if (it0 == 0) RG_STAMP(1);  // first controller done
            const float mrg = __builtin_fmaf((CHUNK - 1) * 1.000001f, __builtin_fabsf(dtv), PRE_SLACK);
            int n_exec = n;             // sub-steps this env executes in this period
            bool died_now = false;
            if constexpr (PM) rm.died = 0;
            // SPARSE collision pre-test (kernel_args.h): v and w are constant inside the period, so between two sub-steps
            // a robot's collision point moves at most |dt v| (the body) + coll_off |dt w| (the chord of its turn) per
            // sub-step.  A test of sub-step u against a threshold widened by the travel of BOTH robots over `span` further
            // sub-steps (2 span M, M = the group's largest per-sub-step travel) covers sub-steps u .. u + span: a pair that
            // passes it cannot be within the collision distance at any of them.  A chunk tests sub-steps 0 (covering 0..2)
            // and 3 (covering the rest) instead of all five; only a chunk that fails goes on to the per-sub-step pre-test
            // and, from there, to the exact replay -- the masks come from the exact test alone, results are unchanged.
            const float mstep = lane_ok ? __builtin_fmaf(__builtin_fabsf(k.coll_off), __builtin_fabsf(dtw), __builtin_fabsf(dtv)) * 1.00001f : 0.0f;
            const float M2 = 2.0f * group_max_nonneg<GW>(mstep);
            auto thr_span = [&](int span) {  // bits of the squared threshold (non-negative floats order like their bit patterns)
                const float t = (k.lin_pre + PRE_SLACK) + static_cast<float>(span) * M2;
                return __builtin_bit_cast(int, (t * t) * 1.00002f);
            };
            const int thr_s1 = thr_span(1), thr_s2 = thr_span(2);
            // the binary16 rounding bound behind lin_pre holds for differences below 0.25 m per axis
            const bool sparse_ok = (k.lin_pre + 2.0f * M2) < 0.24f;
            if constexpr (PM) rm.dense = rm.lane & ~mask_of((k.lin_pre + 2.0f * M2) < 0.24f);

            // C sub-steps starting at sub-step j0 of this period
            auto run_chunk = [&](auto CC, int j0) {
                constexpr int C = decltype(CC)::value;
                const float x0 = x, y0 = y, ox0 = ox, oy0 = oy, c0 = c, s0 = s;
                const bool live = PM ? mask_lane(rm.live) : lane_ok & !dead;
                int q[C];
                // every pre-update position of the chunk lies within (C-1)|dt v| of the first
                const bool bnd_any = live & ((__builtin_fabsf(x - k.xc) + mrg > k.xh) | (__builtin_fabsf(y - k.yc) + mrg > k.yh));
                lane_mask out_m = 0, hit_m = 0;   // PM: bnd_any before `live`; the pre-test's own hits (sparse_hit without `live & !sparse_ok`)
                int q03 = 0;                      // PM: the point the sparse pre-test of this half of the row reads
                if constexpr (PM) out_m = mask_of(__builtin_fabsf(x - k.xc) + mrg > k.xh) | mask_of(__builtin_fabsf(y - k.yc) + mrg > k.yh);
                static_for<0, C>([&](auto UU) {
                    constexpr int u = decltype(UU)::value;
                    const float fx = __builtin_fmaf(k.coll_off, c, x), fy = __builtin_fmaf(k.coll_off, s, y);
                    const int qr = __builtin_bit_cast(int, __builtin_amdgcn_cvt_pkrtz(fx, fy));
                    q[u] = live ? qr : ghost_q;
                    // (one select between the halves' sub-steps, one against the ghost: q[0], q[3] are then the dense path's only)
                    if constexpr (PM && C >= 4 && (u == 0 || u == 3)) q03 = helper == (u == 3) ? qr : q03;
                    // Euler step (Appendix A.4); rotate (cos, sin) by dt*w
                    ox = __builtin_fmaf(c, dtv, ox);
                    oy = __builtin_fmaf(s, dtv, oy);
                    x = bx + ox;
                    y = by + oy;
                    const float cn = __builtin_fmaf(c, cd, -(s * sd));
                    const float sn = __builtin_fmaf(s, cd, c * sd);
                    c = cn;
                    s = sn;
                });
                // smallest squared distance (bits) between this lane's rounded collision point and its partners'
                auto pair_min = [&](int qv) {
                    // the pre-test may visit the pairs in any order.  5 <= N <= 7 in groups of 8: the three quad rounds
                    // cover the pairs inside each quad, then each agent of the upper quad (4 .. N-1) is broadcast over
                    // its quad and mirrored onto the lower one: 3 + (N-4) rounds instead of 7
                    constexpr bool QUAD_COVER = GW == 8 && NT >= 5 && NT <= 7;
                    constexpr int R = QUAD_COVER ? NT - 1 : GW - 1;
                    int d[R];
                    auto diff = [&](int partner_q) {
                        return __builtin_bit_cast(int, __builtin_bit_cast(half2v, qv) - __builtin_bit_cast(half2v, partner_q));
                    };
                    if constexpr (QUAD_COVER) {
                        static_for<1, 4>([&](auto KK) { d[decltype(KK)::value - 1] = diff(xor_lane_i<decltype(KK)::value>(qv)); });
                        static_for<0, NT - 4>([&](auto MM) { d[3 + decltype(MM)::value] = diff(cross_lane_i<decltype(MM)::value>(qv)); });
                    } else {
                        static_for<1, GW>([&](auto KK) { d[decltype(KK)::value - 1] = diff(xor_lane_i<decltype(KK)::value>(qv)); });
                    }
                    int dm = 0x7FFFFFFF;
                    dot2_batch<R>(d);
#pragma unroll
                    for (int r = 0; r < R; ++r) dm = d[r] < dm ? d[r] : dm;
                    return dm;
                };
                // sparse pre-test: sub-step 0 covers 0 .. min(2, C-1), sub-step 3 the rest of the chunk; a chunk that fails
                // adds the remaining sub-steps (the dense pre-test of rounds 1-2: every sub-step against the unwidened
                // threshold), so a failing chunk costs what every chunk used to cost
                int dmin_u[C];  // per sub-step: the replay runs the exact pair test only where the pre-test fired
                bool sparse_hit = live & !sparse_ok;
                {
                    constexpr int SPAN0 = C - 1 < 2 ? C - 1 : 2;
                    const int t0 = SPAN0 == 0 ? thr_pre : SPAN0 == 1 ? thr_s1 : thr_s2;
                    if constexpr (SPAN && C >= 4) {
                        // the group tests sub-step 0, its replica sub-step 3; the wave's vote below ORs the two halves' hits,
                        // and each half's minimum goes across only if the chunk goes on to the dense pre-test
                        const int t3 = C == 4 ? thr_pre : thr_s1;
                        const int dm = pair_min(PM ? (live ? q03 : ghost_q) : helper ? q[3] : q[0]);
                        sparse_hit = sparse_hit | (dm <= (helper ? t3 : t0));
                        if constexpr (PM) hit_m = mask_of(dm <= (helper ? t3 : t0));
                        dmin_u[0] = dmin_u[3] = dm;
                    } else {
                        dmin_u[0] = pair_min(q[0]);
                        sparse_hit = sparse_hit | (dmin_u[0] <= t0);
                        if constexpr (PM) hit_m = mask_of(dmin_u[0] <= t0);
                        if constexpr (C >= 4) {
                            const int t3 = C == 4 ? thr_pre : thr_s1;
                            dmin_u[3] = pair_min(q[3]);
                            sparse_hit = sparse_hit | (dmin_u[3] <= t3);
                            if constexpr (PM) hit_m |= mask_of(dmin_u[3] <= t3);
                        }
                    }
                }
                if (penalize && (PM ? (hit_m | (rm.live & (out_m | rm.dense))) != 0 : __any(sparse_hit | bnd_any))) {
                RG_CHUNK_DENSE_BEGIN()
                if constexpr (SPAN && C >= 4) {  // sub-step 0's minimum from the group, 3's from the replica, into both halves
                    const int mine = dmin_u[0], other = xor_lane_i<8>(mine);
                    dmin_u[0] = helper ? other : mine;
                    dmin_u[3] = helper ? mine : other;
                }
                if constexpr (SPAN && C >= 3) {  // sub-steps 1 and 2 side by side in the two halves; 4 (C = 5) in both
                    const int mine = pair_min(helper ? q[2] : q[1]), other = xor_lane_i<8>(mine);
                    if constexpr (C == 5) dmin_u[4] = pair_min(q[4]);
                    dmin_u[1] = helper ? other : mine;
                    dmin_u[2] = helper ? mine : other;
                } else {
                    static_for<1, C>([&](auto UU) {
                        constexpr int u = decltype(UU)::value;
                        if constexpr (u != 3) dmin_u[u] = pair_min(q[u]);
                    });
                }
                int dmin = dmin_u[0];
                static_for<1, C>([&](auto UU) { dmin = dmin_u[decltype(UU)::value] < dmin ? dmin_u[decltype(UU)::value] : dmin; });
                RG_CHUNK_DENSE_END(dmin)
                if (PM ? (mask_of(dmin <= thr_pre) | (rm.live & out_m)) != 0 : __any((dmin <= thr_pre) | bnd_any)) {
                    replayed = true;
                    // rare: replay the chunk with the exact float tests of _validate (roboEnv.py:82-94): the
                    // boundary test on every sub-step (per lane, cheap), the pair rounds only on the sub-steps
                    // whose own pre-test fired somewhere in the wave (robots cross the 3 mm pre-test band
                    // within a sub-step or two: most sub-steps of a flagged chunk need no pair rounds)
                    float rx = x0, ry = y0, rox = ox0, roy = oy0, rc = c0, rs = s0;
                    static_for<0, C>([&](auto UU) {
                        constexpr int u = decltype(UU)::value;
                        // (`dead` changes from sub-step to sub-step here, and rm.live with it)
                        const bool bnd = (PM ? mask_lane(rm.live) : lane_ok & !dead) & ((rx < k.xmin) | (rx > k.xmax) | (ry < k.ymin) | (ry > k.ymax));
                        const float fx = __builtin_fmaf(k.coll_off, rc, rx), fy = __builtin_fmaf(k.coll_off, rs, ry);
                        bool col = false;
                        // The binary16 figure is a bound for collision points within 0.25 m of the arena only (kernel_args.h).
                        // A robot farther out was put there before the step (a loaded pose; one that walks out ends its env
                        // at the wall) and ends its env in the step's FIRST sub-step: there, with a robot of the wave outside
                        // the arena, the pair rounds run whatever the figure says.
                        bool pairs = __any(dmin_u[u] <= thr_pre);
                        if constexpr (u == 0) {
                            if ((it0 | j0) == 0) pairs = pairs || __any(bnd);
                        }
                        if (!pairs) {
                            // no pair of this sub-step is within the pre-test band: no collision possible
                        } else if constexpr (GW == 8 && NT >= 5 && NT <= 7) {  // same pair cover as the pre-test: 3 + (N-4) rounds
                            static_for<1, 4>([&](auto KK) {
                                constexpr int K = decltype(KK)::value;
                                const float dx = fx - xor_lane<K>(fx), dy = fy - xor_lane<K>(fy);
                                col = col | (((ag ^ K) < N) & (dx * dx + dy * dy <= k.coll_lim2));
                            });
                            static_for<0, NT - 4>([&](auto MM) {  // lower lanes meet agent 4+M, upper lanes agent M
                                constexpr int M = decltype(MM)::value;
                                const float dx = fx - cross_lane<M>(fx), dy = fy - cross_lane<M>(fy);
                                col = col | (dx * dx + dy * dy <= k.coll_lim2);
                            });
                        } else {
                            static_for<1, GW>([&](auto KK) {
                                constexpr int K = decltype(KK)::value;
                                const float dx = fx - xor_lane<K>(fx), dy = fy - xor_lane<K>(fy);
                                col = col | (((ag ^ K) < N) & (dx * dx + dy * dy <= k.coll_lim2));
                            });
                        }
                        col = PM ? col & mask_lane(rm.live) : col & lane_ok & !dead;
                        const int code = (group_any<GW>(col, gbase) ? 1 : 0) | (group_any<GW>(bnd, gbase) ? 2 : 0);
                        rox = __builtin_fmaf(rc, dtv, rox);  // the violating sub-step is still integrated
                        roy = __builtin_fmaf(rs, dtv, roy);
                        rx = bx + rox;
                        ry = by + roy;
                        lane_mask die_m = 0;   // PM: the envs that end in this sub-step
                        if constexpr (PM) die_m = rm.alive & mask_of(code != 0);
                        if (PM ? mask_lane(die_m) : env_ok & !dead & (code != 0)) {
                            viol = code;
                            n_exec = j0 + u + 1;
                            died_now = true;
                            dead = true;
                            fin_x = rx;
                            fin_y = ry;
                        }
                        if constexpr (PM) {
                            rm.alive &= ~die_m;
                            rm.live &= ~die_m;
                            rm.died |= die_m;
                        }
                        const float cn = __builtin_fmaf(rc, cd, -(rs * sd));
                        const float sn = __builtin_fmaf(rs, cd, rc * sd);
                        rc = cn;
                        rs = sn;
                    });
                    RG_CHUNK_REPLAY_END(rx, ry)
                }
                }
            };
            if constexpr (SCHED) {
                // The shape fixes the schedule: every period but the last is F full chunks and a remainder of R sub-steps, the last
                // one FL and RL.  The FC full chunks both kinds have are one loop to a constant bound; ONE decision -- is this the
                // last period? -- picks what follows, at constant j0, nothing where a remainder is 0: in place of the loop to a
                // run-time bound and the chain of tests on n - j.  (29 sub-steps in periods of 15: 5 5 | 5, then 5 5 | 4.)  The loop
                // stays rolled: each copy of a chunk carries its dense pre-test and its replay.
                constexpr int PER = SH::PERIOD, LASTN = SH::U - PER * ((SH::U - 1) / PER);
                constexpr int F = PER / CHUNK, R = PER % CHUNK, FL = LASTN / CHUNK, RL = LASTN % CHUNK, FC = F < FL ? F : FL;
#pragma nounroll
                for (int j = 0; j < FC * CHUNK; j += CHUNK) run_chunk(std::integral_constant<int, CHUNK>{}, j);
                if (it0 + PER < SH::U) {
                    static_for<FC, F>([&](auto II) { run_chunk(std::integral_constant<int, CHUNK>{}, decltype(II)::value * CHUNK); });
                    if constexpr (R > 0) run_chunk(std::integral_constant<int, R>{}, F * CHUNK);
                } else {
                    static_for<FC, FL>([&](auto II) { run_chunk(std::integral_constant<int, CHUNK>{}, decltype(II)::value * CHUNK); });
                    if constexpr (RL > 0) run_chunk(std::integral_constant<int, RL>{}, FL * CHUNK);
                }
            } else {
            int j = 0;
            for (; j + CHUNK <= n; j += CHUNK) run_chunk(std::integral_constant<int, CHUNK>{}, j);
            static_for<1, CHUNK>([&](auto RR) {  // the remainder as one shorter chunk
                if (n - j == decltype(RR)::value) run_chunk(RR, j);
            });
            }

            // period end: heading and distance for the sub-steps this env executed
            const bool upd = PM ? mask_lane(rm.alive | rm.died) : env_ok & (!dead | died_now);
            const float ne = static_cast<float>(n_exec);
            const float adv = __builtin_fabsf(dtv);
            th = upd ? wrap_spec(__builtin_fmaf(ne, dtw, th)) : th;
            acc = upd ? __builtin_fmaf(ne, adv, acc) : acc;
            last = upd ? adv : last;
            {   // base <- base + displacement (= x, y as last formed); displacement <- the exact remainder (TwoSum)
                const float tx = x - bx, ty = y - by;
                ox = (bx - (x - tx)) + (ox - tx);
                oy = (by - (y - ty)) + (oy - ty);
                bx = x;
                by = y;
            }
            if (it0 == 0) RG_STAMP(2);  // first period done
            if (PM ? rm.alive == 0 : !__any(env_ok & !dead)) break;
        }
        if (PM ? mask_lane(rm.env & ~rm.alive) : dead) {
            x = fin_x;
            y = fin_y;
        }
        dist = viol ? acc : acc - last;
        carry = last;
        RG_STAMP(3);  // all periods done
        RG_CTRL_REPORT()
        RG_CHUNK_REPORT()
    }

    // ---- scenario epilogue
    const int D = RG_SHAPED(D, RG_ARG(p.obs_dim));
    const auto obs_row = RG_OUT(obs) + (eN + ag) * D;
    // (SPAN: the prologue's flags formed again from the registers, rather than fetched again)
    const bool ahead_e = ARGV ? AHEAD && (!OBS_ONLY) && RG_ARG(a.next_stride) > 0 && RG_ARG(a.auto_reset) : ahead;
    const bool stats_e = ARGV ? (!OBS_ONLY) && RG_ARG(a.st.ep_return) != nullptr : stats;
    bool done = false;
    int remaining = -1;
    float reward = 0.0f;
    RG_LATE(steps_raw);
    const int steps = steps_raw + (OBS_ONLY ? 0 : 1);
    // an env that ends by a violation or by the step limit (all but a few endings) is known to end already: its
    // drawn-ahead block is fetched now, behind the epilogue
    RG_LATE(rc_raw);
    RG_LATE(nx_tag);
    const bool have_next = ahead_e & (nx_tag == rc_raw);  // the block holds exactly the episode that would start now
    const bool next_early = env_ok & have_next & ((viol != 0) | (steps > RG_ARG(p.max_episode_steps)));
    if constexpr (AHEAD) load_next(next_early & !helper);

    if constexpr (SCN == RG_SCN_PREDATOR_CAPTURE_PREY) {
        const int P = RG_SHAPED(P, RG_ARG_OR(p.num_prey, q_P));
        if constexpr (TEAM) {
            RG_LATE(sr);
            RG_LATE(cr);
        }
        const float sr2 = sr * sr, cr2 = cr * cr;
        if (P > 8) Sync::sync();  // LDS prey block visible (single-wave workgroup: waitcnt + s_barrier)
        if (P <= 8) {  // the flag bytes fetched in the prologue -> bit masks of the env
            RG_LATE(flag_raw[0]);
            RG_LATE(flag_raw[1]);
            uint32_t sb = (flag_raw[0] != 0 ? 1u : 0u) << ag, cb = (flag_raw[1] != 0 ? 1u : 0u) << ag;
            if constexpr (GW < 8) {
                RG_LATE(flag_raw[2]);
                RG_LATE(flag_raw[3]);
                sb |= (flag_raw[2] != 0 ? 1u : 0u) << (ag + GW);
                cb |= (flag_raw[3] != 0 ? 1u : 0u) << (ag + GW);
            }
            sen_lo = group_or<GW>(sb);
            cap_lo = group_or<GW>(cb);
        }
        uint32_t nsen_lo = sen_lo, nsen_hi = sen_hi, ncap_lo = cap_lo, ncap_hi = cap_hi;
        // The prey block is scanned four at a time (LDS reads in flight together).  scan(lo, hi, f)
        // calls f(i, prey_x, prey_y, d2) for i in [lo, hi).
        auto scan = [&](int lo, int hi, auto &&f) {
            for (int i0 = lo; i0 < hi; i0 += 4) {
                float2 pl[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int i = (i0 + t) < hi ? (i0 + t) : (hi - 1);
                    pl[t] = *reinterpret_cast<const float2 *>(&lds.prey[g][2 * i]);
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float dx = x - pl[t].x, dy = y - pl[t].y;
                    f(i0 + t, (i0 + t) < hi, pl[t].x, pl[t].y, dx * dx + dy * dy);
                }
            }
        };
        float closest = -1.0f, qx = -5.0f, qy = -5.0f;
        if (SPAN && P <= 8) {
            // 16-lane rows: the prey pass split between the halves of the row.  prey_r[0 .. 3] holds prey t0 .. t0 + 3 of this
            // half (t0 = 0 in the group half, 4 in the replica), slots past the end a copy of prey P - 1.
            const float2 (&pl)[8] = prey_r;
            const int t0 = helper ? 4 : 0;
            // the membership tests with the lane's conditions folded into the radii: a squared distance is >= 0 (or NaN), so
            // against -1 no test passes -- an idle lane senses nothing, a lane that does not play 'no_action' captures nothing.
            // A copy of prey P - 1 sets its bit at its own slot's index >= P; `in_p` drops those after the reduction.
            const bool acts = lane_ok & (act == 4);
            const float sr2e = lane_ok ? sr2 : -1.0f, cr2e = acts ? cr2 : -1.0f;
            float d2[4];
            uint32_t m = 0;  // bits 0..3: prey t0 + t within this agent's sensing radius; bits 8..11: within its capture radius
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float dx = x - pl[t].x, dy = y - pl[t].y;
                d2[t] = dx * dx + dy * dy;
                m |= (d2[t] <= sr2e ? 1u : 0u) << t;
                m |= (d2[t] <= cr2e ? 1u : 0u) << (8 + t);
            }
            m <<= t0;
            m = group_or<GW>(m);                            // over the agents of this half: its four prey
            m |= static_cast<uint32_t>(xor_lane_i<8>(static_cast<int>(m)));  // and the other half's: all 16 lanes hold all 8
            const uint32_t in_p = (1u << P) - 1u;
            if constexpr (!OBS_ONLY) {  // a11 _update_tracking_and_locations (PredatorCapturePrey.py:72-95)
                const uint32_t s_b = m & in_p, c_b = (m >> 8) & in_p;
                nsen_lo = sen_lo | (s_b & ~cap_lo);            // sensed: any agent in range, prey not yet captured
                ncap_lo = cap_lo | (nsen_lo & c_b & ~cap_lo);  // captured: sensed and a 'no_action' agent in range
                if (env_st && ag < P) {
                    RG_ARG(a.st.prey_sensed)[static_cast<size_t>(e) * P + ag] = (nsen_lo >> ag) & 1u;
                    RG_ARG(a.st.prey_captured)[static_cast<size_t>(e) * P + ag] = (ncap_lo >> ag) & 1u;
                }
            }
            // a13 nearest uncaptured prey within the agent's own sensing radius.  The sequential scan over t = 0 .. P - 1 takes
            // a prey iff it is eligible and strictly nearer than the best so far, so it ends with the LOWEST index among the
            // eligible prey at the minimal distance.  Each half runs that scan over its own four prey from "none"; the group
            // half then takes the replica's candidate iff the replica has one and the group has none or the replica's is
            // STRICTLY nearer: at equal distance the group's stays, whose index is the lower one (0..3 against 4..7).  That is
            // the candidate the one scan over all eight ends with.  (The copies of prey P - 1 count as captured here: never
            // eligible.)  Only the group half's qx, qy are read afterwards.
            const uint32_t cap_l = (ncap_lo | ~in_p) >> t0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const bool cap = ((cap_l >> t) & 1u) != 0;
                const bool take = !cap & (d2[t] <= sr2) & ((d2[t] < closest) | (closest == -1.0f));
                qx = take ? pl[t].x : qx;
                qy = take ? pl[t].y : qy;
                closest = take ? d2[t] : closest;
            }
            const float o_closest = xor_lane<8>(closest), o_qx = xor_lane<8>(qx), o_qy = xor_lane<8>(qy);
            const bool other = (o_closest != -1.0f) & ((closest == -1.0f) | (o_closest < closest));
            qx = other ? o_qx : qx;
            qy = other ? o_qy : qy;
        } else if (P <= 8) {
            // common case (P = 6): the whole prey block in registers, one pass for tracking and
            // the nearest-prey search, no second trip to LDS
            const float2 (&pl)[8] = prey_r;
            float d2[8];
            uint32_t s_b = 0, c_b = 0;
            const bool acts = lane_ok & (act == 4);
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const float dx = x - pl[t].x, dy = y - pl[t].y;
                d2[t] = dx * dx + dy * dy;
                const bool in = t < P;
                s_b |= ((in & lane_ok & (d2[t] <= sr2)) ? 1u : 0u) << t;
                c_b |= ((in & acts & (d2[t] <= cr2)) ? 1u : 0u) << t;
            }
            if constexpr (!OBS_ONLY) {  // a11 _update_tracking_and_locations (PredatorCapturePrey.py:72-95)
                s_b = group_or<GW>(s_b);
                c_b = group_or<GW>(c_b);
                nsen_lo = sen_lo | (s_b & ~cap_lo);            // sensed: any agent in range, prey not yet captured
                ncap_lo = cap_lo | (nsen_lo & c_b & ~cap_lo);  // captured: sensed and a 'no_action' agent in range
                if (env_st && ag < P) {
                    a.st.prey_sensed[static_cast<size_t>(e) * P + ag] = (nsen_lo >> ag) & 1u;
                    a.st.prey_captured[static_cast<size_t>(e) * P + ag] = (ncap_lo >> ag) & 1u;
                }
                if constexpr (GW < 8)
                    if (env_ok && ag + GW < P) {
                        a.st.prey_sensed[static_cast<size_t>(e) * P + ag + GW] = (nsen_lo >> (ag + GW)) & 1u;
                        a.st.prey_captured[static_cast<size_t>(e) * P + ag + GW] = (ncap_lo >> (ag + GW)) & 1u;
                    }
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {  // a13 nearest uncaptured prey within the agent's own sensing radius
                const bool cap = ((ncap_lo >> t) & 1u) != 0;
                const bool take = (t < P) & !cap & (d2[t] <= sr2) & ((d2[t] < closest) | (closest == -1.0f));
                qx = take ? pl[t].x : qx;
                qy = take ? pl[t].y : qy;
                closest = take ? d2[t] : closest;
            }
        } else {
        if constexpr (!OBS_ONLY) {  // a11, general P
            uint32_t s_lo = 0, s_hi = 0, c_lo = 0, c_hi = 0;  // prey this agent senses / could capture
            const bool acts = lane_ok & (act == 4);
            const int P32 = P < 32 ? P : 32;
            scan(0, P32, [&](int i, bool in, float, float, float d2) {
                s_lo |= ((in & lane_ok & (d2 <= sr2)) ? 1u : 0u) << (i & 31);
                c_lo |= ((in & acts & (d2 <= cr2)) ? 1u : 0u) << (i & 31);
            });
            s_lo = group_or<GW>(s_lo);
            c_lo = group_or<GW>(c_lo);
            nsen_lo = sen_lo | (s_lo & ~cap_lo);
            ncap_lo = cap_lo | (nsen_lo & c_lo & ~cap_lo);
            if (P > 32) {
                scan(32, P, [&](int i, bool in, float, float, float d2) {
                    s_hi |= ((in & lane_ok & (d2 <= sr2)) ? 1u : 0u) << ((i - 32) & 31);
                    c_hi |= ((in & acts & (d2 <= cr2)) ? 1u : 0u) << ((i - 32) & 31);
                });
                s_hi = group_or<GW>(s_hi);
                c_hi = group_or<GW>(c_hi);
                nsen_hi = sen_hi | (s_hi & ~cap_hi);
                ncap_hi = cap_hi | (nsen_hi & c_hi & ~cap_hi);
            }
            if (env_st) {
                for (int i = ag; i < P; i += GW) {
                    const uint32_t sw_ = i < 32 ? nsen_lo >> i : nsen_hi >> (i - 32);
                    const uint32_t cw_ = i < 32 ? ncap_lo >> i : ncap_hi >> (i - 32);
                    RG_ARG(a.st.prey_sensed)[static_cast<size_t>(e) * P + i] = sw_ & 1u;
                    RG_ARG(a.st.prey_captured)[static_cast<size_t>(e) * P + i] = cw_ & 1u;
                }
            }
        }
        {   // a13, general P
            auto nearest = [&](uint32_t capmask, int base) {
                return [&, capmask, base](int i, bool in, float px, float py, float d2) {
                    const bool cap = ((capmask >> ((i - base) & 31)) & 1u) != 0;
                    const bool take = in & !cap & (d2 <= sr2) & ((d2 < closest) | (closest == -1.0f));
                    qx = take ? px : qx;
                    qy = take ? py : qy;
                    closest = take ? d2 : closest;
                };
            };
            scan(0, P < 32 ? P : 32, nearest(ncap_lo, 0));
            if (P > 32) scan(32, P, nearest(ncap_hi, 32));
        }
        }
        RG_STAMP_E(0);  // prey tracked, nearest prey found
        const int od = RG_SHAPED(CA, RG_ARG(p.capability_aware)) ? 6 : 4;
        lds.own[lane][0] = x;
        lds.own[lane][1] = y;
        lds.own[lane][2] = qx;
        lds.own[lane][3] = qy;
        lds.own[lane][4] = sr;
        lds.own[lane][5] = cr;
        Sync::sync();
        if (od == 6) {
            if (lane_st) {
#pragma unroll
                for (int cc = 0; cc < 6; ++cc) obs_row[cc] = lds.own[lane][cc];
            }
            write_neighbour_obs<GW, 6, NT, SPAN>(lds, N, RG_SHAPED(M, RG_ARG(p.num_neighbors)), ag, gbase, lane_nb, x, y, obs_row);
        } else {
            if (lane_st) out_store4(obs_row, x, y, qx, qy);
            write_neighbour_obs<GW, 4, NT, SPAN>(lds, N, RG_SHAPED(M, RG_ARG(p.num_neighbors)), ag, gbase, lane_nb, x, y, obs_row);
        }
        RG_STAMP_E(1);  // observations written
        if constexpr (!OBS_ONLY) {  // a14 reward / termination (PredatorCapturePrey.py:155-176, 209-216)
            const int unseen0 = P - __builtin_popcount(sen_lo) - __builtin_popcount(sen_hi);
            const int left0 = P - __builtin_popcount(cap_lo) - __builtin_popcount(cap_hi);
            const int unseen1 = P - __builtin_popcount(nsen_lo) - __builtin_popcount(nsen_hi);
            const int left1 = P - __builtin_popcount(ncap_lo) - __builtin_popcount(ncap_hi);
            if (viol) {
                reward = RG_ARG(p.violation_reward);
                done = true;
            } else {
                reward = 0.0f;
                reward = reward + static_cast<float>(unseen0 - unseen1) * RG_ARG(p.sense_reward);
                reward = reward + static_cast<float>(left0 - left1) * RG_ARG(p.capture_reward);
                reward = reward + RG_ARG(p.time_penalty);
                if (steps > RG_ARG(p.max_episode_steps) || left1 == 0) {
                    done = true;
                    remaining = left1;
                }
            }
        }
    } else if constexpr (SCN == RG_SCN_WAREHOUSE) {  // a15 (warehouse.py:102-178): obs BEFORE the reward mutates `loaded`
        lds.own[lane][0] = x;
        lds.own[lane][1] = y;
        lds.own[lane][2] = loaded ? 1.0f : 0.0f;
        Sync::sync();
        if (lane_st) {
            obs_row[0] = x;
            obs_row[1] = y;
            obs_row[2] = loaded ? 1.0f : 0.0f;
        }
        write_neighbour_obs<GW, 3, NT, SPAN>(lds, N, RG_SHAPED(M, RG_ARG(p.num_neighbors)), ag, gbase, lane_nb, x, y, obs_row);
        if constexpr (!OBS_ONLY) {
            if (viol) {
                reward = RG_ARG(p.violation_reward);
                done = true;
            } else {
                const bool green = (ag % 2) == 0;  // warehouse.py:63-65
                if (loaded) {
                    if (x < -1.5f + RG_ARG(p.goal_width) && ((green && y > 0.0f) || (!green && y <= 0.0f))) {
                        reward = RG_ARG(p.unload_reward);
                        loaded = 0;
                    }
                } else {
                    if (x > 1.5f - RG_ARG(p.goal_width) && ((!green && y > 0.0f) || (green && y <= 0.0f))) {
                        reward = RG_ARG(p.load_reward);
                        loaded = 1;
                    }
                }
                done = steps > RG_ARG(p.max_episode_steps);
                if (lane_st) RG_ARG(a.st.loaded)[eN + ag] = static_cast<uint8_t>(loaded);
            }
        }
    } else if constexpr (SCN == RG_SCN_SIMPLE) {  // scenarios/Simple/simple.py:155-225
        lds.own[lane][0] = x;
        lds.own[lane][1] = y;
        Sync::sync();
        if (lane_st) {
            obs_row[0] = x;
            obs_row[1] = y;
            obs_row[2 * N] = goal_x;
            obs_row[2 * N + 1] = goal_y;
        }
        write_neighbour_obs<GW, 2, NT, SPAN>(lds, N, N - 1, ag, gbase, lane_nb, x, y, obs_row);  // all others, index order
        if constexpr (!OBS_ONLY) {
            if (viol) {
                reward = RG_ARG(p.violation_reward);
                done = true;
            } else {
                const float dx = x - goal_x, dy = y - goal_y;
                const float r = -(dx * dx + dy * dy);
                reward = r * RG_ARG(p.reward_scaler);
                done = steps > RG_ARG(p.max_episode_steps);
            }
        }
    } else if constexpr (SCN == RG_SCN_ARCTIC_TRANSPORT) {  // ArcticTransport.py:84-143, agent.py:14-87
        {
            uint32_t *gdst = reinterpret_cast<uint32_t *>(&lds.grid[g][0]);
#pragma unroll
            for (int t = 0; t < 6; ++t) gdst[ag * 6 + t] = grid_pre[t];
        }
        Sync::sync();
        const uint8_t *grid = &lds.grid[g][0];
        // get_cell_from_pose: int() truncates toward zero; /0.25 is exact
        int row = -static_cast<int>((y - 1.0f) / 0.25f), col = static_cast<int>((x + 1.5f) / 0.25f);
        row = row < 0 ? 0 : row > 7 ? 7 : row;
        col = col < 0 ? 0 : col > 11 ? 11 : col;
        if constexpr (!OBS_ONLY) {
            pix = grid[row * 12 + col];
            reached = reached | (pix == 3 ? 1 : 0);
        }
        const int here = grid[row * 12 + col];
        lds.own[lane][0] = x;
        lds.own[lane][1] = y;
        lds.own[lane][2] = static_cast<float>(here);
        lds.aload[lane] = row * 16 + col;
        Sync::sync();
        const float goalx = static_cast<float>(goal_col) * 0.25f - 1.5f, goaly = -1.0f * 0.25f + 0.75f;
        if (lane_ok) {
            obs_row[0] = x;
            obs_row[1] = y;
            obs_row[2] = static_cast<float>(here);
            // the other three in the order of agent.py:42-69: {1,2,3} {0,2,3} {3,0,1} {2,0,1}
            const int o0 = ag == 0 ? 1 : ag == 1 ? 0 : ag == 2 ? 3 : 2;
            const int o1 = ag < 2 ? 2 : 0, o2 = ag < 2 ? 3 : 1;
            const int oth[3] = {o0, o1, o2};
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                obs_row[3 + 3 * m + 0] = lds.own[gbase + oth[m]][0];
                obs_row[3 + 3 * m + 1] = lds.own[gbase + oth[m]][1];
                obs_row[3 + 3 * m + 2] = lds.own[gbase + oth[m]][2];
            }
            obs_row[12] = goalx;
            obs_row[13] = goaly;
#pragma unroll
            for (int i = 0; i < 2; ++i) {  // the 8 cells around each drone, edges clamped
                const int rc = lds.aload[gbase + i];
                const int r_ = rc >> 4, c_ = rc & 15;
                const int left = c_ > 0 ? c_ - 1 : c_, right = c_ < 11 ? c_ + 1 : c_;
                const int up = r_ > 0 ? r_ - 1 : r_, down = r_ < 7 ? r_ + 1 : r_;
                float *o = obs_row + 14 + 8 * i;
                o[0] = static_cast<float>(grid[up * 12 + left]);
                o[1] = static_cast<float>(grid[r_ * 12 + left]);
                o[2] = static_cast<float>(grid[down * 12 + left]);
                o[3] = static_cast<float>(grid[up * 12 + c_]);
                o[4] = static_cast<float>(grid[down * 12 + c_]);
                o[5] = static_cast<float>(grid[up * 12 + right]);
                o[6] = static_cast<float>(grid[r_ * 12 + right]);
                o[7] = static_cast<float>(grid[down * 12 + right]);
            }
        }
        // (ArcticTransport: the lidar block right after its own columns, before the reward's LDS traffic -- placed after the
        // reward, ROCm 7.2 put register copies above an exec restore in the reward's join, tools/isa_scan.py exec_prologue)
        if constexpr (LIDAR) write_lidar<SCN, GW, OBS_ONLY, Sync>(*lid, a, lds, lane, gbase, N, ag, lane_ok, x, y, th, obs_row);
        if constexpr (!OBS_ONLY) {
            // shared reward over the two ground robots, in agent order (ArcticTransport.py:125-134)
            const float dx = x - goalx, dy = y - goaly;
            lds.ax[lane] = dx * dx + dy * dy;
            lds.ay[lane] = static_cast<float>(pix * 2 + reached);
            Sync::sync();
            if (viol) {
                reward = p.violation_reward;
                done = true;
            } else {
                reward = 0.0f;
                bool all_reached = true;
#pragma unroll
                for (int j = 2; j < 4; ++j) {
                    const int pr = static_cast<int>(lds.ay[gbase + j]);
                    const bool rj = (pr & 1) != 0;
                    if (!rj) reward = reward + p.not_reached_penalty;
                    if ((pr >> 1) != 3) reward = reward + p.dist_multiplier * lds.ax[gbase + j];
                    all_reached = all_reached && rj;
                }
                done = steps > p.max_episode_steps;
                if (!done) done = all_reached;
            }
            if (lane_ok) {
                a.st.pixel_type[eN + ag] = static_cast<uint8_t>(pix);
                a.st.reached_goal[eN + ag] = static_cast<uint8_t>(reached);
            }
        }
    } else {  // a16 MaterialTransport (MaterialTransport.py:113-189)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            RG_LATE(msg[i]);
            if (!OBS_ONLY && i < N) msg[i] = msg[i] % 4;  // MaterialTransport.py:119-120
        }
        if constexpr (TEAM) RG_LATE(tq_raw);
        if (lane_st) {
            obs_row[0] = x;
            obs_row[1] = y;
            obs_row[2] = static_cast<float>(load);
            obs_row[3] = static_cast<float>(zone0);
            obs_row[4] = static_cast<float>(zone1);
#pragma unroll
            for (int i = 0; i < 4; ++i) obs_row[5 + i] = static_cast<float>(msg[i]);
            if (RG_SHAPED(CA, RG_ARG(p.capability_aware))) {
                if constexpr (TEAM) obs_row[9] = static_cast<float>(tq_raw);
                else obs_row[9] = static_cast<float>(p.torque[ag]);
                obs_row[10] = agent_step;
            }
        }
        if constexpr (!OBS_ONLY) {
            lds.ax[lane] = x;
            lds.ay[lane] = y;
            lds.aload[lane] = load;
            if constexpr (TEAM) team_lds<SCN, GW>().torque[lane] = tq_raw;   // the replay reads every partner's
            Sync::sync();
            if (viol) {
                reward = RG_ARG(p.violation_reward);
                done = true;
            } else {
                // zone depletion is order-dependent across agents (MaterialTransport.py:161-189):
                // every lane replays the env's sequential loop from the LDS copy
                reward = RG_ARG(p.time_penalty);
                const float egw = RG_ARG(p.end_goal_width);
                const float zr2 = RG_ARG(p.zone1_radius) * RG_ARG(p.zone1_radius);
                bool any_load = false;
                for (int j = 0; j < N; ++j) {
                    const float jx = lds.ax[gbase + j], jy = lds.ay[gbase + j];
                    int jl = lds.aload[gbase + j];
                    int tq;
                    if constexpr (TEAM) tq = team_lds<SCN, GW>().torque[gbase + j];
                    else if constexpr (ARGV) tq = arg_elem(p.torque, j);
                    else tq = p.torque[j];
                    if (jl > 0) {
                        if (jx < -1.5f + egw) {
                            reward = reward + static_cast<float>(jl) * RG_ARG(p.unload_multiplier);
                            jl = 0;
                        }
                    } else {
                        if (jx > 1.5f - egw) {
                            if (zone1 > tq) {
                                jl = tq;
                                zone1 -= tq;
                            } else {
                                jl = zone1;
                                zone1 = 0;
                            }
                            reward = reward + static_cast<float>(jl) * RG_ARG(p.load_multiplier);
                        } else if (jx * jx + jy * jy <= zr2) {
                            if (zone0 > tq) {
                                jl = tq;
                                zone0 -= tq;
                            } else {
                                jl = zone0;
                                zone0 = 0;
                            }
                            reward = reward + static_cast<float>(jl) * RG_ARG(p.load_multiplier);
                        }
                    }
                    if (j == ag) load = jl;
                    any_load = any_load || (jl != 0);
                }
                done = steps > RG_ARG(p.max_episode_steps);
                if (!done) done = (zone0 == 0 && zone1 == 0 && !any_load);
            }
            int total = 0;
            {   // info['remaining'] = zone loads + agent loads (after the update)
                lds.aload[lane] = lane_ok ? load : 0;
                Sync::sync();
                for (int j = 0; j < N; ++j) total += lds.aload[gbase + j];
            }
            if (done) remaining = zone0 + zone1 + total;
            if (lane_st) RG_ARG(a.st.load)[eN + ag] = load;
            if (lane_st && ag == 0) {
                RG_ARG(a.st.zone_load)[2 * e] = zone0;
                RG_ARG(a.st.zone_load)[2 * e + 1] = zone1;
            }
            if (lane_st && ag < 4) RG_ARG(a.st.messages)[4 * e + ag] = msg[ag == 0 ? 0 : ag == 1 ? 1 : ag == 2 ? 2 : 3];
        }
    }

    // the lidar block, from the poses the own columns were built from (the staged LDS rows are still intact here)
    if constexpr (LIDAR && SCN != RG_SCN_ARCTIC_TRANSPORT) write_lidar<SCN, GW, OBS_ONLY, Sync>(*lid, a, lds, lane, gbase, N, ag, lane_ok, x, y, th, obs_row);
    RG_STAMP(4);  // scenario epilogue computed
    if constexpr (!OBS_ONLY) {
        // gym's TimeLimit on top of the scenario (gymma block of rg_step_io): the limit ends an episode the scenario did not
        constexpr bool gym = GYM;
        bool trunc = false;
        if (gym) {
            RG_LATE(el_raw);
            trunc = env_ok & !done & (el_raw + 1 >= q_tl);
        }
        const bool ended = done | trunc;
        // sum of the agents' rewards in agent order (read when shared_reward == 0, and by the gymma block)
        float rsum = 0.0f;
        if ((stats_e && !RG_ARG(p.shared_reward)) || gym) {
            Sync::sync();
            lds.ax[lane] = lane_ok ? reward : 0.0f;
            Sync::sync();
            for (int j = 0; j < N; ++j) rsum = rsum + lds.ax[gbase + j];
        }
        // ---- stores
        if (lane_st) {
            const auto X = RG_ARG(a.st.poses) + eN * 3;
            X[ag] = x;
            X[N + ag] = y;
            X[2 * N + ag] = th;
            RG_ARG(a.st.carry_dist)[eN + ag] = carry;
            out_store1(RG_OUT(reward) + eN + ag, reward);
            out_store1(RG_OUT(dist_travelled) + eN + ag, dist);
            if (ag == 0) {
                RG_ARG(a.st.episode_steps)[e] = steps;
                if (stats_e) {  // misc.py:178-185: episodeReward += reward[0] | sum(reward)
                    RG_LATE(st_ret);
                    RG_LATE(st_sum);
                    RG_LATE(st_cnt);
                    RG_LATE(st_steps);
                    float ret = st_ret + (RG_ARG(p.shared_reward) ? reward : rsum);
                    if (ended) {  // a truncated episode counts like a finished one (run_env counts them, misc.py:186-206)
                        RG_ARG(a.st.done_return_sum)[e] = st_sum + ret;
                        RG_ARG(a.st.done_count)[e] = st_cnt + 1;
                        RG_ARG(a.st.done_steps_sum)[e] = st_steps + steps;
                        ret = 0.0f;
                    }
                    RG_ARG(a.st.ep_return)[e] = ret;
                }
                RG_OUT(done)[e] = done ? 1 : 0;
                if (gym) {
                    q_el[e] = ended ? 0 : el_raw + 1;
                    sv.io.truncated[e] = trunc ? 1 : 0;
                    sv.io.ended[e] = ended ? 1 : 0;
                    sv.io.reward_sum[e] = rsum;
                }
                RG_OUT(violation)[e] = static_cast<uint8_t>(viol);
                RG_OUT(remaining)[e] = remaining;
                if (RG_OUT(qp_sweeps)) RG_OUT(qp_sweeps)[e] = max_sweeps;
            }
            if constexpr (GYM) {
                // rg_step_io.zero_obs_on_end: an env that ends hands the trainer the reset observation (zeros).  This lane wrote
                // its agent's row above (its own block and its neighbours' slots); the same lane's later stores win.
                if (sv.io.zero_obs_on_end && ended) {
                    for (int c = 0; c < D; ++c) obs_row[c] = 0.0f;
                }
            }
        }
        RG_STAMP(5);  // outputs stored
        // ---- fused auto-reset of finished envs (scenario.reset(); ~1 env in 70 per step)
        // an env whose block holds exactly the episode that starts now copies it; any other runs the sampler
        if (RG_ARG(a.auto_reset) && __any(env_ok & ended)) {
            Sync::sync();  // the wave's state stores are issued before the resetting lanes rewrite them
            if constexpr (AHEAD) load_next(env_st & ended & have_next & !next_early);  // ended some other way: fetched late
            if (__any(env_ok & ended & !have_next)) reset_group<SCN, GW, Sync>(RG_SAMPLER_ARGS, lds, e, g, ag, env_st & ended & !have_next, rc_raw, sv.seed);
            if (env_st & ended & have_next) {  // the same stores reset_group makes with commit = true
                if (ag < N) {
                    const auto X = RG_ARG(a.st.poses) + eN * 3;
                    X[ag] = nx_pose[0];
                    X[N + ag] = nx_pose[1];
                    X[2 * N + ag] = nx_pose[2];
                    RG_ARG(a.st.carry_dist)[eN + ag] = 0.0f;
                    if constexpr (SCN == RG_SCN_WAREHOUSE) RG_ARG(a.st.loaded)[eN + ag] = 0;
                    if constexpr (SCN == RG_SCN_MATERIAL_TRANSPORT) {
                        RG_ARG(a.st.load)[eN + ag] = 0;
                        if (ag < 4) RG_ARG(a.st.messages)[4 * e + ag] = 0;
                    }
                    if constexpr (SCN == RG_SCN_ARCTIC_TRANSPORT) {
                        a.st.pixel_type[eN + ag] = 0;
                        a.st.reached_goal[eN + ag] = 0;
                    }
                }
                if constexpr (SCN == RG_SCN_PREDATOR_CAPTURE_PREY || SCN == RG_SCN_SIMPLE) {
                    const int P = RG_SHAPED(P, RG_ARG_OR(p.num_prey, q_P));
                    const auto nb = RG_ARG_OR(a.st.next_init, q_nin) + static_cast<size_t>(e) * RG_ARG_OR(a.next_stride, q_nst) + 3 * N;
                    for (int i = ag; i < P; i += GW) {  // prey `ag` was prefetched; more than GW prey: the rest from the block
                        const auto pl = RG_ARG(a.st.prey_loc) + (static_cast<size_t>(e) * P + i) * 2;
                        pl[0] = i == ag ? nx_a : nb[2 * i];
                        pl[1] = i == ag ? nx_b : nb[2 * i + 1];
                        if constexpr (SCN == RG_SCN_PREDATOR_CAPTURE_PREY) {
                            RG_ARG(a.st.prey_sensed)[static_cast<size_t>(e) * P + i] = 0;
                            RG_ARG(a.st.prey_captured)[static_cast<size_t>(e) * P + i] = 0;
                        }
                    }
                } else if constexpr (SCN == RG_SCN_MATERIAL_TRANSPORT) {
                    if (ag < 2) RG_ARG(a.st.zone_load)[2 * e + ag] = __builtin_bit_cast(int32_t, nx_a);
                } else if constexpr (SCN == RG_SCN_ARCTIC_TRANSPORT) {
                    uint32_t *gd = reinterpret_cast<uint32_t *>(a.st.grid + static_cast<size_t>(e) * 96);
#pragma unroll
                    for (int t = 0; t < 6; ++t) gd[ag * 6 + t] = nx_grid[t];
                    if (ag == 0) a.st.goal_col[e] = static_cast<int32_t>(nx_grid[6]);
                }
                if (ag == 0) {
                    RG_ARG(a.st.reset_count)[e] = rc_raw + 1;
                    RG_ARG(a.st.episode_steps)[e] = 0;
                }
            }
            // the new episode's team: the episode just started is episode rc_raw on either path above (the drawn-ahead block is
            // tagged with it), and the index is a function of that episode alone -- nothing of it is drawn ahead
            if constexpr (TEAM) {
                if (env_ok & ended & (ag == 0)) q_tidx[e] = team_draw(*tm, static_cast<uint64_t>(a.env_offset + e), rc_raw, a.seed);
            }
        }
        // ---- draw ahead: an env that goes on and whose block does not hold its next episode (consumed by the reset of
        // an earlier launch, or never drawn) gets it now.  The block of an env that finished in THIS launch is left
        // stale on purpose (it is redrawn in a later launch, off this launch's critical path).
        // A wavefront that is already long -- a QP of one of its envs needed more than two sweeps, or a chunk was
        // replayed -- leaves the draw to a later launch (an env that finishes before it happened runs the sampler as
        // before): the draw must not lengthen the waves the launch is waiting for.
        // (PM: "not a long wavefront" is the same in every lane and goes into the vote: one branch less on the common path)
        if (PM ? AHEAD && ahead_e && __any(!(replayed | __any(max_sweeps > 2)) & env_ok & !ended & !have_next)
               : AHEAD && ahead_e && !(replayed | __any(max_sweeps > 2)) && __any(env_ok & !ended & !have_next)) {
            const bool need = env_st & !ended & !have_next;
            Sync::sync();  // (LDS scratch of a reset above is free again)
            reset_group<SCN, GW, Sync>(RG_SAMPLER_ARGS, lds, e, g, ag, need, rc_raw, reset_dst_next(RG_SAMPLER_ARGS, e), sv.seed);
            if (need && ag == 0) RG_ARG(a.st.next_episode)[e] = rc_raw;
        }
        RG_STAMP(6);  // reset done
        RG_STAMPS_WRITE(lane, sv.io.qp_sweeps, chunk * EPW, a.E, max_sweeps)
    }
}

#undef RG_ARG
#undef RG_ARG_BLOCK_OFF
#undef RG_IMG
#undef RG_SAMPLER_ARGS
#undef RG_ARG_OFF
#undef RG_ARG_OR
#undef RG_OUT
#undef RG_SHAPED

// ------------------------------------------------------------------ the step kernels: four families, one body
// The step comes in four families of kernels: plain; with the lidar on (rg_set_lidar: the range block of lidar.h written at the
// end of the observation phase); with a team pool (rg_set_teams: the agents' capabilities from set team_index[e] of team.h, and
// the index of every episode the step starts); with the pose disturbance (rg_set_disturbance: the poses displaced by the draw of
// disturb.h before the step reads them).  None of the last three has a thread-per-env form: such a handle always runs
// these.  A family is described by its argument block (the step's own KernelArgs, and the side block next to it that the other
// kernels never see), by what it hands step_once, and by whether a rollout re-addresses the block every step.
struct PlainFamily {
    using Args = KernelArgs;
    static constexpr bool LIDAR = false, TEAM = false, NOISE = false, READDRESS = false;
    static Args args(const KernelArgs &a, const GroupSide &) { return a; }
    __device__ __forceinline__ static const KernelArgs &kernel_args(const Args &x) { return x; }
    __device__ __forceinline__ static const rg_lidar_params *lidar(const Args &) { return nullptr; }
    __device__ __forceinline__ static const rg_team_params *teams(const Args &) { return nullptr; }
    __device__ __forceinline__ static const DisturbScale *disturb(const Args &) { return nullptr; }
};
struct LidarFamily {
    using Args = LidarArgs;
    static constexpr bool LIDAR = true, TEAM = false, NOISE = false, READDRESS = true;
    static Args args(const KernelArgs &a, const GroupSide &side) { return Args{a, *side.lidar}; }
    __device__ __forceinline__ static const KernelArgs &kernel_args(const Args &x) { return x.k; }
    __device__ __forceinline__ static const rg_lidar_params *lidar(const Args &x) { return &x.lid; }
    __device__ __forceinline__ static const rg_team_params *teams(const Args &) { return nullptr; }
    __device__ __forceinline__ static const DisturbScale *disturb(const Args &) { return nullptr; }
};
struct TeamFamily {
    using Args = TeamArgs;
    static constexpr bool LIDAR = false, TEAM = true, NOISE = false, READDRESS = true;
    static Args args(const KernelArgs &a, const GroupSide &side) { return Args{a, *side.teams}; }
    __device__ __forceinline__ static const KernelArgs &kernel_args(const Args &x) { return x.k; }
    __device__ __forceinline__ static const rg_lidar_params *lidar(const Args &) { return nullptr; }
    __device__ __forceinline__ static const rg_team_params *teams(const Args &x) { return &x.tp; }
    __device__ __forceinline__ static const DisturbScale *disturb(const Args &) { return nullptr; }
};
struct DisturbFamily {
    using Args = DisturbArgs;
    static constexpr bool LIDAR = false, TEAM = false, NOISE = true, READDRESS = true;
    static Args args(const KernelArgs &a, const GroupSide &side) { return Args{a, *side.disturb}; }
    __device__ __forceinline__ static const KernelArgs &kernel_args(const Args &x) { return x.k; }
    __device__ __forceinline__ static const rg_lidar_params *lidar(const Args &) { return nullptr; }
    __device__ __forceinline__ static const rg_team_params *teams(const Args &) { return nullptr; }
    __device__ __forceinline__ static const DisturbScale *disturb(const Args &x) { return &x.ds; }
};

// The argument block of a rollout's next step.  READDRESS: through an opaque copy of the kernel-argument segment's address
// (device_common.h kernarg_block).  Left loop-invariant, the compiler hoists the block's loads out of the step loop and holds
// them across the whole step -- the lidar rollout of PredatorCapturePrey GW 4: 273 VGPRs + 17 AGPRs and 148 bytes of scratch,
// against 169 and none.  The plain rollout keeps the block it was given (its code predates the finding and is left as it is).
template <class F>
__device__ __forceinline__ const typename F::Args &rollout_step_args(const typename F::Args &args) {
    if constexpr (F::READDRESS) return *(const typename F::Args *)kernarg_block<typename F::Args>();
    else return args;
}

// ROLLOUT = false: one env step per launch (rg_step, rg_get_obs).  ROLLOUT = true (rg_rollout): the
// wave's envs advance num_steps times with no device-wide synchronisation between steps; state
// round-trips through this CU's caches (workgroup-scope visibility after the barrier).  Separate
// instantiations: the loop keeps more values live (at N = 5 the thread-per-env kernel goes from 237 to
// 313 VGPRs) and would slow the single-step launch down.
// QPM = RG_QP_CVXOPT: the certificate's QP by the interior-point iteration of ipm_qp.h.  Its own instantiations (generic agent
// count): the launch is then dominated by that iteration (about ten times the rest of the step), and it needs one wave per SIMD.
// SPAN: one env per 16-lane row (step_once).
template <class F, int SCN, int GW, bool OBS_ONLY, int NT, bool ROLLOUT, bool GYM, int QPM, bool SPAN = false>
__device__ __forceinline__ void step_kernel_body(const typename F::Args &args) {
    constexpr bool IPM = QPM == RG_QP_CVXOPT;
    static_assert(!IPM || GW == 4 || GW == 8, "the interior-point mode admits n_agents <= 8");
    static_assert(!IPM || !OBS_ONLY, "an observation-only launch runs no controller");
    static_assert(!SPAN || (!ROLLOUT && !OBS_ONLY), "the 16-lane rows: the single-step launch");
    __shared__ Lds<GW> lds;
    using Q = std::conditional_t<IPM, ipm::GroupLds<GW>, void>;
    Q *qp_lds = nullptr;
    if constexpr (IPM) {
        __shared__ Q qp_block;   // records + one workspace per env (ipm_qp.h): these instantiations only
        qp_lds = &qp_block;
    }
    const KernelArgs &a = F::kernel_args(args);
    const int N = NT > 0 ? NT : a.p.n_agents;
    if constexpr (!ROLLOUT) {
        step_once<SCN, GW, OBS_ONLY, NT, true, GYM, QPM, Q, WgSync, F::LIDAR, F::TEAM, SPAN, F::NOISE>(a, lds, step_view(a, 0, N, a.p.obs_dim), qp_lds,
                                                                                                     F::lidar(args), F::teams(args), F::disturb(args));
    } else {
        for (int t = 0; t < a.num_steps; ++t) {
            if (t) __syncthreads();
            const typename F::Args &now = rollout_step_args<F>(args);
            const KernelArgs &at = F::kernel_args(now);
            step_once<SCN, GW, OBS_ONLY, NT, false, false, QPM, Q, WgSync, F::LIDAR, F::TEAM, false, F::NOISE>(at, lds, step_view(at, t, N, at.p.obs_dim), qp_lds,
                                                                                                            F::lidar(now), F::teams(now), F::disturb(now));
        }
    }
}

// The __global__ templates: one per family.  Their names, template parameter lists and argument types are an interface (the
// mangled names are matched by bench.py, the resource tests and the profile tools).
template <int SCN, int GW, bool OBS_ONLY, int NT, bool ROLLOUT, bool GYM = false, int QPM = 0>
__global__ __launch_bounds__(WAVE) void step_kernel(const KernelArgs a) {
    step_kernel_body<PlainFamily, SCN, GW, OBS_ONLY, NT, ROLLOUT, GYM, QPM>(a);
}
// ROW = 16: one env per 16-lane row (step_once SPAN), 4 envs per wave; the single-step exact-mode launch with GW = 8 only
// (step_kernel<SCN, 8, false, NT, false, 16>).  A template of its own, so that every existing instantiation keeps its name.
template <int SCN, int GW, bool OBS_ONLY, int NT, bool ROLLOUT, int ROW, std::enable_if_t<ROW == 16, int> = 0>
__global__ __launch_bounds__(WAVE) void step_kernel(const KernelArgs a) {
    step_kernel_body<PlainFamily, SCN, GW, OBS_ONLY, NT, ROLLOUT, false, 0, true>(a);
}
#ifndef RG_HOST_SIM
// RESIDENT: the row kernel again, taking the handle's resident image and the per-call arguments (kernel_args.h ResidentCall: the
// parameters below are its members in its order).  The image is never written once a launch may read it -- a change takes a fresh
// slot (robogym_capi.hip) -- so it is read through the CONSTANT address space: the compiler keeps scalar loads for its uniform
// members, as it does for kernel arguments.  Instantiated in robogym_resident.hip alone, whose flags hand the leading
// parameters over in scalar registers.  (A further overload: the by-value row kernels keep their names.)
template <int SCN, int GW, bool OBS_ONLY, int NT, bool ROLLOUT, int ROW, bool RESIDENT, std::enable_if_t<ROW == 16 && RESIDENT, int> = 0>
__global__ __launch_bounds__(WAVE) void step_kernel(const KernelArgs *image, const int32_t *actions, const uint64_t seed, const int32_t auto_reset,
                                                    const int32_t grid, const rg_step_io io) {
    static_assert(GW == 8 && !OBS_ONLY && !ROLLOUT, "the 16-lane rows: the single-step launch at GW 8");
    typedef const __attribute__((address_space(4))) KernelArgs *ConstImage;
    ConstImage ci = (ConstImage)image;
    asm volatile("" : "+s"(ci));   // (opaque, as in kernarg_block: seen through, the cast folds away and the loads are global ones)
    const KernelArgs &a = *(const KernelArgs *)ci;
    __shared__ Lds<GW> lds;
    const StepView sv = {actions, io, &auto_reset, &seed, grid};
    step_once<SCN, GW, false, NT, true, false, 0, void, WgSync, false, false, true, false, true>(a, lds, sv);
}
// ... and the resident kernel of a reference shape (kernel_args.h RG_REF_SHAPES): SH's fields are constants of the body.  The same
// parameters, image and flags; instantiated in robogym_resident_shapes.hip alone.  (One more overload: every kernel above keeps
// its name, and these share the leading template arguments that the profile tools match the headline kernel by.)
template <int SCN, int GW, bool OBS_ONLY, int NT, bool ROLLOUT, int ROW, bool RESIDENT, class SH, std::enable_if_t<ROW == 16 && RESIDENT, int> = 0>
__global__ __launch_bounds__(WAVE) void step_kernel(const KernelArgs *image, const int32_t *actions, const uint64_t seed, const int32_t auto_reset,
                                                    const int32_t grid, const rg_step_io io) {
    static_assert(GW == 8 && !OBS_ONLY && !ROLLOUT, "the 16-lane rows: the single-step launch at GW 8");
    typedef const __attribute__((address_space(4))) KernelArgs *ConstImage;
    ConstImage ci = (ConstImage)image;
    asm volatile("" : "+s"(ci));
    const KernelArgs &a = *(const KernelArgs *)ci;
    __shared__ Lds<GW> lds;
    const StepView sv = {actions, io, &auto_reset, &seed, grid};
    step_once<SCN, GW, false, NT, true, false, 0, void, WgSync, false, false, true, false, true, SH>(a, lds, sv);
}
#endif
// generic agent count (NT = 0) throughout
template <int SCN, int GW, bool OBS_ONLY, bool ROLLOUT, bool GYM, int QPM>
__global__ __launch_bounds__(WAVE) void lidar_step_kernel(const LidarArgs la) {
    step_kernel_body<LidarFamily, SCN, GW, OBS_ONLY, 0, ROLLOUT, GYM, QPM>(la);
}
template <int SCN, int GW, bool OBS_ONLY, int NT, bool ROLLOUT, bool GYM, int QPM>
__global__ __launch_bounds__(WAVE) void team_step_kernel(const TeamArgs ta) {
    step_kernel_body<TeamFamily, SCN, GW, OBS_ONLY, NT, ROLLOUT, GYM, QPM>(ta);
}

// generic agent count (NT = 0) throughout; no observation-only form (rg_get_obs displaces nothing: the plain kernel)
template <int SCN, int GW, bool ROLLOUT, bool GYM, int QPM>
__global__ __launch_bounds__(WAVE) void disturb_step_kernel(const DisturbArgs da) {
    step_kernel_body<DisturbFamily, SCN, GW, false, 0, ROLLOUT, GYM, QPM>(da);
}

template <int SCN, int GW>
__global__ __launch_bounds__(WAVE) void reset_kernel(const KernelArgs a) {
    constexpr int EPW = WAVE / GW;
    __shared__ Lds<GW> lds;
    const int lane = threadIdx.x;
    const int ag = lane & (GW - 1);
    const int g = lane / GW;
    const int e = blockIdx.x * EPW + g;
    const bool env_ok = e < a.E;
    const bool want = env_ok && (a.reset_mask == nullptr || a.reset_mask[e] != 0);
    if (!__any(want)) return;
    // the running return restarts with the episode; RG_RESET_BOOK_EPISODE first books the abandoned
    // episode as finished (an episode cut short by a time limit outside the scenario)
    const bool stats = want && ag == 0 && a.st.ep_return != nullptr;
    const int steps_before = stats ? a.st.episode_steps[e] : 0;
    reset_group<SCN, GW>(a, lds, e, g, ag, want);
    if (stats) {
        if ((a.reset_flags & RG_RESET_BOOK_EPISODE) && steps_before > 0) {
            a.st.done_return_sum[e] = a.st.done_return_sum[e] + a.st.ep_return[e];
            a.st.done_count[e] = a.st.done_count[e] + 1;
            a.st.done_steps_sum[e] = a.st.done_steps_sum[e] + steps_before;
        }
        a.st.ep_return[e] = 0.0f;
    }
}

}  // namespace rg


// ------------------------------------------------------------------ host side: launch dispatch
// A switch from the values of the launch's plan (launch_plan.h: the one place that decides) to template arguments.  Nothing is
// derived here; the `if constexpr` guards only keep instantiations that no plan names out of the build.
namespace rg {

// one launch of family F's __global__ template (ROWS: the plain family's 16-lane-row overload)
template <class F, int SCN, int GW, bool OBS_ONLY, int NT, bool ROLLOUT, bool GYM, int QPM, bool ROWS = false>
static void launch_kernel(const typename F::Args &args, int grid, hipStream_t stream) {
    if constexpr (ROWS) hipLaunchKernelGGL((step_kernel<SCN, GW, OBS_ONLY, NT, ROLLOUT, 16>), dim3(grid), dim3(WAVE), 0, stream, args);
    else if constexpr (F::LIDAR) hipLaunchKernelGGL((lidar_step_kernel<SCN, GW, OBS_ONLY, ROLLOUT, GYM, QPM>), dim3(grid), dim3(WAVE), 0, stream, args);
    else if constexpr (F::TEAM) hipLaunchKernelGGL((team_step_kernel<SCN, GW, OBS_ONLY, NT, ROLLOUT, GYM, QPM>), dim3(grid), dim3(WAVE), 0, stream, args);
    else if constexpr (F::NOISE) hipLaunchKernelGGL((disturb_step_kernel<SCN, GW, ROLLOUT, GYM, QPM>), dim3(grid), dim3(WAVE), 0, stream, args);
    else hipLaunchKernelGGL((step_kernel<SCN, GW, OBS_ONLY, NT, ROLLOUT, GYM, QPM>), dim3(grid), dim3(WAVE), 0, stream, args);
}

// The kernel of (family, scenario, launch kind, mode) at pl.gw, pl.nt and pl.rows.  (The resident forms of a row kernel are
// entries of their own, robogym_resident*.hip: the plan's kind selects them.)
template <class F, int SCN, bool OBS_ONLY, bool ROLLOUT, bool GYM, int QPM>
static hipError_t launch_gw(const typename F::Args &args, const LaunchPlan &pl, hipStream_t stream) {
    constexpr bool EXACT = QPM == RG_QP_EXACT;
    constexpr bool BY_N = EXACT && !OBS_ONLY && !GYM && !F::LIDAR && !F::NOISE;
    constexpr bool ROWS = BY_N && !ROLLOUT && !F::TEAM && !kStampsBuild;
    if (pl.gw == 4) {
        launch_kernel<F, SCN, 4, OBS_ONLY, 0, ROLLOUT, GYM, QPM>(args, pl.grid, stream);
    } else if constexpr (SCN == RG_SCN_ARCTIC_TRANSPORT) {
        return hipErrorInvalidValue;   // (rg_create admits exactly 4 agents)
    } else if (pl.gw == 16) {
        if constexpr (EXACT) launch_kernel<F, SCN, 16, OBS_ONLY, 0, ROLLOUT, GYM, QPM>(args, pl.grid, stream);
        else return hipErrorInvalidValue;   // (rg_create admits n_agents <= 8 in the interior-point mode)
    } else if constexpr (BY_N) {
        auto by_n = [&](auto rows_c) {
            constexpr bool R = decltype(rows_c)::value;
            switch (pl.nt) {
                case 5: launch_kernel<F, SCN, 8, false, 5, ROLLOUT, false, QPM, R>(args, pl.grid, stream); break;
                case 6: launch_kernel<F, SCN, 8, false, 6, ROLLOUT, false, QPM, R>(args, pl.grid, stream); break;
                case 7: launch_kernel<F, SCN, 8, false, 7, ROLLOUT, false, QPM, R>(args, pl.grid, stream); break;
                default: launch_kernel<F, SCN, 8, false, 8, ROLLOUT, false, QPM, R>(args, pl.grid, stream); break;
            }
        };
        if (ROWS && pl.rows) by_n(std::integral_constant<bool, ROWS>());
        else by_n(std::false_type());
    } else {
        launch_kernel<F, SCN, 8, OBS_ONLY, 0, ROLLOUT, GYM, QPM>(args, pl.grid, stream);
    }
    return hipGetLastError();
}

// The lane-group launch of family F: every translation unit's entry is one instantiation of this (OBS_ONLY exists for the single
// launch of the exact mode only: an observation runs no controller).  `a` as the caller filled it, envs_per_wave from the plan.
template <class F, bool OBS_ONLY, bool ROLLOUT, int QPM>
static hipError_t launch_group(const KernelArgs &a, const GroupSide &side, hipStream_t stream) {
    static_assert(!OBS_ONLY || (!ROLLOUT && QPM == RG_QP_EXACT), "rg_get_obs is a single launch of the exact mode's kernel");
    static_assert(!OBS_ONLY || !F::NOISE, "rg_get_obs of a disturbed handle is the plain family's launch");
    return for_scenario(a.p.scenario, [&](auto scn) -> hipError_t {
        constexpr int SCN = decltype(scn)::value;
        if constexpr (SCN == RG_SCN_ARCTIC_TRANSPORT && F::TEAM) {
            return hipErrorInvalidValue;   // refused by rg_set_teams: the scenario fixes its agent types
        } else {
            const typename F::Args args = F::args(a, side);
            if constexpr (!OBS_ONLY && !ROLLOUT) {
                if (side.plan.gym) return launch_gw<F, SCN, false, false, true, QPM>(args, side.plan, stream);   // gymma block: its own instantiations
            }
            return launch_gw<F, SCN, OBS_ONLY, ROLLOUT, false, QPM>(args, side.plan, stream);
        }
    });
}

}  // namespace rg
