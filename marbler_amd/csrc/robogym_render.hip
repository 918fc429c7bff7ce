// robogym_render.hip -- rg_render: K RGB frames of K envs' state in one launch (include/robogym.h; the picture: render.h).
//
// The output is the traffic: K * H * W * 3 bytes, written once.  A lane owns quads of 4 horizontally adjacent pixels and stores
// a quad's 12 bytes as three dwords with one vector store (width % 4 == 0 keeps it dword-aligned); the lanes of a wave hold
// consecutive quads of a frame, so a wave's store covers 768 contiguous bytes.  A work-group of 256 lanes covers a tile of 1024
// consecutive quads of ONE frame (lane t owns quads t, t + 256, t + 512, t + 768 of the tile): it first stages that env's
// shape list in LDS -- the robots with the sine and cosine of their heading, the prey with their colour, the terrain bytes, the
// palette -- and every lane then tests its pixel centres against the staged list.  What does not depend on the env (the view,
// the arena, the fixed zone rectangles, the classes' colours and ring radii) arrives by value and stays in scalar registers.
//
// Culling is by wave: a wave's 64 quads lie in three or four image rows at 84 x 84, a robot covers five, a prey two.  Each wave
// holds the shape list in registers, a shape per lane; per 64 quads the lanes test THEIR shape against the wave's rows, a ballot
// turns that into a mask, and only the shapes in the mask are drawn, in index order, their fields fetched by lane reads into
// scalar registers.  The row test only leaves out shapes none of whose pixel tests can pass: it allows CULL_MARGIN (1 mm) more
// than the shape's extent, where the roundings of the pixel test amount to an ulp of a coordinate (1.5e-5 m at the 200 m the
// arena's domain ends at).  (The first form of the kernel tested every pixel against every shape and spent ~1000 instructions
// per quad: 8 x the time of writing the output.)
//
// The host entry is handle-free and keeps its own last-error text (as actor_mfma.hip does): every argument check comes before
// the first HIP call, so the refusals can be exercised without a device.
#include <hip/hip_runtime.h>

#include <cmath>

#include "host_checks.h"
#include "render.h"
#include "sim_math.h"

namespace rg {
namespace render {

#ifndef RG_RENDER_HOST_ONLY   // (the sanitized host build, build.py build_host_sanitized: the argument checks without the kernel)
struct Staged {
    float rx[RG_MAX_AGENTS], ry[RG_MAX_AGENTS], rs[RG_MAX_AGENTS], rc[RG_MAX_AGENTS];
    float qx[RG_MAX_PREY], qy[RG_MAX_PREY];
    uint8_t qcol[RG_MAX_PREY];     // 0: not drawn
    uint8_t grid[RG_ARCTIC_ROWS * RG_ARCTIC_COLS];
    uint32_t palette[16];          // 0x00BBGGRR
};

__constant__ uint8_t PALETTE_RGB[COL_COUNT][3] = {RG_RENDER_PALETTE};

struct Quad {
    uint32_t a, b, c;
};

#define RG_RENDER_EACH(p) for (int p = 0; p < 4; ++p)

// lane `lane`'s value of v, for a wave-uniform lane index: a scalar
__device__ __forceinline__ float lane_value(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ uint32_t lane_value(uint32_t v, int lane) {
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), lane));
}
// the image row of quad q: q / quads_per_row by one multiplication.  (q + 0.5) / quads_per_row lies at least 0.5 / 256 from an
// integer, the product's rounding error stays below 1024 * 4e-7.
__device__ __forceinline__ int row_of(int q, float inv_quads_per_row) {
    return static_cast<int>((static_cast<float>(q) + 0.5f) * inv_quads_per_row);
}
// can a shape centred at height y, reaching `reach` up and down, touch the rows [y_lo, y_hi]?  False for a NaN.
__device__ __forceinline__ bool near_rows(float y, float reach, float y_lo, float y_hi) {
    return y - y_hi <= reach && y_lo - y <= reach;
}

__global__ __launch_bounds__(BLOCK) void render_kernel(const Args a) {
    __shared__ Staged s;
    const int tid = static_cast<int>(threadIdx.x);
    const int frame = static_cast<int>(blockIdx.x) / a.tiles;
    const int tile = static_cast<int>(blockIdx.x) - frame * a.tiles;
    const int env = a.env_index ? a.env_index[frame] : frame;
    const bool live = env >= 0 && env < a.num_envs;
    const float nan = __builtin_nanf("");

    // ---- stage the env's shape list
    if (tid < RG_MAX_AGENTS) {
        float x = nan, y = nan, sn = nan, cs = nan;
        if (live && tid < a.n_agents) {
            const float *p = a.poses + static_cast<size_t>(env) * 3 * a.n_agents;
            x = p[tid];
            y = p[a.n_agents + tid];
            const float th = p[2 * a.n_agents + tid];
            if (__builtin_fabsf(th) <= MAX_HEADING_ANGLE) sincos_spec(th, sn, cs);
        }
        s.rx[tid] = x;
        s.ry[tid] = y;
        s.rs[tid] = sn;
        s.rc[tid] = cs;
    } else if (tid >= 64 && tid < 64 + RG_MAX_PREY) {
        const int j = tid - 64;
        float x = nan, y = nan;
        uint8_t col = 0;
        if (live && a.prey_loc && j < a.num_prey) {
            const size_t at = static_cast<size_t>(env) * a.num_prey + j;
            x = a.prey_loc[2 * at];
            y = a.prey_loc[2 * at + 1];
            if (a.prey_captured[at] == 0) col = a.prey_sensed[at] != 0 ? COL_PREY_SENSED : COL_PREY;
        }
        s.qx[j] = x;
        s.qy[j] = y;
        s.qcol[j] = col;
    } else if (tid >= 128 && tid < 128 + RG_ARCTIC_ROWS * RG_ARCTIC_COLS) {
        const int j = tid - 128;
        s.grid[j] = (live && a.arctic) ? a.grid[static_cast<size_t>(env) * (RG_ARCTIC_ROWS * RG_ARCTIC_COLS) + j] : 0;
    } else if (tid >= 224 && tid < 240) {
        const int j = tid - 224 < COL_COUNT ? tid - 224 : 0;
        s.palette[tid - 224] = static_cast<uint32_t>(PALETTE_RGB[j][0]) | static_cast<uint32_t>(PALETTE_RGB[j][1]) << 8 |
                               static_cast<uint32_t>(PALETTE_RGB[j][2]) << 16;
    }
    __syncthreads();

    // ---- every wave keeps the list in registers, a shape per lane: robot (lane & 15) and prey (lane).  A shape that the wave's
    // rows can reach is then fetched with a lane read into scalar registers -- no LDS round trip, no per-lane copy of it.
    const int lane = tid & 63;
    const int layers = a.layers;
    const float px = a.px, rr = a.robot_r;
    const float my_rx = s.rx[lane & 15], my_ry = s.ry[lane & 15], my_rs = s.rs[lane & 15], my_rc = s.rc[lane & 15];
    const float my_ring = a.ring_r[lane & 15];
    const uint32_t my_cls = a.cls_colour[lane & 15];
    const float my_qx = s.qx[lane], my_qy = s.qy[lane];
    const uint32_t my_qcol = s.qcol[lane];
    const bool is_robot = lane < a.n_agents;
    const bool is_prey = (layers & RG_RENDER_MARKERS) && lane < a.num_prey && my_qcol != 0;
    const bool is_ring = (layers & RG_RENDER_RINGS) && is_robot && my_ring > 0.0f;
    const bool is_disk = (layers & RG_RENDER_ROBOTS) && is_robot, is_heading = (layers & RG_RENDER_HEADING) && is_robot;
    // how far above and below its centre a shape can cover a pixel, plus CULL_MARGIN; the heading segment's own extent
    const float reach_disk = rr + CULL_MARGIN, reach_prey = PREY_RADIUS + CULL_MARGIN;
    const float reach_heading = (__builtin_fabsf(rr * my_rs) + __builtin_fabsf(px * my_rc)) + CULL_MARGIN;
    const float reach_ring = (my_ring + px) + CULL_MARGIN, reach_zone1 = (a.zone1_r + px) + CULL_MARGIN;
    // an outline's two rims, squared
    const float my_ring_in = my_ring - px > 0.0f ? my_ring - px : 0.0f, my_ring_out = my_ring + px;
    const float my_ring_in2 = my_ring_in * my_ring_in, my_ring_out2 = my_ring_out * my_ring_out;
    const float zone1_in = a.zone1_r - px > 0.0f ? a.zone1_r - px : 0.0f, zone1_out = a.zone1_r + px;
    // is the surround out of sight?  (the columns are the same in every row)
    const bool arena_spans_x = a.x0 + 0.5f * a.sx >= a.ax0 && a.x0 + (static_cast<float>(a.width - 1) + 0.5f) * a.sx <= a.ax1;

    for (int it = 0; it < QUADS_PER_LANE; ++it) {
        // the wave's 64 quads, and the image rows they lie in
        const int q0 = __builtin_amdgcn_readfirstlane((tile * QUADS_PER_LANE + it) * BLOCK + (tid - lane));
        if (q0 >= a.quads) break;
        const int q_last = q0 + 63 < a.quads ? q0 + 63 : a.quads - 1;
        const float y_hi = a.y_top - (static_cast<float>(row_of(q0, a.inv_quads_per_row)) + 0.5f) * a.sy;
        const float y_lo = a.y_top - (static_cast<float>(row_of(q_last, a.inv_quads_per_row)) + 0.5f) * a.sy;
        const int q = q0 + lane;                 // (past the frame's end in the last wave: computed, not stored)
        const int row = row_of(q, a.inv_quads_per_row);
        const int col = (q - row * a.quads_per_row) * 4;
        const float wy = a.y_top - (static_cast<float>(row) + 0.5f) * a.sy;
        float wx[4];
        uint32_t c[4];
        RG_RENDER_EACH(p) {
            wx[p] = a.x0 + (static_cast<float>(col + p) + 0.5f) * a.sx;
            c[p] = COL_BACKGROUND;
        }
        // 1 arena
        if ((layers & RG_RENDER_ARENA) && !(arena_spans_x && y_lo >= a.ay0 && y_hi <= a.ay1)) {
            const bool in_y = wy >= a.ay0 && wy <= a.ay1;
            RG_RENDER_EACH(p) if (!(in_y && wx[p] >= a.ax0 && wx[p] <= a.ax1)) c[p] = COL_SURROUND;
        }
        // 2 zones
        if (layers & RG_RENDER_ZONES) {
#pragma unroll
            for (int r = 0; r < MAX_RECTS; ++r) {
                if (r < a.n_rects && y_hi >= a.rect[r][2] && y_lo <= a.rect[r][3]) {
                    const bool in_y = wy >= a.rect[r][2] && wy <= a.rect[r][3];
                    RG_RENDER_EACH(p) if (in_y && wx[p] >= a.rect[r][0] && wx[p] <= a.rect[r][1]) c[p] = a.rect_colour[r];
                }
            }
            if (a.arctic) {
                const float v = (1.0f - wy) * 4.0f;
                if (v >= 0.0f && v < static_cast<float>(RG_ARCTIC_ROWS)) {
                    const int gi = static_cast<int>(v) * RG_ARCTIC_COLS;
                    RG_RENDER_EACH(p) {
                        const float u = (wx[p] + 1.5f) * 4.0f;
                        if (u >= 0.0f && u < static_cast<float>(RG_ARCTIC_COLS)) {
                            const int t = s.grid[gi + static_cast<int>(u)];
                            if (t > 0) c[p] = t == 1 ? COL_ICE : t == 2 ? COL_WATER : COL_GOAL;
                        }
                    }
                }
            }
        }
        // 3 markers
        for (uint64_t m = __ballot(is_prey && near_rows(my_qy, reach_prey, y_lo, y_hi)); m; m &= m - 1) {
            const int j = __builtin_ctzll(m);
            const float x = lane_value(my_qx, j), dy = wy - lane_value(my_qy, j);
            const uint32_t pc = lane_value(my_qcol, j);
            RG_RENDER_EACH(p) {
                const float dx = wx[p] - x;
                if (dx * dx + dy * dy <= PREY_RADIUS * PREY_RADIUS) c[p] = pc;
            }
        }
        if ((layers & RG_RENDER_MARKERS) && a.zone1 && near_rows(0.0f, reach_zone1, y_lo, y_hi)) {
            RG_RENDER_EACH(p) {
                const float d2 = wx[p] * wx[p] + wy * wy;
                if (d2 >= zone1_in * zone1_in && d2 <= zone1_out * zone1_out) c[p] = COL_ZONE1;
            }
        }
        // 4 capability rings
        for (uint64_t m = __ballot(is_ring && near_rows(my_ry, reach_ring, y_lo, y_hi)); m; m &= m - 1) {
            const int r = __builtin_ctzll(m);
            const float x = lane_value(my_rx, r), dy = wy - lane_value(my_ry, r);
            const float in2 = lane_value(my_ring_in2, r), out2 = lane_value(my_ring_out2, r);
            const uint32_t rc = lane_value(my_cls, r);
            RG_RENDER_EACH(p) {
                const float dx = wx[p] - x;
                const float d2 = dx * dx + dy * dy;
                if (d2 >= in2 && d2 <= out2) c[p] = rc;
            }
        }
        // 5 robots
        for (uint64_t m = __ballot(is_disk && near_rows(my_ry, reach_disk, y_lo, y_hi)); m; m &= m - 1) {
            const int r = __builtin_ctzll(m);
            const float x = lane_value(my_rx, r), dy = wy - lane_value(my_ry, r);
            const uint32_t rc = lane_value(my_cls, r);
            RG_RENDER_EACH(p) {
                const float dx = wx[p] - x;
                if (dx * dx + dy * dy <= rr * rr) c[p] = rc;
            }
        }
        // 6 headings
        for (uint64_t m = __ballot(is_heading && near_rows(my_ry, reach_heading, y_lo, y_hi)); m; m &= m - 1) {
            const int r = __builtin_ctzll(m);
            const float x = lane_value(my_rx, r), dy = wy - lane_value(my_ry, r);
            const float sn = lane_value(my_rs, r), cs = lane_value(my_rc, r);
            RG_RENDER_EACH(p) {
                const float dx = wx[p] - x;
                const float along = dx * cs + dy * sn;
                const float across = dy * cs - dx * sn;
                if (along >= 0.0f && along <= rr && __builtin_fabsf(across) <= px) c[p] = COL_HEADING;
            }
        }
        if (q < a.quads) {
            // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
            const uint32_t p0 = s.palette[c[0]], p1 = s.palette[c[1]], p2 = s.palette[c[2]], p3 = s.palette[c[3]];
            Quad out;
            out.a = p0 | p1 << 24;
            out.b = p1 >> 8 | p2 << 16;
            out.c = p2 >> 16 | p3 << 8;
            const size_t at = (static_cast<size_t>(frame) * a.quads + q) * 12;
            *reinterpret_cast<Quad *>(a.rgb + at) = out;
        }
    }
}

static bool launch(const Args &a, uint32_t blocks, void *hip_stream) {
    hipLaunchKernelGGL(render_kernel, dim3(blocks), dim3(BLOCK), 0, static_cast<hipStream_t>(hip_stream), a);
    return hipGetLastError() == hipSuccess;
}
#else
static bool launch(const Args &, uint32_t, void *) { return false; }
#endif

}  // namespace render
}  // namespace rg

static thread_local char g_render_err[256] = "";

extern "C" const char *rg_render_last_error(void) { return g_render_err; }
extern "C" int rg_sizeof_render_params(void) { return static_cast<int>(sizeof(rg_render_params)); }

extern "C" int rg_render(const rg_scenario_params *params, const rg_state *state, int32_t num_envs, const rg_render_params *rp,
                         uint8_t *rgb, void *hip_stream) {
    using namespace rg::render;
    const rg::Fail fail{g_render_err, sizeof(g_render_err), "rg_render"};
    if (!params) return fail(-1, "params is NULL");
    if (!state) return fail(-2, "state is NULL");
    if (!rp) return fail(-3, "rp (rg_render_params) is NULL");
    if (!rgb) return fail(-4, "rgb is NULL");
    if (!rg::all_aligned(4, rgb)) return fail(-5, "rgb must be 4-byte aligned");
    const rg_scenario_params &p = *params;
    if (p.scenario < RG_SCN_PREDATOR_CAPTURE_PREY || p.scenario > RG_SCN_ARCTIC_TRANSPORT) return fail(-80, "params.scenario unknown");
    if (p.n_agents < 1 || p.n_agents > RG_MAX_AGENTS) return fail(-81, "params.n_agents outside 1..16");
    const bool has_prey = p.scenario == RG_SCN_PREDATOR_CAPTURE_PREY || p.scenario == RG_SCN_SIMPLE;
    if (has_prey && (p.num_prey < 1 || p.num_prey > RG_MAX_PREY)) return fail(-82, "params.num_prey outside 1..64");
    if (!std::isfinite(p.bound_x0) || !std::isfinite(p.bound_y0) || !std::isfinite(p.bound_w) || !std::isfinite(p.bound_h) ||
        !(p.bound_w > 0.0f) || !(p.bound_h > 0.0f) || std::fabs(p.bound_x0) > MAX_COORDINATE || std::fabs(p.bound_y0) > MAX_COORDINATE ||
        p.bound_w > MAX_COORDINATE || p.bound_h > MAX_COORDINATE)
        return fail(-83, "params.bound_x0 / bound_y0 / bound_w / bound_h: the arena must be finite, of a positive size, within 1000 m");
    if (!(p.robot_diameter > 0.0f) || !std::isfinite(p.robot_diameter)) return fail(-84, "params.robot_diameter must be positive and finite");
    if (num_envs < 1) return fail(-85, "num_envs must be >= 1");
    if (rp->width < 8 || rp->width > 1024) return fail(-86, "width outside 8..1024");
    if (rp->width % 4 != 0) return fail(-87, "width must be a multiple of 4");
    if (rp->height < 8 || rp->height > 1024) return fail(-88, "height outside 8..1024");
    if (rp->n_frames < 1) return fail(-89, "n_frames must be >= 1");
    const int64_t n_tiles = (static_cast<int64_t>(rp->width / 4) * rp->height + BLOCK * QUADS_PER_LANE - 1) / (BLOCK * QUADS_PER_LANE);
    if (!rg::elements_fit(n_tiles, rp->n_frames)) return fail(-90, "n_frames: more than 2^31 - 1 work-groups at this width and height");
    const int32_t all = RG_RENDER_ARENA | RG_RENDER_ZONES | RG_RENDER_MARKERS | RG_RENDER_RINGS | RG_RENDER_ROBOTS | RG_RENDER_HEADING;
    if (rp->layers & ~all) return fail(-91, "layers has bits outside the RG_RENDER_* mask");
    if (!rp->env_index && rp->n_frames > num_envs) return fail(-92, "env_index is NULL and n_frames exceeds num_envs");
    // (a coordinate's ulp stays far below CULL_MARGIN: 1.2e-4 m at 2000 m)
    if (!(std::fabs(rp->view_x0) <= MAX_COORDINATE) || !(std::fabs(rp->view_y0) <= MAX_COORDINATE))
        return fail(-93, "view_x0 / view_y0 must be finite and within 1000 m of the origin");
    if (!(rp->view_w >= 0.0f && rp->view_w <= MAX_COORDINATE)) return fail(-94, "view_w must be finite, not negative, at most 1000 m");
    if (!(rp->view_h >= 0.0f && rp->view_h <= MAX_COORDINATE)) return fail(-95, "view_h must be finite, not negative, at most 1000 m");
    if (rp->view_w > 0.0f && !(rp->view_h > 0.0f)) return fail(-96, "view_h must be positive when view_w is");
    if (!state->poses) return fail(-97, "state.poses is NULL");
    if (has_prey && (!state->prey_loc || !state->prey_sensed || !state->prey_captured))
        return fail(-98, "state.prey_loc / prey_sensed / prey_captured is NULL (the scenario draws its prey)");
    if (p.scenario == RG_SCN_ARCTIC_TRANSPORT && !state->grid) return fail(-99, "state.grid is NULL (ArcticTransport draws its terrain)");

    Args a = {};
    a.poses = state->poses;
    a.prey_loc = has_prey ? state->prey_loc : nullptr;
    a.prey_sensed = state->prey_sensed;
    a.prey_captured = state->prey_captured;
    a.grid = state->grid;
    a.env_index = rp->env_index;
    a.rgb = rgb;
    a.num_envs = num_envs;
    a.n_agents = p.n_agents;
    a.num_prey = has_prey ? p.num_prey : 0;
    a.width = rp->width;
    a.height = rp->height;
    a.layers = rp->layers ? rp->layers : all;
    a.quads_per_row = rp->width / 4;
    a.quads = a.quads_per_row * rp->height;
    a.inv_quads_per_row = 1.0f / static_cast<float>(a.quads_per_row);
    a.arctic = p.scenario == RG_SCN_ARCTIC_TRANSPORT;
    a.zone1 = p.scenario == RG_SCN_MATERIAL_TRANSPORT;
    const bool whole = rp->view_w == 0.0f;
    const float vx0 = whole ? p.bound_x0 : rp->view_x0, vy0 = whole ? p.bound_y0 : rp->view_y0;
    const float vw = whole ? p.bound_w : rp->view_w, vh = whole ? p.bound_h : rp->view_h;
    a.x0 = vx0;
    a.y_top = vy0 + vh;
    a.sx = vw / static_cast<float>(rp->width);
    a.sy = vh / static_cast<float>(rp->height);
    a.px = a.sx > a.sy ? a.sx : a.sy;
    a.ax0 = p.bound_x0;
    a.ax1 = p.bound_x0 + p.bound_w;
    a.ay0 = p.bound_y0;
    a.ay1 = p.bound_y0 + p.bound_h;
    a.robot_r = p.robot_diameter * 0.5f;
    a.zone1_r = p.zone1_radius;
    auto rect = [&a](float x0, float x1, float y0, float y1, uint8_t colour) {
        float *r = a.rect[a.n_rects];
        r[0] = x0, r[1] = x1, r[2] = y0, r[3] = y1;
        a.rect_colour[a.n_rects++] = colour;
    };
    if (p.scenario == RG_SCN_WAREHOUSE) {           // Warehouse/visualize.py:20-23
        const float w = p.goal_width;
        rect(-1.5f, -1.5f + w, -1.0f, 0.0f, COL_ZONE_A);
        rect(-1.5f, -1.5f + w, 0.0f, 1.0f, COL_ZONE_B);
        rect(1.5f - w, 1.5f, -1.0f, 0.0f, COL_ZONE_B);
        rect(1.5f - w, 1.5f, 0.0f, 1.0f, COL_ZONE_A);
    } else if (p.scenario == RG_SCN_MATERIAL_TRANSPORT) {   // MaterialTransport/visualize.py:21-22
        const float w = p.end_goal_width;
        rect(-1.5f, -1.5f + w, -1.0f, 1.0f, COL_ZONE_A);
        rect(1.5f - w, 1.5f, -1.0f, 1.0f, COL_ZONE_B);
    }
    int n_fast = 0;
    while (n_fast < p.n_agents && p.agent_step[n_fast] == p.agent_step[0]) ++n_fast;
    for (int i = 0; i < p.n_agents; ++i) {
        int cls = 0;
        switch (p.scenario) {
            case RG_SCN_PREDATOR_CAPTURE_PREY:
                cls = p.sensing_radius[i] > 0.0f ? 0 : 1;
                a.ring_r[i] = p.sensing_radius[i] > 0.0f ? p.sensing_radius[i] : p.capture_radius[i] > 0.0f ? p.capture_radius[i] : 0.0f;
                break;
            case RG_SCN_WAREHOUSE: cls = i & 1; break;
            case RG_SCN_MATERIAL_TRANSPORT: cls = i < n_fast ? 0 : 1; break;
            case RG_SCN_ARCTIC_TRANSPORT: cls = i < 2 ? 0 : i == 2 ? 1 : 2; break;
            default: break;
        }
        a.cls_colour[i] = static_cast<uint8_t>(COL_CLASS0 + cls);
    }
    a.tiles = static_cast<int32_t>(n_tiles);
    if (!launch(a, static_cast<uint32_t>(n_tiles * rp->n_frames), hip_stream)) return fail(-30, "the launch failed");
    return 0;
}
