// render.h -- the picture rg_render draws (include/robogym.h), stated once: palette, layers, shapes, draw order.
//
// A frame is a function of one env's state.  It draws the elements the reference's visualisers draw
// (scenarios/*/visualize.py, shown by utilities/roboEnv.py:67-76), in their roles; it does not reproduce matplotlib's pixels.
// No text (MaterialTransport's zone-load numbers), no window frame, nothing that depends on a figure size.
//
// View.  The image shows the world rectangle (view_x0, view_y0, view_w, view_h); view_w == 0 selects the arena
// (bound_x0, bound_y0, bound_w, bound_h).  With sx = view_w / W and sy = view_h / H, pixel (row i from the top, column j) has the
// world point
//     wx = view_x0 + (j + 0.5) * sx,     wy = (view_y0 + view_h) - (i + 0.5) * sy,
// and px = max(sx, sy) is "one pixel's world size".  All of it binary32, one rounding per operation written (-ffp-contract=off).
//
// Draw order.  A pixel takes the colour of the LAST of these shapes that covers its centre (dx = wx - x, dy = wy - y of a shape
// at (x, y); a disk of radius r covers dx dx + dy dy <= r r; an outline of radius r covers the points whose distance d from the
// centre has |d - r| <= px, evaluated without a root as lo lo <= dx dx + dy dy <= hi hi with lo = max(r - px, 0), hi = r + px; a
// rectangle covers its closed point set):
//   1 RG_RENDER_ARENA    white everywhere, then light grey outside the arena [bound_x0, bound_x0 + bound_w] x
//                        [bound_y0, bound_y0 + bound_h].  (Without the layer the whole image starts white.)
//   2 RG_RENDER_ZONES    Warehouse: [-1.5, -1.5 + goal_width] x [-1, 0] and [1.5 - goal_width, 1.5] x [0, 1] in ZONE_A,
//                          [-1.5, -1.5 + goal_width] x [0, 1] and [1.5 - goal_width, 1.5] x [-1, 0] in ZONE_B, in the order of
//                          Warehouse/visualize.py:20-23.
//                        MaterialTransport: [-1.5, -1.5 + end_goal_width] x [-1, 1] in ZONE_A, [1.5 - end_goal_width, 1.5] x
//                          [-1, 1] in ZONE_B.
//                        ArcticTransport: terrain cell (i, j) with grid[i][j] > 0 is the square [0.25 j - 1.5, 0.25 j - 1.25] x
//                          [0.75 - 0.25 i, 1 - 0.25 i] (the reference's get_pose_from_cell, the inverse of the step kernels' cell
//                          lookup) in ICE (1), WATER (2) or GOAL (3).  Evaluated per pixel as u = (wx + 1.5) * 4,
//                          v = (1 - wy) * 4, cell (floor v, floor u) where 0 <= u < 12 and 0 <= v < 8.
//   3 RG_RENDER_MARKERS  PredatorCapturePrey: every prey with prey_captured == 0 as a disk of radius 0.025 m, PREY, or
//                          PREY_SENSED where prey_sensed != 0.  Simple: its goal (prey_loc, one entry) the same way.
//                        MaterialTransport: the outline of radius zone1_radius about the origin, ZONE1.
//   4 RG_RENDER_RINGS    PredatorCapturePrey: per agent the outline of radius sensing_radius[a] if that is > 0, otherwise
//                          capture_radius[a] (none if that is not > 0 either), in the agent's class colour.  True radii of
//                          rg_scenario_params -- not a team pool's.
//   5 RG_RENDER_ROBOTS   per agent a disk of radius robot_diameter / 2 in its class colour.  Classes: PredatorCapturePrey
//                          sensing_radius[a] > 0 -> 0, else 1; Warehouse even index 0, odd 1; MaterialTransport 0 for the leading
//                          agents whose agent_step equals agent_step[0] (the fast ones: index < n_fast_agents), 1 after them;
//                          ArcticTransport index < 2 -> 0, == 2 -> 1, the rest 2; Simple 0.
//   6 RG_RENDER_HEADING  per agent with |theta| <= 8 (sincos_spec's domain) the segment from the centre to the rim along
//                          (c, s) = sincos_spec(theta): covered where 0 <= dx c + dy s <= robot_diameter / 2 and
//                          |dy c - dx s| <= px, HEADING.
// Within a layer shapes are drawn in index order.  Every test is a comparison that is false for a NaN, so a non-finite pose
// draws nothing; what lies outside the view is clipped.  An env_index entry outside [0, E) gives a frame without state-dependent
// shapes (arena and fixed zones only).
#pragma once
#include <stdint.h>

#include "../../include/robogym.h"

namespace rg {
namespace render {

// the palette: index -> (R, G, B).  marbler_amd/render.py PALETTE mirrors it; every entry is distinct.
enum Colour : uint8_t {
    COL_BACKGROUND = 0, COL_SURROUND, COL_ZONE_A, COL_ZONE_B, COL_ICE, COL_WATER, COL_GOAL, COL_PREY, COL_PREY_SENSED, COL_ZONE1,
    COL_CLASS0, COL_CLASS1, COL_CLASS2, COL_HEADING, COL_COUNT
};
#define RG_RENDER_PALETTE                                                                                                          \
    {255, 255, 255}, {224, 224, 224}, {255, 221, 128}, {170, 238, 153}, {190, 230, 255}, {70, 130, 220}, {120, 200, 120},          \
        {0, 170, 90}, {170, 60, 200}, {230, 130, 40}, {220, 40, 40}, {40, 90, 220}, {240, 190, 20}, {30, 30, 30}

constexpr int MAX_RECTS = 4;
constexpr float PREY_RADIUS = 0.025f;
constexpr float MAX_HEADING_ANGLE = 8.0f;
constexpr float MAX_COORDINATE = 1000.0f;   // metres: the view's and the arena's corner and size, each (rg_render refuses more)
constexpr float CULL_MARGIN = 1e-3f;   // metres a wave's row test allows beyond a shape's extent (robogym_render.hip)
constexpr int BLOCK = 256;          // lanes of a work-group
constexpr int QUADS_PER_LANE = 4;   // a lane owns this many 4-pixel quads of its tile, BLOCK quads apart

// What the kernel gets by value: everything that does not depend on the env, worked out once by the host in binary32.
struct Args {
    const float *poses;            // [E][3][N]
    const float *prey_loc;         // [E][P][2] or NULL
    const uint8_t *prey_sensed;    // [E][P]
    const uint8_t *prey_captured;  // [E][P]
    const uint8_t *grid;           // [E][96] or NULL
    const int32_t *env_index;      // [K] or NULL
    uint8_t *rgb;                  // [K][H][W][3]
    int32_t num_envs, n_agents, num_prey, width, height, layers;
    int32_t quads_per_row, quads;  // W / 4, H * W / 4
    float inv_quads_per_row;
    int32_t tiles;                 // work-groups per frame
    int32_t arctic, zone1;         // draw the terrain / the zone-1 outline
    float x0, y_top, sx, sy, px;   // view
    float ax0, ax1, ay0, ay1;      // arena
    float robot_r, zone1_r;
    int32_t n_rects;
    float rect[MAX_RECTS][4];      // x0, x1, y0, y1
    uint8_t rect_colour[MAX_RECTS];
    float ring_r[RG_MAX_AGENTS];   // 0: none
    uint8_t cls_colour[RG_MAX_AGENTS];
};

}  // namespace render
}  // namespace rg
