// mixer_tile.h -- what the kernels of td_targets.h and mixer_grad.h share: the tile of 32 flat rows, the workgroup of three
// wavefronts, the column layout of the first layers' LDS image (td_targets.h "The kernels" explains each), and the accumulator type
// of v_mfma_f32_32x32x2_f32.
#pragma once

namespace rg {

constexpr int TD_TM = 32;                 // rows of a tile
constexpr int TD_NT = 192;                // threads of the qmix workgroup: three wavefronts
constexpr int TD_EMBED = 32;              // mixing_embed_dim
constexpr int TD_HYPER = 64;              // hypernet_embed
constexpr int TD_C1 = 192;                // first-layer columns: 64 + 64 + 32 + 32
constexpr int TD_H1S = TD_C1 + 1;         // row stride of the first layers' LDS image (odd)
constexpr int TD_MAX_SP = 256;            // the padded state width the LDS image holds
constexpr int TD_COL_WF = 64, TD_COL_V = 128, TD_COL_B1 = 160;   // where each hypernetwork's first layer starts
constexpr int TD_PS = TD_EMBED + 1;       // row stride of the [32][32] images of step 5

using f32x16 = __attribute__((ext_vector_type(16))) float;

}  // namespace rg
