/* robogym_learn.h -- the training side of the C ABI, beside robogym.h: rg_gru_scan_forward() and rg_gru_scan_backward(), the
 * sequential part of a recurrent actor's pass WITH gradients over a whole episode batch, in one launch each.  Additive: robogym.h,
 * its function list and RG_ABI_VERSION are unchanged; a program that wants these entries includes this header (which includes
 * robogym.h) and links the same library.
 *
 * torch.nn.GRUCell's recurrence for every flat row (b, n) -- agent n of episode b -- independently, all in float32.  The rule is
 * stated once in csrc/gru_scan.h (DESIGN.md section 4 "Trainable actor"); in short, with H = hidden_dim and the gates in torch's
 * order r, z, n:
 *   forward   for t = 0 .. rows-1: gh = h_{t-1} W_hh^T + b_hh; r = s(gi_r + gh_r); z = s(gi_z + gh_z); n = tanh(gi_n + r gh_n);
 *             h_t = (1 - z) n + z h_{t-1}; h and (when asked for) gates = (r, z, n, gh_n) of every step are stored;
 *   backward  for t = rows-1 .. 0: dh = dh_ext_t + carry; dn = dh (1 - z); dz = dh (h_{t-1} - n); da_n = dn (1 - n^2);
 *             da_r = (da_n gh_n) r (1 - r); da_z = dz z (1 - z); dgi = (da_r, da_z, da_n); dghn = da_n r;
 *             carry = dh z + (da_r, da_z, dghn) W_hh.
 * What is batched over all rows -- the input products in front of gi, the output layer behind h, and every weight gradient -- is the
 * caller's (marbler_amd/learn.py does it with torch's GEMMs).
 *
 * The weights are torch's own: w_hh [A][3H][H] (GRUCell.weight_hh) and b_hh [A][3H], with A = n_sets = 1 (shared) or n_agents (one
 * set per agent).  w_hh_t, optional, is a copy [A][H][3H] (each set transposed) for the forward launch; NULL: the forward launch
 * gathers its operand from w_hh once.  Layout: 3 pointers + 4 ints = 40 bytes, checked with rg_sizeof_gru_scan_weights(). */
#ifndef ROBOGYM_LEARN_H
#define ROBOGYM_LEARN_H

#include "robogym.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RG_GRU_SCAN_MAX_ROWS = 4096 };
typedef struct rg_gru_scan_weights {
    const float *w_hh;      /* [A][3H][H], 16-byte aligned */
    const float *b_hh;      /* [A][3H]; the forward launch only (the backward launch does not look at it) */
    const float *w_hh_t;    /* [A][H][3H] or NULL; the forward launch only */
    int32_t n_sets;         /* 1 or io.n_agents */
    int32_t hidden_dim;     /* 64 or 128 */
    int32_t reserved[2];
} rg_gru_scan_weights;
int rg_sizeof_gru_scan_weights(void);
/* Layout: 10 pointers + 8 ints = 112 bytes, checked with rg_sizeof_gru_scan_io().  B = num_episodes, N = n_agents. */
typedef struct rg_gru_scan_io {
    const float *gi;            /* forward in:  [B][gi_pitch][N][3H] */
    const float *hidden_in;     /* both, in:    [B][N][H] or NULL (zeros): the state before row 0 */
    float *h;                   /* forward out, backward in: [B][save_pitch][N][H] */
    float *gates;               /* forward out (or NULL), backward in: [B][save_pitch][N][4H] = (r, z, n, gh_n) */
    float *hidden_out;          /* forward out: [B][N][H] or NULL, the state after the last row */
    const float *dh_ext;        /* backward in:  [B][grad_pitch][N][H] */
    const float *d_hidden_out;  /* backward in:  [B][N][H] or NULL (zeros): the gradient of hidden_out */
    float *dgi;                 /* backward out: [B][grad_pitch][N][3H] */
    float *dghn;                /* backward out: [B][grad_pitch][N][H] */
    float *d_hidden_in;         /* backward out: [B][N][H] or NULL, the gradient of hidden_in */
    int32_t num_episodes, n_agents, rows;
    int32_t gi_pitch, save_pitch, grad_pitch;   /* rows an episode takes in gi; in h and gates; in dh_ext, dgi and dghn */
    int32_t reserved[2];
} rg_gru_scan_io;
int rg_sizeof_gru_scan_io(void);
/* Handle-free; never allocate, copy or synchronise (safe under stream capture); launch on `hip_stream` of the caller's CURRENT
 * device.  Every argument is checked before the first HIP call; a launch looks only at its own pointers and pitches (forward: gi,
 * hidden_in, h, gates, hidden_out, gi_pitch, save_pitch; backward: the others, with h, gates, hidden_in and save_pitch).  Rows
 * behind `rows` and the pitch padding of every output are not touched.  Errors (text via rg_gru_scan_last_error(), which names the
 * argument): -1 w, -2 io NULL; -3 a required array of io NULL (forward: gi, h; backward: h, dh_ext, dgi, dghn); -4 w.w_hh NULL, or
 * w.b_hh in the forward launch; -5 an array of w not 16-byte aligned, or one of io not 4-byte aligned; -6 hidden_dim neither 64 nor
 * 128; -7 n_sets neither 1 nor n_agents; -8 n_agents outside 1..RG_MAX_AGENTS; -9 num_episodes below 1; -10 rows below 1; -11 rows
 * above RG_GRU_SCAN_MAX_ROWS; -12 gi_pitch, -13 save_pitch, -14 grad_pitch below rows; -15 the backward launch without gates; -20 a
 * reserved field != 0; -21 an array of more than 2^31 - 1 elements; -30 the launch failed. */
int rg_gru_scan_forward(const rg_gru_scan_weights *w, const rg_gru_scan_io *io, void *hip_stream);
int rg_gru_scan_backward(const rg_gru_scan_weights *w, const rg_gru_scan_io *io, void *hip_stream);
const char *rg_gru_scan_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
