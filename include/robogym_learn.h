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

/* rg_mixer_forward() and rg_mixer_backward(): the ONLINE mixer's pass of a Q-learner's training step with gradients -- the chosen
 * actions' values of rows t < T = rows - 1 of an episode batch, mixed by none / vdn / EPyMARL's QMixer on the state of row t -- in one
 * launch each.  The rule is stated once in csrc/mixer_grad.h (DESIGN.md section 4 "Trainable mixer").  The backward launch recomputes
 * the forward pass and writes d_q whole (zeros included) and, for qmix, the per-row arrays that the weight gradients are sums of;
 * the sums themselves are the caller's (marbler_amd/mixers.py does them with torch's GEMMs).
 *
 * The weights: `m` as rg_td_targets takes them (robogym.h rg_mixer_weights: the packed, K-major arrays; none / vdn: kind and n_agents
 * alone), and for the qmix backward launch the second layers as torch keeps them: w1b = hyper_w_1.2.weight [32 N][64] and wfb =
 * hyper_w_final.2.weight [32][64], 16-byte aligned.  Layout: 88 + 2 pointers = 104 bytes, checked with rg_sizeof_mixer_grad_weights(). */
typedef struct rg_mixer_grad_weights {
    rg_mixer_weights m;
    const float *w1b;       /* [32 N][64]; the qmix backward launch only */
    const float *wfb;       /* [32][64];   the qmix backward launch only */
} rg_mixer_grad_weights;
int rg_sizeof_mixer_grad_weights(void);
/* Layout: 10 pointers + 10 ints = 120 bytes, checked with rg_sizeof_mixer_grad_io().  B = num_episodes, N = n_agents, T = rows - 1. */
typedef struct rg_mixer_grad_io {
    const float *q;             /* both (backward: qmix only), in: [B][q_pitch][N][A] */
    const int32_t *actions;     /* both, in: [B][q_pitch][N] */
    const float *obs;           /* qmix, both, in: [B][obs_pitch][N][D] */
    const float *mask;          /* both, in: [B][out_pitch] */
    float *mixed;               /* forward out: [B][out_pitch], with RG_MIXER_NONE [B][out_pitch][N] */
    const float *d_mixed;       /* backward in: laid out as mixed */
    float *d_q;                 /* backward out: [B][q_pitch][N][A], rows 0 .. T written */
    float *d_pre;               /* qmix backward out: [B][aux_pitch][192], rows 0 .. T written */
    float *d_p2;                /* qmix backward out: [B][aux_pitch][32 N + 32] */
    float *g;                   /* qmix backward out: [B][aux_pitch][160] */
    int32_t num_episodes, n_agents, obs_dim, n_actions, rows;
    int32_t q_pitch, obs_pitch, out_pitch, aux_pitch;   /* rows an episode takes in q, actions and d_q; in obs; in mask, mixed and d_mixed; in d_pre, d_p2 and g */
    int32_t reserved;
} rg_mixer_grad_io;
int rg_sizeof_mixer_grad_io(void);
/* Handle-free; never allocate, copy or synchronise (safe under stream capture); launch on `hip_stream` of the caller's CURRENT
 * device.  Every argument is checked before the first HIP call; a launch looks only at its own pointers and pitches.  Errors (text via
 * rg_mixer_grad_last_error(), which names the argument): -1 w, -2 io NULL; -3 a required array of io NULL (forward: q, actions, mask,
 * mixed, and obs with qmix; backward: actions, mask, d_mixed, d_q, and with qmix q, obs, d_pre, d_p2, g); -4 w.m.kind; -5 a weight array
 * of the qmix mixer NULL (backward: w1b and wfb too); -6 a weight array not 16-byte aligned, or an array of io not 4-byte aligned; -7
 * embed_dim != 32 or hypernet_embed != 64; -8 w.m.n_agents != io.n_agents; -9 w.m.state_dim != n_agents * obs_dim; -10 num_episodes
 * below 1; -11 rows below 2; -12 n_agents outside 1..RG_MAX_AGENTS; -13 n_actions outside 1..32; -14 obs_dim below 1 or the padded
 * state wider than 256 (qmix); -15 obs_pitch below rows (qmix); -16 q_pitch below rows; -17 out_pitch below rows - 1; -18 aux_pitch
 * below rows (qmix backward); -20 a reserved field != 0; -21 an array of more than 2^31 - 1 elements; -30 the launch failed. */
int rg_mixer_forward(const rg_mixer_grad_weights *w, const rg_mixer_grad_io *io, void *hip_stream);
int rg_mixer_backward(const rg_mixer_grad_weights *w, const rg_mixer_grad_io *io, void *hip_stream);
const char *rg_mixer_grad_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
