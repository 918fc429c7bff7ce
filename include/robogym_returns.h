/* robogym_returns.h -- the policy-gradient side of the C ABI, beside robogym.h: rg_nstep_returns(), the TARGET CRITIC over a whole
 * episode batch and MAPPO's n-step returns in ONE launch.  Additive: robogym.h, its function list and RG_ABI_VERSION are unchanged;
 * a program that wants these entries includes this header (which includes robogym.h) and links the same library.
 *
 * What EPyMARL's ppo_learner computes under no_grad every epoch (critic_type cv_critic / cv_critic_ns, q_nstep n,
 * add_value_last_step; `state` is the concatenated observations).  The rule is stated once in csrc/nstep_returns.h (DESIGN.md
 * section 4 "N-step returns"); in short, for every episode b, with T = rows - 1:
 *   mask    m[t] = filled[t] && (t == 0 || !terminated[t-1]) for t < T, written as 0.0 / 1.0;
 *   needed  row t < T iff m[t]; row T iff add_value_last_step && m[T-1]; nothing else of obs is read;
 *   values  [t][a] = fl(fl(value_scale c) + value_shift) on needed rows, c the critic's output for agent a, and 0.0 elsewhere;
 *   returns [t0][a] = sum over k = 0 .. n, t = t0 + k < T, of g[k] reward[t] m[t] (k < n) or g[n] values[t][a] m[t] (k == n), plus
 *           g[k+1] values[T][a] at t == T-1 when add_value_last_step && m[T-1]; 0.0 where m[t0] == 0; g[k] = (float) pow(gamma, k).
 *
 * The critic's weights, packed once on the host into the K-major layout the kernel streams (marbler_amd/returns.py TargetCritic;
 * torch's Linear.weight is [out][in], every matrix here is its transpose [in][out]); each array 16-byte aligned.  One network for
 * RG_CRITIC_CV, N networks `net_stride` floats apart for RG_CRITIC_CV_NS (network a's arrays start net_stride * a floats behind
 * the pointers); H = hidden_dim, SP = state_dim rounded up to a multiple of 8:
 *   w1    [SP][H]  fc1.weight's state columns, the rows behind state_dim zero;
 *   w1_id [N][H]   RG_CRITIC_CV only (NULL otherwise): fc1.weight's columns state_dim + a, the one-hot agent id's;
 *   b1 [H]; w2 [H][H] fc2.weight; b2 [H]; w3 [H] fc3.weight; b3 [1].
 * Layout: 7 pointers + 6 ints = 80 bytes, checked with rg_sizeof_critic_weights(). */
#ifndef ROBOGYM_RETURNS_H
#define ROBOGYM_RETURNS_H

#include "robogym.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RG_CRITIC_CV = 0, RG_CRITIC_CV_NS = 1 };
enum { RG_NSTEP_MAX = 32, RG_RETURNS_MAX_ROWS = 4096 };
typedef struct rg_critic_weights {
    const float *w1, *w1_id, *b1, *w2, *b2, *w3, *b3;
    int32_t kind;             /* RG_CRITIC_* */
    int32_t n_agents;         /* must equal io.n_agents */
    int32_t state_dim;        /* must equal io.n_agents * io.obs_dim */
    int32_t hidden_dim;       /* 64 or 128 */
    int32_t net_stride;       /* RG_CRITIC_CV_NS: floats between two agents' networks, a multiple of 4; RG_CRITIC_CV: 0 */
    int32_t reserved;
} rg_critic_weights;
int rg_sizeof_critic_weights(void);
/* Layout: 7 pointers + 10 ints + 3 floats + 1 int = 112 bytes, checked with rg_sizeof_nstep_returns_io(). */
typedef struct rg_nstep_returns_io {
    const float *obs;           /* [B][obs_pitch][N][D] */
    const float *reward;        /* [B][flag_pitch] */
    const uint8_t *terminated;  /* [B][flag_pitch] */
    const uint8_t *filled;      /* [B][flag_pitch] */
    float *returns;             /* [B][out_pitch][N]: rows 0 .. rows - 2 are written */
    float *values;              /* [B][value_pitch][N]: rows 0 .. rows - 1 are written */
    float *mask;                /* [B][out_pitch] or NULL: rows 0 .. rows - 2 */
    int32_t num_episodes, n_agents, obs_dim, rows, nstep, add_value_last_step;
    int32_t obs_pitch, flag_pitch, out_pitch, value_pitch;   /* rows an episode takes in obs; the flags; returns and mask; values */
    float gamma, value_scale, value_shift;
    int32_t reserved;
} rg_nstep_returns_io;
int rg_sizeof_nstep_returns_io(void);
/* Handle-free; never allocates, copies or synchronises (safe under stream capture); launches on `hip_stream` of the caller's CURRENT
 * device.  Every argument is checked before the first HIP call.  Errors (text via rg_nstep_returns_last_error(), which names the
 * argument): -1 w, -2 io NULL; -3 obs, reward, terminated, filled, returns or values NULL; -4 an unknown kind; -5 a weight array
 * NULL (w1_id with RG_CRITIC_CV only); -6 or not 16-byte aligned; -7 hidden_dim neither 64 nor 128; -8 w.n_agents != io.n_agents;
 * -9 w.state_dim != io.n_agents * io.obs_dim; -10 num_episodes below 1; -11 rows below 2; -12 n_agents outside 1..RG_MAX_AGENTS;
 * -13 nstep outside 1..RG_NSTEP_MAX; -14 obs_dim below 1, or the padded state wider than 256; -15 obs_pitch, -16 flag_pitch,
 * -17 value_pitch below rows; -18 out_pitch below rows - 1; -19 gamma not finite or outside [0, 1]; -20 w.reserved or io.reserved
 * != 0; -21 an array of more than 2^31 - 1 elements; -22 add_value_last_step neither 0 nor 1; -23 value_scale or value_shift not
 * finite; -24 net_stride: nonzero with RG_CRITIC_CV, or with RG_CRITIC_CV_NS not a multiple of 4 or below 1; -25 rows above
 * RG_RETURNS_MAX_ROWS (the episode's mask is held on chip); -30 the launch failed. */
int rg_nstep_returns(const rg_critic_weights *w, const rg_nstep_returns_io *io, void *hip_stream);
const char *rg_nstep_returns_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
