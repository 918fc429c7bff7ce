// robogym_actor_unroll.hip -- rg_actor_unroll: the recurrent actor over every time step of an episode batch in one launch
// (include/robogym.h; the rule and the kernel: actor_unroll.h).  Instantiates unroll_kernel for hidden sizes 64 and 128.
//
// The host entry is handle-free and keeps its own last-error text (as robogym_render.hip and robogym_episodes.hip do): every
// argument check comes before the first HIP call, so the refusals can be exercised without a device.
#include <hip/hip_runtime.h>

#include <cstring>

#include "host_checks.h"

#ifndef RG_UNROLL_HOST_ONLY   // (the sanitized host build, build.py build_host_sanitized: the argument checks without the kernel)
#include "actor_unroll.h"

// every argument validated by rg_actor_unroll below; ip = the padded input width
static hipError_t launch(const rg_actor_weights &w, const rg_actor_unroll_io &io, int ip, void *hip_stream) {
    rg::UnrollArgs ua;
    memset(&ua, 0, sizeof(ua));
    ua.act.w = w;
    ua.act.obs = io.obs;
    ua.act.q = io.q;
    ua.act.actions = io.actions;
    ua.act.E = io.num_episodes;
    ua.act.N = io.n_agents;
    ua.act.D = io.obs_dim;
    ua.act.append_agent_id = io.append_agent_id ? 1 : 0;
    ua.act.ip = ip;
    ua.hidden_in = io.hidden_in;
    ua.hidden_out = io.hidden_out;
    ua.rows = io.rows;
    ua.in_pitch = io.obs_pitch;
    ua.out_pitch = io.out_pitch;
    const int N = io.n_agents;
    ua.tile_inv = (w.n_sets != 1 && N > 1) ? static_cast<uint32_t>(((1ull << 32) + N - 1) / N) : 0u;
    const dim3 tiles(static_cast<uint32_t>(rg::actor_tiles(w.n_sets, io.num_episodes, N)));   // (within 2^31: the entry's element count)
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (w.hidden_dim == 64) hipLaunchKernelGGL((rg::unroll_kernel<64>), tiles, dim3(128), 0, stream, ua);
    else hipLaunchKernelGGL((rg::unroll_kernel<128>), tiles, dim3(256), 0, stream, ua);
    return hipGetLastError();
}
#else
#include "actor_common.h"
static hipError_t launch(const rg_actor_weights &, const rg_actor_unroll_io &, int, void *) { return hipErrorNotSupported; }
#endif

static thread_local char g_unroll_err[256] = "";

extern "C" const char *rg_actor_unroll_last_error(void) { return g_unroll_err; }
extern "C" int rg_sizeof_actor_unroll_io(void) { return static_cast<int>(sizeof(rg_actor_unroll_io)); }

extern "C" int rg_actor_unroll(const rg_actor_weights *w, const rg_actor_unroll_io *io, void *hip_stream) {
    const rg::Fail fail{g_unroll_err, sizeof(g_unroll_err), "rg_actor_unroll"};
    if (!w) return fail(-1, "w", "is NULL");
    if (!io) return fail(-2, "io", "is NULL");
    if (!io->obs) return fail(-3, "io.obs", "is NULL");
    const rg::NamedPtr arrays[] = {{w->w1, "w.w1"}, {w->b1, "w.b1"}, {w->wih, "w.wih"}, {w->bih, "w.bih"},
                                   {w->whh, "w.whh"}, {w->bhh, "w.bhh"}, {w->w2, "w.w2"}, {w->b2, "w.b2"}};
    if (const rg::NamedPtr *f = rg::first_null(arrays)) return fail(-4, f->name, "is NULL (a weight array)");
    if (!w->use_rnn) return fail(-5, "w.use_rnn", "must be nonzero: the actor must be a GRU with gru_packed == 3 (two binary16 planes, pack_gru='f16x2')");
    if (w->gru_packed != 3) return fail(-5, "w.gru_packed", "must be 3: the actor must be a GRU packed as two binary16 planes (pack_gru='f16x2')");
    if (w->hidden_dim != 64 && w->hidden_dim != 128) return fail(-6, "w.hidden_dim", "must be 64 or 128");
    if (w->n_actions < 1 || w->n_actions > 32) return fail(-7, "w.n_actions", "must be in 1..32");
    if (io->num_episodes < 1) return fail(-9, "io.num_episodes", "must be >= 1");
    if (io->n_agents < 1) return fail(-10, "io.n_agents", "must be >= 1");
    if (io->n_agents > 65536) return fail(-10, "io.n_agents", "must be <= 65536");   // (actor_unroll.h: the tile row of a flat row)
    if (io->obs_dim < 1) return fail(-11, "io.obs_dim", "must be >= 1");
    if (io->rows < 1) return fail(-12, "io.rows", "must be >= 1");
    if (w->n_sets != 1 && w->n_sets != io->n_agents) return fail(-8, "w.n_sets", "must be 1 (shared) or io.n_agents");
    const int64_t in_dim = static_cast<int64_t>(io->obs_dim) + (io->append_agent_id ? io->n_agents : 0);
    if (in_dim != w->input_dim) return fail(-13, "w.input_dim", "differs from io.obs_dim (+ io.n_agents with append_agent_id)");
    if (!rg::input_width_fits(in_dim)) return fail(-14, "w.input_dim", "above 64 (padded to a multiple of 8) is not supported");
    if (io->obs_pitch < io->rows) return fail(-15, "io.obs_pitch", "is below io.rows");
    if (io->out_pitch < io->rows) return fail(-16, "io.out_pitch", "is below io.rows");
    if (io->reserved != 0) return fail(-17, "io.reserved", "must be 0");
    if (!io->q && !io->actions && !io->hidden_out) return fail(-18, "io.q, io.actions and io.hidden_out", "are all NULL: nothing to compute");
    const rg::NamedPtr aligned[] = {{io->hidden_in, "io.hidden_in"}, {io->hidden_out, "io.hidden_out"}, {w->w1, "w.w1"},
                                    {w->wih, "w.wih"}, {w->whh, "w.whh"}, {w->w2, "w.w2"}};
    if (const rg::NamedPtr *f = rg::first_misaligned(aligned, 16)) return fail(-19, f->name, "must be 16-byte aligned");
    // the kernel indexes rows and elements of obs, q and actions with 32-bit integers
    const int pitch = io->obs_pitch > io->out_pitch ? io->obs_pitch : io->out_pitch;
    const int width = io->obs_dim > w->n_actions ? io->obs_dim : w->n_actions;
    if (!rg::elements_fit(io->num_episodes, pitch, io->n_agents, width))
        return fail(-20, "io.num_episodes * pitch * n_agents * max(obs_dim, n_actions)", "exceeds 2^31 - 1 elements");

    const hipError_t err = launch(*w, *io, rg::padded_input_width(static_cast<int>(in_dim)), hip_stream);
    if (err != hipSuccess) return fail(-30, "the launch failed:", hipGetErrorString(err));
    return 0;
}
