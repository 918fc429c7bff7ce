// robogym_td_targets.hip -- rg_td_targets: the target mixer and the double-Q TD targets of an episode batch in one launch
// (include/robogym.h; the rule and the kernels: td_targets.h).
//
// The host entry is handle-free and keeps its own last-error text (as robogym_actor_unroll.hip does): every argument check comes
// before the first HIP call, so the refusals can be exercised without a device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "host_checks.h"

#ifndef RG_TD_TARGETS_HOST_ONLY   // (the sanitized host program, tests/sanitize/td_targets_host.cpp: the argument checks without the kernels)
#include "td_targets.h"

// every argument validated by rg_td_targets below
static hipError_t launch(const rg_mixer_weights &m, const rg_td_targets_io &io, void *hip_stream) {
    rg::TdArgs ta;
    memset(&ta, 0, sizeof(ta));
    ta.m = m;
    ta.io = io;
    ta.T = io.rows - 1;
    ta.total = io.num_episodes * (io.rows - 1);
    ta.sp = (io.n_agents * io.obs_dim + 3) / 4 * 4;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (m.kind == RG_MIXER_QMIX) hipLaunchKernelGGL(rg::td_qmix_kernel, dim3((ta.total + rg::TD_TM - 1) / rg::TD_TM), dim3(rg::TD_NT), 0, stream, ta);
    else hipLaunchKernelGGL(rg::td_gather_kernel, dim3((ta.total + 255) / 256), dim3(256), 0, stream, ta);
    return hipGetLastError();
}
#else
#include "../../include/robogym.h"
hipError_t rg_td_targets_launch_stub(const rg_mixer_weights &m, const rg_td_targets_io &io, void *hip_stream);   // the program's own
static hipError_t launch(const rg_mixer_weights &m, const rg_td_targets_io &io, void *hip_stream) { return rg_td_targets_launch_stub(m, io, hip_stream); }
#endif

static thread_local char g_td_err[256] = "";

extern "C" const char *rg_td_targets_last_error(void) { return g_td_err; }
extern "C" int rg_sizeof_td_targets_io(void) { return static_cast<int>(sizeof(rg_td_targets_io)); }
extern "C" int rg_sizeof_mixer_weights(void) { return static_cast<int>(sizeof(rg_mixer_weights)); }

extern "C" int rg_td_targets(const rg_mixer_weights *m, const rg_td_targets_io *io, void *hip_stream) {
    const rg::Fail fail{g_td_err, sizeof(g_td_err), "rg_td_targets"};
    if (!m) return fail(-1, "m", "is NULL");
    if (!io) return fail(-2, "io", "is NULL");
    const rg::NamedPtr required[] = {{io->qt, "io.qt"}, {io->reward, "io.reward"}, {io->terminated, "io.terminated"}, {io->filled, "io.filled"},
                                 {io->targets, "io.targets"}};
    if (const rg::NamedPtr *f = rg::first_null(required)) return fail(-3, f->name, "is NULL");
    if (m->kind != RG_MIXER_NONE && m->kind != RG_MIXER_VDN && m->kind != RG_MIXER_QMIX)
        return fail(-4, "m.kind", "is none of RG_MIXER_NONE, RG_MIXER_VDN, RG_MIXER_QMIX");
    const bool qmix = m->kind == RG_MIXER_QMIX;
    if (qmix) {
        if (!io->obs) return fail(-3, "io.obs", "is NULL (the qmix mixer reads the state from it)");
        const rg::NamedPtr weights[] = {{m->w_in, "m.w_in"}, {m->b_in, "m.b_in"}, {m->w_w1, "m.w_w1"}, {m->b_w1, "m.b_w1"},
                                    {m->w_wf, "m.w_wf"}, {m->b_wf, "m.b_wf"}, {m->w_v, "m.w_v"}, {m->b_v, "m.b_v"}};
        if (const rg::NamedPtr *f = rg::first_null(weights)) return fail(-5, f->name, "is NULL (a weight array of the qmix mixer)");
        if (const rg::NamedPtr *f = rg::first_misaligned(weights, 16)) return fail(-6, f->name, "must be 16-byte aligned");
        if (m->embed_dim != 32) return fail(-7, "m.embed_dim", "must be 32 (mixing_embed_dim: 32 is the only instantiation)");
        if (m->hypernet_embed != 64) return fail(-7, "m.hypernet_embed", "must be 64 (hypernet_layers: 2 with hypernet_embed: 64 is the only instantiation)");
    }
    if (m->n_agents != io->n_agents) return fail(-8, "m.n_agents", "differs from io.n_agents");
    if (io->num_episodes < 1) return fail(-10, "io.num_episodes", "must be >= 1");
    if (io->rows < 2) return fail(-11, "io.rows", "must be >= 2");
    if (io->n_agents < 1 || io->n_agents > RG_MAX_AGENTS) return fail(-12, "io.n_agents", "must be in 1..16 (RG_MAX_AGENTS)");
    if (io->n_actions < 1 || io->n_actions > 32) return fail(-13, "io.n_actions", "must be in 1..32");
    if (io->obs_dim < 1) return fail(-14, "io.obs_dim", "must be >= 1");
    const int64_t S = static_cast<int64_t>(io->n_agents) * io->obs_dim;
    if (qmix) {
        if (m->state_dim != S) return fail(-9, "m.state_dim", "differs from io.n_agents * io.obs_dim");
        if ((S + 3) / 4 * 4 > 256) return fail(-14, "io.obs_dim", "makes the state (n_agents * obs_dim, padded to a multiple of 4) wider than 256");
    }
    if (io->obs_pitch < io->rows) return fail(-15, "io.obs_pitch", "is below io.rows");
    if (io->q_pitch < io->rows) return fail(-16, "io.q_pitch", "is below io.rows");
    if (io->flag_pitch < io->rows) return fail(-17, "io.flag_pitch", "is below io.rows");
    if (io->out_pitch < io->rows - 1) return fail(-18, "io.out_pitch", "is below io.rows - 1");
    if (!std::isfinite(io->gamma) || io->gamma < 0.0f || io->gamma > 1.0f) return fail(-19, "io.gamma", "must be finite and in [0, 1]");
    if (m->reserved != 0) return fail(-20, "m.reserved", "must be 0");
    if (io->reserved != 0) return fail(-20, "io.reserved", "must be 0");
    // the element counts of every array: below 2^31 (a row is a product of two 32-bit factors)
    const struct {
        int64_t pitch, row;
        const char *name;
    } counts[] = {{io->q_pitch, static_cast<int64_t>(io->n_agents) * io->n_actions, "io.num_episodes * q_pitch * n_agents * n_actions"},
                  {io->obs_pitch, S, "io.num_episodes * obs_pitch * n_agents * obs_dim"},
                  {io->flag_pitch, 1, "io.num_episodes * flag_pitch"},
                  {io->out_pitch, io->n_agents, "io.num_episodes * out_pitch * n_agents"}};
    for (const auto &c : counts)
        if (!rg::elements_fit(io->num_episodes, c.pitch, c.row)) return fail(-21, c.name, "exceeds 2^31 - 1 elements");

    const hipError_t err = launch(*m, *io, hip_stream);
    if (err != hipSuccess) return fail(-30, "the launch failed:", hipGetErrorString(err));
    return 0;
}
