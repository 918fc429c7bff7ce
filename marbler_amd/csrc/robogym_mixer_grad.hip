// robogym_mixer_grad.hip -- rg_mixer_forward / rg_mixer_backward: the online mixer's pass of an episode batch with gradients, one
// launch each (include/robogym_learn.h; the rule and the kernels: mixer_grad.h).
//
// The host entries are handle-free and keep their own last-error text (as robogym_gru_scan.hip does): every argument check comes
// before the first HIP call, so the refusals can be exercised without a device.
#include <hip/hip_runtime.h>

#include <cstring>

#include "host_checks.h"

#ifndef RG_MIXER_GRAD_HOST_ONLY   // (the sanitized host program, tests/sanitize/mixer_host.cpp: the argument checks without the kernels)
#include "mixer_grad.h"

// every argument validated by mix() below; tiles: the workgroups of the launch
static hipError_t launch(const rg_mixer_grad_weights &w, const rg_mixer_grad_io &io, int backward, int tiles, void *hip_stream) {
    rg::MgArgs ma;
    memset(&ma, 0, sizeof(ma));
    ma.w = w;
    ma.io = io;
    ma.T = io.rows - 1;
    ma.total = io.num_episodes * (io.rows - 1);
    ma.sp = (io.n_agents * io.obs_dim + 3) / 4 * 4;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (w.m.kind == RG_MIXER_QMIX) {
        const dim3 grid(tiles), block(rg::TD_NT);
        if (!backward) hipLaunchKernelGGL(rg::mix_qmix_forward_kernel, grid, block, 0, stream, ma);
        else if (io.n_agents <= 8) hipLaunchKernelGGL(rg::mix_qmix_backward_kernel<8>, grid, block, 0, stream, ma);
        else hipLaunchKernelGGL(rg::mix_qmix_backward_kernel<16>, grid, block, 0, stream, ma);
    } else {
        if (backward) hipLaunchKernelGGL(rg::mix_gather_backward_kernel, dim3(tiles), dim3(256), 0, stream, ma);
        else hipLaunchKernelGGL(rg::mix_gather_forward_kernel, dim3(tiles), dim3(256), 0, stream, ma);
    }
    return hipGetLastError();
}
#else
#include "../../include/robogym_learn.h"
// the program's own
hipError_t rg_mixer_grad_launch_stub(const rg_mixer_grad_weights &w, const rg_mixer_grad_io &io, int backward, int tiles, void *hip_stream);
static hipError_t launch(const rg_mixer_grad_weights &w, const rg_mixer_grad_io &io, int backward, int tiles, void *hip_stream) {
    return rg_mixer_grad_launch_stub(w, io, backward, tiles, hip_stream);
}
#endif

static thread_local char g_mg_err[256] = "";

extern "C" const char *rg_mixer_grad_last_error(void) { return g_mg_err; }
extern "C" int rg_sizeof_mixer_grad_weights(void) { return static_cast<int>(sizeof(rg_mixer_grad_weights)); }
extern "C" int rg_sizeof_mixer_grad_io(void) { return static_cast<int>(sizeof(rg_mixer_grad_io)); }

static int mix(const char *entry, int backward, const rg_mixer_grad_weights *w, const rg_mixer_grad_io *io, void *hip_stream) {
    const rg::Fail fail{g_mg_err, sizeof(g_mg_err), entry};
    if (!w) return fail(-1, "w", "is NULL");
    if (!io) return fail(-2, "io", "is NULL");
    const rg_mixer_weights &m = w->m;
    if (m.kind != RG_MIXER_NONE && m.kind != RG_MIXER_VDN && m.kind != RG_MIXER_QMIX)
        return fail(-4, "w.m.kind", "is none of RG_MIXER_NONE, RG_MIXER_VDN, RG_MIXER_QMIX");
    const bool qmix = m.kind == RG_MIXER_QMIX;
    // what this launch reads and writes
    const rg::NamedPtr fwd[] = {{io->q, "io.q", 4}, {io->actions, "io.actions", 4}, {io->mask, "io.mask", 4}, {io->mixed, "io.mixed", 4},
                                {io->obs, "io.obs", 4}};
    const rg::NamedPtr bwd[] = {{io->actions, "io.actions", 4}, {io->mask, "io.mask", 4}, {io->d_mixed, "io.d_mixed", 4}, {io->d_q, "io.d_q", 4},
                                {io->q, "io.q", 4}, {io->obs, "io.obs", 4}, {io->d_pre, "io.d_pre", 4}, {io->d_p2, "io.d_p2", 4}, {io->g, "io.g", 4}};
    if (const rg::NamedPtr *f = backward ? rg::first_null(bwd, qmix ? 9 : 4) : rg::first_null(fwd, qmix ? 5 : 4)) return fail(-3, f->name, "is NULL");
    if (const rg::NamedPtr *f = backward ? rg::first_misaligned(bwd) : rg::first_misaligned(fwd)) return fail(-6, f->name, "must be 4-byte aligned");
    if (qmix) {
        const rg::NamedPtr weights[] = {{m.w_in, "w.m.w_in"}, {m.b_in, "w.m.b_in"}, {m.w_w1, "w.m.w_w1"}, {m.b_w1, "w.m.b_w1"}, {m.w_wf, "w.m.w_wf"},
                                        {m.b_wf, "w.m.b_wf"}, {m.w_v, "w.m.w_v"}, {m.b_v, "w.m.b_v"}, {w->w1b, "w.w1b"}, {w->wfb, "w.wfb"}};
        if (const rg::NamedPtr *f = rg::first_null(weights, backward ? 10 : 8)) return fail(-5, f->name, "is NULL (a weight array of the qmix mixer)");
        if (const rg::NamedPtr *f = rg::first_misaligned(weights, 16)) return fail(-6, f->name, "must be 16-byte aligned");
        if (m.embed_dim != 32) return fail(-7, "w.m.embed_dim", "must be 32 (mixing_embed_dim: 32 is the only instantiation)");
        if (m.hypernet_embed != 64) return fail(-7, "w.m.hypernet_embed", "must be 64 (hypernet_layers: 2 with hypernet_embed: 64 is the only instantiation)");
    }
    if (m.n_agents != io->n_agents) return fail(-8, "w.m.n_agents", "differs from io.n_agents");
    if (io->num_episodes < 1) return fail(-10, "io.num_episodes", "must be >= 1");
    if (io->rows < 2) return fail(-11, "io.rows", "must be >= 2");
    if (io->n_agents < 1 || io->n_agents > RG_MAX_AGENTS) return fail(-12, "io.n_agents", "must be in 1..16 (RG_MAX_AGENTS)");
    if (io->n_actions < 1 || io->n_actions > 32) return fail(-13, "io.n_actions", "must be in 1..32");
    const int64_t S = static_cast<int64_t>(io->n_agents) * io->obs_dim;
    if (qmix) {
        if (io->obs_dim < 1) return fail(-14, "io.obs_dim", "must be >= 1");
        if (m.state_dim != S) return fail(-9, "w.m.state_dim", "differs from io.n_agents * io.obs_dim");
        if ((S + 3) / 4 * 4 > 256) return fail(-14, "io.obs_dim", "makes the state (n_agents * obs_dim, padded to a multiple of 4) wider than 256");
        if (io->obs_pitch < io->rows) return fail(-15, "io.obs_pitch", "is below io.rows");
    }
    if (io->q_pitch < io->rows) return fail(-16, "io.q_pitch", "is below io.rows");
    if (io->out_pitch < io->rows - 1) return fail(-17, "io.out_pitch", "is below io.rows - 1");
    if (qmix && backward && io->aux_pitch < io->rows) return fail(-18, "io.aux_pitch", "is below io.rows");
    if (m.reserved != 0) return fail(-20, "w.m.reserved", "must be 0");
    if (io->reserved != 0) return fail(-20, "io.reserved", "must be 0");
    // the element counts of every array of this launch: below 2^31 (a row is a product of 32-bit factors)
    const int64_t B = io->num_episodes, N = io->n_agents;
    if (!rg::elements_fit(B, io->q_pitch, N, io->n_actions)) return fail(-21, "io.num_episodes * q_pitch * n_agents * n_actions", "exceeds 2^31 - 1 elements");
    if (qmix && !rg::elements_fit(B, io->obs_pitch, N, io->obs_dim)) return fail(-21, "io.num_episodes * obs_pitch * n_agents * obs_dim", "exceeds 2^31 - 1 elements");
    if (!rg::elements_fit(B, io->out_pitch, N)) return fail(-21, "io.num_episodes * out_pitch * n_agents", "exceeds 2^31 - 1 elements");
    if (qmix && backward && !rg::elements_fit(B, io->aux_pitch, 32 * N + 32)) return fail(-21, "io.num_episodes * aux_pitch * (32 n_agents + 32)", "exceeds 2^31 - 1 elements");

    // qmix: one workgroup per tile of 32 flat rows r = b T + t; none / vdn: 256 rows per workgroup
    const int64_t total = B * (io->rows - 1), per = qmix ? 32 : 256;
    const hipError_t err = launch(*w, *io, backward, static_cast<int>((total + per - 1) / per), hip_stream);
    if (err != hipSuccess) return fail(-30, "the launch failed:", hipGetErrorString(err));
    return 0;
}

extern "C" int rg_mixer_forward(const rg_mixer_grad_weights *w, const rg_mixer_grad_io *io, void *hip_stream) {
    return mix("rg_mixer_forward", 0, w, io, hip_stream);
}
extern "C" int rg_mixer_backward(const rg_mixer_grad_weights *w, const rg_mixer_grad_io *io, void *hip_stream) {
    return mix("rg_mixer_backward", 1, w, io, hip_stream);
}
