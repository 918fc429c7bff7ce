// robogym_nstep_returns.hip -- rg_nstep_returns: the target critic and MAPPO's n-step returns of an episode batch in one launch
// (include/robogym_returns.h; the rule and the kernel: nstep_returns.h).
//
// The host entry is handle-free and keeps its own last-error text (as robogym_td_targets.hip does): every argument check comes
// before the first HIP call, so the refusals can be exercised without a device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "host_checks.h"

#ifndef RG_NSTEP_RETURNS_HOST_ONLY   // (the sanitized host program, tests/sanitize/nstep_returns_host.cpp: the argument checks without the kernel)
#include "nstep_returns.h"

// every argument validated by rg_nstep_returns below
static hipError_t launch(const rg_critic_weights &w, const rg_nstep_returns_io &io, const float *g, void *hip_stream) {
    rg::NrArgs na;
    memset(&na, 0, sizeof(na));
    na.w = w;
    na.io = io;
    na.T = io.rows - 1;
    na.sp = (io.n_agents * io.obs_dim + 7) / 8 * 8;
    memcpy(na.g, g, sizeof(na.g));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (w.hidden_dim == 128) hipLaunchKernelGGL(rg::nstep_returns_kernel<128>, dim3(io.num_episodes), dim3(256), 0, stream, na);
    else hipLaunchKernelGGL(rg::nstep_returns_kernel<64>, dim3(io.num_episodes), dim3(128), 0, stream, na);
    return hipGetLastError();
}
#else
#include "../../include/robogym_returns.h"
// the program's own; g: the discounts g[0 .. RG_NSTEP_MAX + 1], zero behind nstep + 1
hipError_t rg_nstep_returns_launch_stub(const rg_critic_weights &w, const rg_nstep_returns_io &io, const float *g, void *hip_stream);
static hipError_t launch(const rg_critic_weights &w, const rg_nstep_returns_io &io, const float *g, void *hip_stream) {
    return rg_nstep_returns_launch_stub(w, io, g, hip_stream);
}
#endif

static thread_local char g_nr_err[256] = "";

extern "C" const char *rg_nstep_returns_last_error(void) { return g_nr_err; }
extern "C" int rg_sizeof_nstep_returns_io(void) { return static_cast<int>(sizeof(rg_nstep_returns_io)); }
extern "C" int rg_sizeof_critic_weights(void) { return static_cast<int>(sizeof(rg_critic_weights)); }

extern "C" int rg_nstep_returns(const rg_critic_weights *w, const rg_nstep_returns_io *io, void *hip_stream) {
    const rg::Fail fail{g_nr_err, sizeof(g_nr_err), "rg_nstep_returns"};
    if (!w) return fail(-1, "w", "is NULL");
    if (!io) return fail(-2, "io", "is NULL");
    const rg::NamedPtr required[] = {{io->obs, "io.obs"}, {io->reward, "io.reward"}, {io->terminated, "io.terminated"}, {io->filled, "io.filled"},
                                     {io->returns, "io.returns"}, {io->values, "io.values"}};
    if (const rg::NamedPtr *f = rg::first_null(required)) return fail(-3, f->name, "is NULL");
    if (w->kind != RG_CRITIC_CV && w->kind != RG_CRITIC_CV_NS) return fail(-4, "w.kind", "is neither RG_CRITIC_CV nor RG_CRITIC_CV_NS");
    const bool cv = w->kind == RG_CRITIC_CV;
    // (w1_id last: the first 6 entries are every kind's)
    const rg::NamedPtr weights[] = {{w->w1, "w.w1"}, {w->b1, "w.b1"}, {w->w2, "w.w2"}, {w->b2, "w.b2"}, {w->w3, "w.w3"}, {w->b3, "w.b3"}, {w->w1_id, "w.w1_id"}};
    if (const rg::NamedPtr *f = rg::first_null(weights, cv ? 7 : 6)) return fail(-5, f->name, "is NULL (a weight array of the critic)");
    if (const rg::NamedPtr *f = rg::first_misaligned(weights, 16)) return fail(-6, f->name, "must be 16-byte aligned");
    if (w->hidden_dim != 64 && w->hidden_dim != 128) return fail(-7, "w.hidden_dim", "must be 64 or 128");
    if (w->n_agents != io->n_agents) return fail(-8, "w.n_agents", "differs from io.n_agents");
    if (io->num_episodes < 1) return fail(-10, "io.num_episodes", "must be >= 1");
    if (io->rows < 2) return fail(-11, "io.rows", "must be >= 2");
    if (io->rows > RG_RETURNS_MAX_ROWS) return fail(-25, "io.rows", "is above 4096 (RG_RETURNS_MAX_ROWS: the episode's mask is held on chip)");
    if (io->n_agents < 1 || io->n_agents > RG_MAX_AGENTS) return fail(-12, "io.n_agents", "must be in 1..16 (RG_MAX_AGENTS)");
    if (io->nstep < 1 || io->nstep > RG_NSTEP_MAX) return fail(-13, "io.nstep", "must be in 1..32 (RG_NSTEP_MAX)");
    if (io->obs_dim < 1) return fail(-14, "io.obs_dim", "must be >= 1");
    const int64_t S = static_cast<int64_t>(io->n_agents) * io->obs_dim;
    if (w->state_dim != S) return fail(-9, "w.state_dim", "differs from io.n_agents * io.obs_dim");
    if ((S + 7) / 8 * 8 > 256) return fail(-14, "io.obs_dim", "makes the state (n_agents * obs_dim, padded to a multiple of 8) wider than 256");
    if (io->obs_pitch < io->rows) return fail(-15, "io.obs_pitch", "is below io.rows");
    if (io->flag_pitch < io->rows) return fail(-16, "io.flag_pitch", "is below io.rows");
    if (io->value_pitch < io->rows) return fail(-17, "io.value_pitch", "is below io.rows");
    if (io->out_pitch < io->rows - 1) return fail(-18, "io.out_pitch", "is below io.rows - 1");
    if (!std::isfinite(io->gamma) || io->gamma < 0.0f || io->gamma > 1.0f) return fail(-19, "io.gamma", "must be finite and in [0, 1]");
    if (io->add_value_last_step != 0 && io->add_value_last_step != 1) return fail(-22, "io.add_value_last_step", "must be 0 or 1");
    if (!std::isfinite(io->value_scale)) return fail(-23, "io.value_scale", "must be finite");
    if (!std::isfinite(io->value_shift)) return fail(-23, "io.value_shift", "must be finite");
    if (cv ? w->net_stride != 0 : (w->net_stride < 1 || w->net_stride % 4 != 0))
        return fail(-24, "w.net_stride", cv ? "must be 0 with RG_CRITIC_CV" : "must be a positive multiple of 4 with RG_CRITIC_CV_NS");
    // the element counts of every array: below 2^31 (a row is a product of two 32-bit factors)
    const struct {
        int64_t pitch, row;
        const char *name;
    } counts[] = {{io->obs_pitch, S, "io.num_episodes * obs_pitch * n_agents * obs_dim"},
                  {io->flag_pitch, 1, "io.num_episodes * flag_pitch"},
                  {io->out_pitch, io->n_agents, "io.num_episodes * out_pitch * n_agents"},
                  {io->value_pitch, io->n_agents, "io.num_episodes * value_pitch * n_agents"}};
    for (const auto &c : counts)
        if (!rg::elements_fit(io->num_episodes, c.pitch, c.row)) return fail(-21, c.name, "exceeds 2^31 - 1 elements");
    if (!cv && !rg::elements_fit(w->net_stride, io->n_agents)) return fail(-21, "w.net_stride * n_agents", "exceeds 2^31 - 1 elements");

    if (w->reserved != 0) return fail(-20, "w.reserved", "must be 0");
    if (io->reserved != 0) return fail(-20, "io.reserved", "must be 0");

    float g[RG_NSTEP_MAX + 2] = {0};   // what `gamma ** k * tensor` multiplies by in torch: the power in binary64, rounded once
    for (int k = 0; k <= io->nstep + 1; ++k) g[k] = static_cast<float>(std::pow(static_cast<double>(io->gamma), static_cast<double>(k)));
    const hipError_t err = launch(*w, *io, g, hip_stream);
    if (err != hipSuccess) return fail(-30, "the launch failed:", hipGetErrorString(err));
    return 0;
}
