// robogym_gru_scan.hip -- rg_gru_scan_forward / rg_gru_scan_backward: the GRU recurrence of a recurrent actor over a whole episode
// batch, forward and backward, one launch each (include/robogym_learn.h; the rule and the kernels: gru_scan.h).
//
// The host entries are handle-free and keep their own last-error text (as robogym_nstep_returns.hip does): every argument check
// comes before the first HIP call, so the refusals can be exercised without a device.
#include <hip/hip_runtime.h>

#include <cstring>

#include "host_checks.h"

#ifndef RG_GRU_SCAN_HOST_ONLY   // (the sanitized host program, tests/sanitize/gru_scan_host.cpp: the argument checks without the kernels)
#include "gru_scan.h"

// every argument validated by check() below
static hipError_t launch(const rg_gru_scan_weights &w, const rg_gru_scan_io &io, int backward, int tiles, void *hip_stream) {
    rg::GsArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.w = w;
    ga.io = io;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const dim3 grid(tiles), block(2 * w.hidden_dim);
    if (w.hidden_dim == 128) {
        if (backward) hipLaunchKernelGGL(rg::gru_scan_backward_kernel<128>, grid, block, 0, stream, ga);
        else hipLaunchKernelGGL(rg::gru_scan_forward_kernel<128>, grid, block, 0, stream, ga);
    } else {
        if (backward) hipLaunchKernelGGL(rg::gru_scan_backward_kernel<64>, grid, block, 0, stream, ga);
        else hipLaunchKernelGGL(rg::gru_scan_forward_kernel<64>, grid, block, 0, stream, ga);
    }
    return hipGetLastError();
}
#else
#include "../../include/robogym_learn.h"
// the program's own; tiles: the workgroups of the launch
hipError_t rg_gru_scan_launch_stub(const rg_gru_scan_weights &w, const rg_gru_scan_io &io, int backward, int tiles, void *hip_stream);
static hipError_t launch(const rg_gru_scan_weights &w, const rg_gru_scan_io &io, int backward, int tiles, void *hip_stream) {
    return rg_gru_scan_launch_stub(w, io, backward, tiles, hip_stream);
}
#endif

static thread_local char g_gs_err[256] = "";

extern "C" const char *rg_gru_scan_last_error(void) { return g_gs_err; }
extern "C" int rg_sizeof_gru_scan_weights(void) { return static_cast<int>(sizeof(rg_gru_scan_weights)); }
extern "C" int rg_sizeof_gru_scan_io(void) { return static_cast<int>(sizeof(rg_gru_scan_io)); }

static int scan(const char *entry, int backward, const rg_gru_scan_weights *w, const rg_gru_scan_io *io, void *hip_stream) {
    const rg::Fail fail{g_gs_err, sizeof(g_gs_err), entry};
    if (!w) return fail(-1, "w", "is NULL");
    if (!io) return fail(-2, "io", "is NULL");
    // what this launch reads and writes: the required arrays first
    const rg::NamedPtr fwd[] = {{io->gi, "io.gi", 4}, {io->h, "io.h", 4}, {io->hidden_in, "io.hidden_in", 4}, {io->gates, "io.gates", 4},
                                {io->hidden_out, "io.hidden_out", 4}, {w->w_hh, "w.w_hh", 16}, {w->b_hh, "w.b_hh", 16}, {w->w_hh_t, "w.w_hh_t", 16}};
    const rg::NamedPtr bwd[] = {{io->h, "io.h", 4}, {io->dh_ext, "io.dh_ext", 4}, {io->dgi, "io.dgi", 4}, {io->dghn, "io.dghn", 4},
                                {io->gates, "io.gates", 4}, {io->hidden_in, "io.hidden_in", 4}, {io->d_hidden_out, "io.d_hidden_out", 4},
                                {io->d_hidden_in, "io.d_hidden_in", 4}, {w->w_hh, "w.w_hh", 16}};
    if (const rg::NamedPtr *f = backward ? rg::first_null(bwd, 4) : rg::first_null(fwd, 2)) return fail(-3, f->name, "is NULL");
    if (!w->w_hh) return fail(-4, "w.w_hh", "is NULL");
    if (!backward && !w->b_hh) return fail(-4, "w.b_hh", "is NULL");
    if (const rg::NamedPtr *f = backward ? rg::first_misaligned(bwd) : rg::first_misaligned(fwd))
        return fail(-5, f->name, f->align == 16 ? "must be 16-byte aligned" : "must be 4-byte aligned");
    if (w->hidden_dim != 64 && w->hidden_dim != 128) return fail(-6, "w.hidden_dim", "must be 64 or 128");
    if (io->n_agents < 1 || io->n_agents > RG_MAX_AGENTS) return fail(-8, "io.n_agents", "must be in 1..16 (RG_MAX_AGENTS)");
    if (w->n_sets != 1 && w->n_sets != io->n_agents) return fail(-7, "w.n_sets", "must be 1 or io.n_agents");
    if (io->num_episodes < 1) return fail(-9, "io.num_episodes", "must be >= 1");
    if (io->rows < 1) return fail(-10, "io.rows", "must be >= 1");
    if (io->rows > RG_GRU_SCAN_MAX_ROWS) return fail(-11, "io.rows", "is above 4096 (RG_GRU_SCAN_MAX_ROWS)");
    if (!backward && io->gi_pitch < io->rows) return fail(-12, "io.gi_pitch", "is below io.rows");
    if (io->save_pitch < io->rows) return fail(-13, "io.save_pitch", "is below io.rows");
    if (backward && io->grad_pitch < io->rows) return fail(-14, "io.grad_pitch", "is below io.rows");
    if (backward && !io->gates) return fail(-15, "io.gates", "is NULL: the backward launch needs the gates the forward launch saved");
    if (w->reserved[0] != 0 || w->reserved[1] != 0) return fail(-20, "w.reserved", "must be 0");
    if (io->reserved[0] != 0 || io->reserved[1] != 0) return fail(-20, "io.reserved", "must be 0");
    // the element counts of every array of this launch: below 2^31 (the kernels index with 32-bit row numbers)
    const int64_t H = w->hidden_dim, B = io->num_episodes, N = io->n_agents;
    if (!backward && !rg::elements_fit(B, io->gi_pitch, N, 3 * H)) return fail(-21, "io.num_episodes * gi_pitch * n_agents * 3 hidden_dim", "exceeds 2^31 - 1 elements");
    if (!rg::elements_fit(B, io->save_pitch, N, 4 * H)) return fail(-21, "io.num_episodes * save_pitch * n_agents * 4 hidden_dim", "exceeds 2^31 - 1 elements");
    if (backward && !rg::elements_fit(B, io->grad_pitch, N, 3 * H)) return fail(-21, "io.num_episodes * grad_pitch * n_agents * 3 hidden_dim", "exceeds 2^31 - 1 elements");

    // one workgroup per tile of 32 flat rows: flat with shared weights, 32 episodes of one agent with one set per agent
    const int64_t tiles = w->n_sets == 1 ? (B * N + 31) / 32 : N * ((B + 31) / 32);
    const hipError_t err = launch(*w, *io, backward, static_cast<int>(tiles), hip_stream);
    if (err != hipSuccess) return fail(-30, "the launch failed:", hipGetErrorString(err));
    return 0;
}

extern "C" int rg_gru_scan_forward(const rg_gru_scan_weights *w, const rg_gru_scan_io *io, void *hip_stream) {
    return scan("rg_gru_scan_forward", 0, w, io, hip_stream);
}
extern "C" int rg_gru_scan_backward(const rg_gru_scan_weights *w, const rg_gru_scan_io *io, void *hip_stream) {
    return scan("rg_gru_scan_backward", 1, w, io, hip_stream);
}
