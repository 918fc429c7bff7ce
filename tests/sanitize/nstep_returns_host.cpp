// nstep_returns_host.cpp -- the host half of csrc/robogym_nstep_returns.hip (compiled with -DRG_NSTEP_RETURNS_HOST_ONLY, for the host
// alone, under ASan + UBSan) in a stand-alone program: its own main and its own launch stub.  It walks every refusal of
// rg_nstep_returns with pointers that are never dereferenced, then lets calls through to the stub and checks what arrives there, the
// discounts included.  Built and run by tests/test_nstep_returns_host_sanitized.py; test infrastructure only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>

#include "../../include/robogym_returns.h"

static int g_launches = 0;
static hipError_t g_stub_result = hipSuccess;
static rg_critic_weights g_seen_w;
static rg_nstep_returns_io g_seen_io;
static float g_seen_g[RG_NSTEP_MAX + 2];
static void *g_seen_stream = nullptr;

hipError_t rg_nstep_returns_launch_stub(const rg_critic_weights &w, const rg_nstep_returns_io &io, const float *g, void *hip_stream) {
    ++g_launches;
    g_seen_w = w;
    g_seen_io = io;
    memcpy(g_seen_g, g, sizeof(g_seen_g));   // (the whole array: a shorter one is the sanitizer's to find)
    g_seen_stream = hip_stream;
    return g_stub_result;
}

template <class T>
static T *fake(uintptr_t a) { return reinterpret_cast<T *>(a); }

static void good(rg_critic_weights &w, rg_nstep_returns_io &io, int kind) {
    memset(&w, 0, sizeof(w));
    memset(&io, 0, sizeof(io));
    const float **p[] = {&w.w1, &w.w1_id, &w.b1, &w.w2, &w.b2, &w.w3, &w.b3};
    for (int i = 0; i < 7; ++i) *p[i] = fake<const float>(0x10000u * (i + 1));
    if (kind == RG_CRITIC_CV_NS) w.w1_id = nullptr;
    w.kind = kind, w.n_agents = 4, w.state_dim = 64, w.hidden_dim = 128, w.net_stride = kind == RG_CRITIC_CV_NS ? 25092 : 0;
    io.obs = fake<const float>(0x1000000), io.reward = fake<const float>(0x1100000), io.terminated = fake<const uint8_t>(0x1200000);
    io.filled = fake<const uint8_t>(0x1300000), io.returns = fake<float>(0x1400000), io.values = fake<float>(0x1500000);
    io.mask = fake<float>(0x1600000);
    io.num_episodes = 3, io.n_agents = 4, io.obs_dim = 16, io.rows = 7, io.nstep = 5, io.add_value_last_step = 1;
    io.obs_pitch = 9, io.flag_pitch = 8, io.out_pitch = 6, io.value_pitch = 7, io.gamma = 0.99f, io.value_scale = 1.0f, io.value_shift = 0.0f;
}

static int g_failed = 0, g_checked = 0;

static void expect(int want, const char *word, int kind, const std::function<void(rg_critic_weights &, rg_nstep_returns_io &)> &change) {
    rg_critic_weights w;
    rg_nstep_returns_io io;
    good(w, io, kind);
    change(w, io);
    const int before = g_launches;
    const int rc = rg_nstep_returns(&w, &io, nullptr);
    const char *msg = rg_nstep_returns_last_error();
    ++g_checked;
    if (rc != want || !strstr(msg, word) || strncmp(msg, "rg_nstep_returns: ", 18) != 0 || g_launches != before) {
        ++g_failed;
        printf("FAIL: wanted %d naming '%s', got %d '%s' (%d launches)\n", want, word, rc, msg, g_launches - before);
    }
}

int main() {
    const int CV = RG_CRITIC_CV, NS = RG_CRITIC_CV_NS;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int big = std::numeric_limits<int>::max(), small = std::numeric_limits<int>::min();
    {
        rg_critic_weights w;
        rg_nstep_returns_io io;
        good(w, io, CV);
        ++g_checked;
        if (rg_nstep_returns(nullptr, &io, nullptr) != -1 || !strstr(rg_nstep_returns_last_error(), "w is NULL")) ++g_failed, printf("FAIL: w NULL\n");
        ++g_checked;
        if (rg_nstep_returns(&w, nullptr, nullptr) != -2 || !strstr(rg_nstep_returns_last_error(), "io is NULL")) ++g_failed, printf("FAIL: io NULL\n");
    }
    for (int kind : {CV, NS}) {
        expect(-3, "io.obs", kind, [](auto &, auto &io) { io.obs = nullptr; });
        expect(-3, "io.reward", kind, [](auto &, auto &io) { io.reward = nullptr; });
        expect(-3, "io.terminated", kind, [](auto &, auto &io) { io.terminated = nullptr; });
        expect(-3, "io.filled", kind, [](auto &, auto &io) { io.filled = nullptr; });
        expect(-3, "io.returns", kind, [](auto &, auto &io) { io.returns = nullptr; });
        expect(-3, "io.values", kind, [](auto &, auto &io) { io.values = nullptr; });
    }
    for (int kind : {-1, 2, 1 << 30, small}) expect(-4, "w.kind", kind, [](auto &, auto &) {});
    const char *names[] = {"w.w1", "w.w1_id", "w.b1", "w.w2", "w.b2", "w.w3", "w.b3"};
    for (int i = 0; i < 7; ++i) {
        auto field = [i](rg_critic_weights &w) -> const float *& {
            const float **p[] = {&w.w1, &w.w1_id, &w.b1, &w.w2, &w.b2, &w.w3, &w.b3};
            return *p[i];
        };
        expect(-5, names[i], CV, [&](auto &w, auto &) { field(w) = nullptr; });
        if (i != 1) expect(-5, names[i], NS, [&](auto &w, auto &) { field(w) = nullptr; });
        for (uintptr_t off : {4u, 8u, 12u})
            for (int kind : {CV, NS}) expect(-6, names[i], kind, [&](auto &w, auto &) { field(w) = fake<const float>(0x700000 + off); });
    }
    for (int h : {0, 32, 96, 256, -128, big}) expect(-7, "w.hidden_dim", CV, [h](auto &w, auto &) { w.hidden_dim = h; });
    expect(-8, "w.n_agents", CV, [](auto &w, auto &) { w.n_agents = 5; });
    expect(-9, "w.state_dim", CV, [](auto &w, auto &) { w.state_dim = 60; });
    expect(-9, "w.state_dim", NS, [](auto &, auto &io) { io.obs_dim = 15; });
    expect(-9, "w.state_dim", CV, [big](auto &, auto &io) { io.obs_dim = big; });   // 4 x (2^31 - 1): no overflow on the way
    for (int v : {0, -3, small}) {
        expect(-10, "io.num_episodes", CV, [v](auto &, auto &io) { io.num_episodes = v; });
        expect(-11, "io.rows", CV, [v](auto &, auto &io) { io.rows = v; });
        expect(-13, "io.nstep", NS, [v](auto &, auto &io) { io.nstep = v; });
        expect(-14, "io.obs_dim", CV, [v](auto &, auto &io) { io.obs_dim = v; });
    }
    expect(-11, "io.rows", CV, [](auto &, auto &io) { io.rows = 1; });
    expect(-13, "io.nstep", CV, [](auto &, auto &io) { io.nstep = 33; });
    expect(-13, "io.nstep", CV, [big](auto &, auto &io) { io.nstep = big; });
    for (int n : {0, -1, 17, big}) expect(-12, "io.n_agents", CV, [n](auto &w, auto &io) { w.n_agents = io.n_agents = n; });
    expect(-14, "wider than 256", CV, [](auto &w, auto &io) { io.obs_dim = 65, w.state_dim = 260; });
    expect(-14, "wider than 256", NS, [](auto &w, auto &io) { w.n_agents = io.n_agents = 1, io.obs_dim = 257, w.state_dim = 257; });
    expect(-15, "io.obs_pitch", CV, [](auto &, auto &io) { io.obs_pitch = 6; });
    expect(-16, "io.flag_pitch", CV, [](auto &, auto &io) { io.flag_pitch = 6; });
    expect(-17, "io.value_pitch", CV, [](auto &, auto &io) { io.value_pitch = 6; });
    expect(-18, "io.out_pitch", CV, [](auto &, auto &io) { io.out_pitch = 5; });
    for (float g : {-0.01f, 1.01f, inf, -inf, nan}) expect(-19, "io.gamma", CV, [g](auto &, auto &io) { io.gamma = g; });
    expect(-20, "io.reserved", CV, [](auto &, auto &io) { io.reserved = 1; });
    expect(-20, "w.reserved", NS, [](auto &w, auto &) { w.reserved = -1; });
    expect(-21, "obs_pitch * n_agents * obs_dim", CV, [](auto &, auto &io) { io.num_episodes = 1 << 22, io.obs_pitch = 8; });
    expect(-21, "io.num_episodes * flag_pitch", CV, [](auto &, auto &io) { io.flag_pitch = 1 << 30; });
    expect(-21, "out_pitch * n_agents", CV, [](auto &, auto &io) { io.num_episodes = 1 << 20, io.out_pitch = 1 << 9; });
    expect(-21, "value_pitch * n_agents", CV, [](auto &, auto &io) { io.num_episodes = 1 << 20, io.value_pitch = 1 << 9; });
    expect(-21, "w.net_stride * n_agents", NS, [](auto &w, auto &) { w.net_stride = 1 << 29; });
    expect(-21, "exceeds 2^31 - 1", CV, [big](auto &, auto &io) { io.num_episodes = big; });
    expect(-21, "exceeds 2^31 - 1", CV, [big](auto &, auto &io) {   // every factor as large as an int gets: no overflow on the way
        io.num_episodes = io.obs_pitch = io.flag_pitch = io.out_pitch = io.value_pitch = big;
    });
    for (int v : {-1, 2, big, small}) expect(-22, "io.add_value_last_step", CV, [v](auto &, auto &io) { io.add_value_last_step = v; });
    for (float v : {inf, -inf, nan}) {
        expect(-23, "io.value_scale", CV, [v](auto &, auto &io) { io.value_scale = v; });
        expect(-23, "io.value_shift", NS, [v](auto &, auto &io) { io.value_shift = v; });
    }
    for (int v : {4, -4, 1, big}) expect(-24, "w.net_stride", CV, [v](auto &w, auto &) { w.net_stride = v; });
    for (int v : {0, -4, 25090, small, big}) expect(-24, "w.net_stride", NS, [v](auto &w, auto &) { w.net_stride = v; });
    expect(-25, "io.rows", CV, [](auto &, auto &io) { io.rows = io.obs_pitch = io.flag_pitch = io.value_pitch = 4097, io.out_pitch = 4096; });
    expect(-25, "io.rows", CV, [big](auto &, auto &io) { io.rows = big; });

    // calls that pass every check arrive at the launch exactly as given, with the discounts (float) pow((double) gamma, k)
    int stream_tag = 0;
    for (int kind : {CV, NS}) {
        rg_critic_weights w;
        rg_nstep_returns_io io;
        good(w, io, kind);
        if (kind == NS) io.mask = nullptr, io.add_value_last_step = 0, w.hidden_dim = 64;
        const int before = g_launches;
        const int rc = rg_nstep_returns(&w, &io, &stream_tag);
        ++g_checked;
        bool ok = rc == 0 && g_launches == before + 1 && memcmp(&g_seen_w, &w, sizeof(w)) == 0 && memcmp(&g_seen_io, &io, sizeof(io)) == 0 &&
                  g_seen_stream == &stream_tag;
        for (int k = 0; k < RG_NSTEP_MAX + 2; ++k) {
            const float want = k <= io.nstep + 1 ? static_cast<float>(std::pow(static_cast<double>(0.99f), static_cast<double>(k))) : 0.0f;
            ok = ok && memcmp(&g_seen_g[k], &want, sizeof(float)) == 0;
        }
        if (!ok) ++g_failed, printf("FAIL: a good call of kind %d returned %d '%s'\n", kind, rc, rg_nstep_returns_last_error());
    }
    {   // the edges of what is accepted: gamma 0 and 1, the widest state, the most agents, steps and rows, rows = 2
        rg_critic_weights w;
        rg_nstep_returns_io io;
        good(w, io, CV);
        io.gamma = 0.0f, io.n_agents = w.n_agents = 16, io.obs_dim = 16, w.state_dim = 256, io.nstep = 32, io.rows = 2, io.out_pitch = 1;
        io.value_scale = -1.7f, io.value_shift = 1e30f;
        ++g_checked;
        if (rg_nstep_returns(&w, &io, nullptr) != 0 || g_seen_g[0] != 1.0f || g_seen_g[1] != 0.0f || g_seen_g[33] != 0.0f)
            ++g_failed, printf("FAIL: the widest call: %s\n", rg_nstep_returns_last_error());
        io.gamma = 1.0f, io.rows = io.obs_pitch = io.flag_pitch = io.value_pitch = 4096, io.out_pitch = 4095;
        ++g_checked;
        if (rg_nstep_returns(&w, &io, nullptr) != 0 || g_seen_g[33] != 1.0f) ++g_failed, printf("FAIL: gamma = 1: %s\n", rg_nstep_returns_last_error());
    }
    {   // a failed launch is -30 and says what the runtime says
        rg_critic_weights w;
        rg_nstep_returns_io io;
        good(w, io, NS);
        g_stub_result = hipErrorInvalidValue;
        const int rc = rg_nstep_returns(&w, &io, nullptr);
        g_stub_result = hipSuccess;
        ++g_checked;
        if (rc != -30 || !strstr(rg_nstep_returns_last_error(), "the launch failed")) ++g_failed, printf("FAIL: launch failure gave %d '%s'\n", rc, rg_nstep_returns_last_error());
    }
    if (rg_sizeof_critic_weights() != 80 || rg_sizeof_nstep_returns_io() != 112) ++g_failed, printf("FAIL: struct sizes\n");
    printf("nstep_returns_host: %d checks, %d failed, %d launches reached the stub\n", g_checked, g_failed, g_launches);
    return g_failed ? 1 : 0;
}
