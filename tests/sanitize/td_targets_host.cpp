// td_targets_host.cpp -- the host half of csrc/robogym_td_targets.hip (compiled with -DRG_TD_TARGETS_HOST_ONLY, for the host alone,
// under ASan + UBSan) in a stand-alone program: its own main and its own launch stub.  It walks every refusal of rg_td_targets with
// pointers that are never dereferenced, then lets calls through to the stub and checks what arrives there.  Built and run by
// tests/test_td_targets_host_sanitized.py; test infrastructure only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>

#include "../../include/robogym.h"

static int g_launches = 0;
static hipError_t g_stub_result = hipSuccess;
static rg_mixer_weights g_seen_m;
static rg_td_targets_io g_seen_io;
static void *g_seen_stream = nullptr;

hipError_t rg_td_targets_launch_stub(const rg_mixer_weights &m, const rg_td_targets_io &io, void *hip_stream) {
    ++g_launches;
    g_seen_m = m;
    g_seen_io = io;
    g_seen_stream = hip_stream;
    return g_stub_result;
}

template <class T>
static T *fake(uintptr_t a) { return reinterpret_cast<T *>(a); }

static void good(rg_mixer_weights &m, rg_td_targets_io &io, int kind) {
    memset(&m, 0, sizeof(m));
    memset(&io, 0, sizeof(io));
    const float **w[] = {&m.w_in, &m.b_in, &m.w_w1, &m.b_w1, &m.w_wf, &m.b_wf, &m.w_v, &m.b_v};
    for (int i = 0; i < 8; ++i) *w[i] = fake<const float>(0x10000u * (i + 1));
    m.kind = kind, m.n_agents = 4, m.state_dim = 64, m.embed_dim = 32, m.hypernet_embed = 64;
    io.qt = fake<const float>(0x1000000), io.sel = fake<const int32_t>(0x1100000), io.obs = fake<const float>(0x1200000);
    io.reward = fake<const float>(0x1300000), io.terminated = fake<const uint8_t>(0x1400000), io.filled = fake<const uint8_t>(0x1500000);
    io.targets = fake<float>(0x1600000), io.mask = fake<float>(0x1700000), io.agent_q = fake<float>(0x1800000);
    io.num_episodes = 3, io.n_agents = 4, io.obs_dim = 16, io.n_actions = 5, io.rows = 7;
    io.q_pitch = 8, io.obs_pitch = 9, io.flag_pitch = 7, io.out_pitch = 6, io.gamma = 0.99f;
}

static int g_failed = 0, g_checked = 0;

static void expect(int want, const char *word, int kind, const std::function<void(rg_mixer_weights &, rg_td_targets_io &)> &change) {
    rg_mixer_weights m;
    rg_td_targets_io io;
    good(m, io, kind);
    change(m, io);
    const int before = g_launches;
    const int rc = rg_td_targets(&m, &io, nullptr);
    const char *msg = rg_td_targets_last_error();
    ++g_checked;
    if (rc != want || !strstr(msg, word) || strncmp(msg, "rg_td_targets: ", 15) != 0 || g_launches != before) {
        ++g_failed;
        printf("FAIL: wanted %d naming '%s', got %d '%s' (%d launches)\n", want, word, rc, msg, g_launches - before);
    }
}

int main() {
    const int Q = RG_MIXER_QMIX, V = RG_MIXER_VDN, NONE = RG_MIXER_NONE;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    {
        rg_mixer_weights m;
        rg_td_targets_io io;
        good(m, io, Q);
        ++g_checked;
        if (rg_td_targets(nullptr, &io, nullptr) != -1 || !strstr(rg_td_targets_last_error(), "m is NULL")) ++g_failed, printf("FAIL: m NULL\n");
        ++g_checked;
        if (rg_td_targets(&m, nullptr, nullptr) != -2 || !strstr(rg_td_targets_last_error(), "io is NULL")) ++g_failed, printf("FAIL: io NULL\n");
    }
    for (int kind : {NONE, V, Q}) {
        expect(-3, "io.qt", kind, [](auto &, auto &io) { io.qt = nullptr; });
        expect(-3, "io.reward", kind, [](auto &, auto &io) { io.reward = nullptr; });
        expect(-3, "io.terminated", kind, [](auto &, auto &io) { io.terminated = nullptr; });
        expect(-3, "io.filled", kind, [](auto &, auto &io) { io.filled = nullptr; });
        expect(-3, "io.targets", kind, [](auto &, auto &io) { io.targets = nullptr; });
    }
    expect(-3, "io.obs", Q, [](auto &, auto &io) { io.obs = nullptr; });
    for (int kind : {-1, 3, 1 << 30}) expect(-4, "m.kind", kind, [](auto &, auto &) {});
    const char *names[] = {"m.w_in", "m.b_in", "m.w_w1", "m.b_w1", "m.w_wf", "m.b_wf", "m.w_v", "m.b_v"};
    for (int i = 0; i < 8; ++i) {
        auto field = [i](rg_mixer_weights &m) -> const float *& {
            const float **w[] = {&m.w_in, &m.b_in, &m.w_w1, &m.b_w1, &m.w_wf, &m.b_wf, &m.w_v, &m.b_v};
            return *w[i];
        };
        expect(-5, names[i], Q, [&](auto &m, auto &) { field(m) = nullptr; });
        for (uintptr_t off : {4u, 8u, 12u}) expect(-6, names[i], Q, [&](auto &m, auto &) { field(m) = fake<const float>(0x700000 + off); });
    }
    for (int e : {0, 16, 64}) expect(-7, "m.embed_dim", Q, [e](auto &m, auto &) { m.embed_dim = e; });
    for (int e : {0, 32, 128}) expect(-7, "m.hypernet_embed", Q, [e](auto &m, auto &) { m.hypernet_embed = e; });
    expect(-8, "m.n_agents", V, [](auto &m, auto &) { m.n_agents = 5; });
    expect(-9, "m.state_dim", Q, [](auto &m, auto &) { m.state_dim = 60; });
    expect(-9, "m.state_dim", Q, [](auto &, auto &io) { io.obs_dim = 15; });
    for (int v : {0, -3, std::numeric_limits<int>::min()}) {
        expect(-10, "io.num_episodes", V, [v](auto &, auto &io) { io.num_episodes = v; });
        expect(-11, "io.rows", V, [v](auto &, auto &io) { io.rows = v; });
        expect(-13, "io.n_actions", V, [v](auto &, auto &io) { io.n_actions = v; });
        expect(-14, "io.obs_dim", V, [v](auto &, auto &io) { io.obs_dim = v; });
    }
    expect(-11, "io.rows", Q, [](auto &, auto &io) { io.rows = 1; });
    expect(-13, "io.n_actions", Q, [](auto &, auto &io) { io.n_actions = 33; });
    for (int n : {0, -1, 17, std::numeric_limits<int>::max()}) expect(-12, "io.n_agents", V, [n](auto &m, auto &io) { m.n_agents = io.n_agents = n; });
    expect(-14, "wider than 256", Q, [](auto &m, auto &io) { io.obs_dim = 65, m.state_dim = 260; });
    expect(-15, "io.obs_pitch", Q, [](auto &, auto &io) { io.obs_pitch = 6; });
    expect(-16, "io.q_pitch", Q, [](auto &, auto &io) { io.q_pitch = 6; });
    expect(-17, "io.flag_pitch", Q, [](auto &, auto &io) { io.flag_pitch = 6; });
    expect(-18, "io.out_pitch", Q, [](auto &, auto &io) { io.out_pitch = 5; });
    for (float g : {-0.01f, 1.01f, inf, -inf, nan}) expect(-19, "io.gamma", Q, [g](auto &, auto &io) { io.gamma = g; });
    expect(-20, "io.reserved", Q, [](auto &, auto &io) { io.reserved = 1; });
    expect(-20, "m.reserved", Q, [](auto &m, auto &) { m.reserved = -1; });
    const int big = std::numeric_limits<int>::max();
    expect(-21, "q_pitch * n_agents * n_actions", Q, [](auto &, auto &io) { io.num_episodes = 1 << 24, io.q_pitch = io.obs_pitch = 7, io.out_pitch = 6; });
    expect(-21, "obs_pitch * n_agents * obs_dim", V, [](auto &, auto &io) { io.n_actions = 1, io.num_episodes = 1 << 21, io.obs_pitch = 16; });
    expect(-21, "io.num_episodes * flag_pitch", V, [](auto &, auto &io) { io.flag_pitch = 1 << 30; });
    expect(-21, "exceeds 2^31 - 1", V, [big](auto &, auto &io) { io.num_episodes = big; });
    expect(-21, "exceeds 2^31 - 1", V, [big](auto &, auto &io) {   // every factor as large as an int gets: no overflow on the way
        io.num_episodes = io.rows = io.q_pitch = io.obs_pitch = io.flag_pitch = io.out_pitch = big;
        io.obs_dim = big, io.n_actions = 32;
    });
    expect(-21, "out_pitch * n_agents", V, [](auto &m, auto &io) {
        io.n_actions = io.obs_dim = 1, io.num_episodes = 1 << 23, io.out_pitch = 1 << 6, m.n_agents = io.n_agents = 16;
        io.q_pitch = io.obs_pitch = io.flag_pitch = 7;
    });

    // calls that pass every check arrive at the launch exactly as given
    int stream_tag = 0;
    for (int kind : {NONE, V, Q}) {
        rg_mixer_weights m;
        rg_td_targets_io io;
        good(m, io, kind);
        io.sel = nullptr, io.mask = nullptr, io.agent_q = nullptr;
        if (kind != Q) {
            memset(&m, 0, sizeof(m));
            m.kind = kind, m.n_agents = 4;
            io.obs = nullptr;
        }
        const int before = g_launches;
        const int rc = rg_td_targets(&m, &io, &stream_tag);
        ++g_checked;
        if (rc != 0 || g_launches != before + 1 || memcmp(&g_seen_m, &m, sizeof(m)) != 0 || memcmp(&g_seen_io, &io, sizeof(io)) != 0 ||
            g_seen_stream != &stream_tag) {
            ++g_failed;
            printf("FAIL: a good call of kind %d returned %d '%s'\n", kind, rc, rg_td_targets_last_error());
        }
    }
    {   // the edges of what is accepted: gamma 0 and 1, the widest state, the most agents and actions, rows = 2
        rg_mixer_weights m;
        rg_td_targets_io io;
        good(m, io, Q);
        io.gamma = 0.0f, io.n_agents = m.n_agents = 16, io.obs_dim = 16, m.state_dim = 256, io.n_actions = 32, io.rows = 2, io.out_pitch = 1;
        ++g_checked;
        if (rg_td_targets(&m, &io, nullptr) != 0) ++g_failed, printf("FAIL: the widest call: %s\n", rg_td_targets_last_error());
        io.gamma = 1.0f;
        ++g_checked;
        if (rg_td_targets(&m, &io, nullptr) != 0) ++g_failed, printf("FAIL: gamma = 1: %s\n", rg_td_targets_last_error());
    }
    {   // a failed launch is -30 and says what the runtime says
        rg_mixer_weights m;
        rg_td_targets_io io;
        good(m, io, V);
        g_stub_result = hipErrorInvalidValue;
        const int rc = rg_td_targets(&m, &io, nullptr);
        g_stub_result = hipSuccess;
        ++g_checked;
        if (rc != -30 || !strstr(rg_td_targets_last_error(), "the launch failed")) ++g_failed, printf("FAIL: launch failure gave %d '%s'\n", rc, rg_td_targets_last_error());
    }
    if (rg_sizeof_mixer_weights() != 88 || rg_sizeof_td_targets_io() != 120) ++g_failed, printf("FAIL: struct sizes\n");
    printf("td_targets_host: %d checks, %d failed, %d launches reached the stub\n", g_checked, g_failed, g_launches);
    return g_failed ? 1 : 0;
}
