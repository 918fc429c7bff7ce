// mixer_host.cpp -- the host half of csrc/robogym_mixer_grad.hip (compiled with -DRG_MIXER_GRAD_HOST_ONLY, for the host alone, under
// ASan + UBSan) in a stand-alone program: its own main and its own launch stub.  It walks every refusal of rg_mixer_forward and
// rg_mixer_backward with pointers that are never dereferenced, then lets calls through to the stub and checks what arrives there,
// the number of workgroups included.  Built and run by tests/test_mixer_host_sanitized.py; test infrastructure only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>

#include "../../include/robogym_learn.h"

static int g_launches = 0;
static hipError_t g_stub_result = hipSuccess;
static rg_mixer_grad_weights g_seen_w;
static rg_mixer_grad_io g_seen_io;
static int g_seen_backward = -1, g_seen_tiles = -1;
static void *g_seen_stream = nullptr;

hipError_t rg_mixer_grad_launch_stub(const rg_mixer_grad_weights &w, const rg_mixer_grad_io &io, int backward, int tiles, void *hip_stream) {
    ++g_launches;
    g_seen_w = w;
    g_seen_io = io;
    g_seen_backward = backward, g_seen_tiles = tiles;
    g_seen_stream = hip_stream;
    return g_stub_result;
}

template <class T>
static T *fake(uintptr_t a) { return reinterpret_cast<T *>(a); }

// N = 4, D = 16, A = 5, B = 3 episodes of 7 rows
static void good(rg_mixer_grad_weights &w, rg_mixer_grad_io &io, int kind) {
    memset(&w, 0, sizeof(w));
    memset(&io, 0, sizeof(io));
    const float **weights[] = {&w.m.w_in, &w.m.b_in, &w.m.w_w1, &w.m.b_w1, &w.m.w_wf, &w.m.b_wf, &w.m.w_v, &w.m.b_v, &w.w1b, &w.wfb};
    for (int i = 0; i < 10; ++i) *weights[i] = fake<const float>(0x10000 * (i + 1));
    w.m.kind = kind, w.m.n_agents = 4, w.m.state_dim = 64, w.m.embed_dim = 32, w.m.hypernet_embed = 64;
    io.q = fake<const float>(0x1000000), io.actions = fake<const int32_t>(0x1100000), io.obs = fake<const float>(0x1200000);
    io.mask = fake<const float>(0x1300000), io.mixed = fake<float>(0x1400000), io.d_mixed = fake<const float>(0x1500000);
    io.d_q = fake<float>(0x1600000), io.d_pre = fake<float>(0x1700000), io.d_p2 = fake<float>(0x1800000), io.g = fake<float>(0x1900000);
    io.num_episodes = 3, io.n_agents = 4, io.obs_dim = 16, io.n_actions = 5, io.rows = 7;
    io.q_pitch = 8, io.obs_pitch = 9, io.out_pitch = 6, io.aux_pitch = 7;
}

static int g_failed = 0, g_checked = 0;
typedef int (*entry_t)(const rg_mixer_grad_weights *, const rg_mixer_grad_io *, void *);
static const entry_t ENTRY[2] = {rg_mixer_forward, rg_mixer_backward};
static const char *PREFIX[2] = {"rg_mixer_forward: ", "rg_mixer_backward: "};
typedef std::function<void(rg_mixer_grad_weights &, rg_mixer_grad_io &)> change_t;

// `which`: 0 forward, 1 backward, 2 both; `kinds`: a bit per mixer kind
static void expect(int which, int kinds, int want, const char *word, const change_t &change) {
    for (int b = 0; b < 2; ++b)
        for (int kind = 0; kind < 3; ++kind) {
            if ((which != 2 && which != b) || !(kinds & (1 << kind))) continue;
            rg_mixer_grad_weights w;
            rg_mixer_grad_io io;
            good(w, io, kind);
            change(w, io);
            const int before = g_launches;
            const int rc = ENTRY[b](&w, &io, nullptr);
            const char *msg = rg_mixer_grad_last_error();
            ++g_checked;
            if (rc != want || !strstr(msg, word) || strncmp(msg, PREFIX[b], strlen(PREFIX[b])) != 0 || g_launches != before) {
                ++g_failed;
                printf("FAIL (%skind %d): wanted %d naming '%s', got %d '%s' (%d launches)\n", PREFIX[b], kind, want, word, rc, msg, g_launches - before);
            }
        }
}

int main() {
    const int big = std::numeric_limits<int>::max(), small = std::numeric_limits<int>::min();
    const int ALL = 7, QMIX = 4, PLAIN = 3;
    for (int b = 0; b < 2; ++b) {
        rg_mixer_grad_weights w;
        rg_mixer_grad_io io;
        good(w, io, 2);
        ++g_checked;
        if (ENTRY[b](nullptr, &io, nullptr) != -1 || !strstr(rg_mixer_grad_last_error(), "w is NULL")) ++g_failed, printf("FAIL: w NULL\n");
        ++g_checked;
        if (ENTRY[b](&w, nullptr, nullptr) != -2 || !strstr(rg_mixer_grad_last_error(), "io is NULL")) ++g_failed, printf("FAIL: io NULL\n");
    }
    expect(0, ALL, -3, "io.q is NULL", [](auto &, auto &io) { io.q = nullptr; });
    expect(1, QMIX, -3, "io.q is NULL", [](auto &, auto &io) { io.q = nullptr; });
    expect(2, ALL, -3, "io.actions is NULL", [](auto &, auto &io) { io.actions = nullptr; });
    expect(2, ALL, -3, "io.mask is NULL", [](auto &, auto &io) { io.mask = nullptr; });
    expect(0, ALL, -3, "io.mixed is NULL", [](auto &, auto &io) { io.mixed = nullptr; });
    expect(1, ALL, -3, "io.d_mixed is NULL", [](auto &, auto &io) { io.d_mixed = nullptr; });
    expect(1, ALL, -3, "io.d_q is NULL", [](auto &, auto &io) { io.d_q = nullptr; });
    expect(2, QMIX, -3, "io.obs is NULL", [](auto &, auto &io) { io.obs = nullptr; });
    expect(1, QMIX, -3, "io.d_pre is NULL", [](auto &, auto &io) { io.d_pre = nullptr; });
    expect(1, QMIX, -3, "io.d_p2 is NULL", [](auto &, auto &io) { io.d_p2 = nullptr; });
    expect(1, QMIX, -3, "io.g is NULL", [](auto &, auto &io) { io.g = nullptr; });
    for (int k : {-1, 3, 99, big, small}) expect(2, 1, -4, "w.m.kind", [k](auto &w, auto &) { w.m.kind = k; });
    const char *names[] = {"w.m.w_in", "w.m.b_in", "w.m.w_w1", "w.m.b_w1", "w.m.w_wf", "w.m.b_wf", "w.m.w_v", "w.m.b_v", "w.w1b", "w.wfb"};
    for (int i = 0; i < 10; ++i) {
        auto set = [i](rg_mixer_grad_weights &w, const float *p) {
            const float **weights[] = {&w.m.w_in, &w.m.b_in, &w.m.w_w1, &w.m.b_w1, &w.m.w_wf, &w.m.b_wf, &w.m.w_v, &w.m.b_v, &w.w1b, &w.wfb};
            *weights[i] = p;
        };
        char null_word[64], align_word[64];
        snprintf(null_word, sizeof(null_word), "%s is NULL", names[i]);
        snprintf(align_word, sizeof(align_word), "%s must be 16-byte aligned", names[i]);
        expect(i < 8 ? 2 : 1, QMIX, -5, null_word, [&](auto &w, auto &) { set(w, nullptr); });
        for (uintptr_t off : {4u, 8u, 12u}) expect(2, QMIX, -6, align_word, [&](auto &w, auto &) { set(w, fake<const float>(0x700000 + off)); });
    }
    for (uintptr_t off : {1u, 2u, 3u}) {
        expect(0, ALL, -6, "io.q must be 4-byte aligned", [off](auto &, auto &io) { io.q = fake<const float>(0x700000 + off); });
        expect(2, ALL, -6, "io.actions must be 4-byte aligned", [off](auto &, auto &io) { io.actions = fake<const int32_t>(0x700000 + off); });
        expect(2, ALL, -6, "io.mask must be 4-byte aligned", [off](auto &, auto &io) { io.mask = fake<const float>(0x700000 + off); });
        expect(0, ALL, -6, "io.mixed must be 4-byte aligned", [off](auto &, auto &io) { io.mixed = fake<float>(0x700000 + off); });
        expect(1, ALL, -6, "io.d_mixed must be 4-byte aligned", [off](auto &, auto &io) { io.d_mixed = fake<const float>(0x700000 + off); });
        expect(1, ALL, -6, "io.d_q must be 4-byte aligned", [off](auto &, auto &io) { io.d_q = fake<float>(0x700000 + off); });
        expect(1, ALL, -6, "io.g must be 4-byte aligned", [off](auto &, auto &io) { io.g = fake<float>(0x700000 + off); });
    }
    for (int e : {0, 16, 64, big, small}) expect(2, QMIX, -7, "w.m.embed_dim", [e](auto &w, auto &) { w.m.embed_dim = e; });
    for (int e : {0, 32, 128, big, small}) expect(2, QMIX, -7, "w.m.hypernet_embed", [e](auto &w, auto &) { w.m.hypernet_embed = e; });
    expect(2, ALL, -8, "w.m.n_agents", [](auto &w, auto &) { w.m.n_agents = 5; });
    expect(2, QMIX, -9, "w.m.state_dim", [](auto &w, auto &) { w.m.state_dim = 60; });
    expect(2, QMIX, -9, "w.m.state_dim", [](auto &, auto &io) { io.obs_dim = 15; });
    for (int v : {0, -3, small}) {
        expect(2, ALL, -10, "io.num_episodes", [v](auto &, auto &io) { io.num_episodes = v; });
        expect(2, ALL, -11, "io.rows", [v](auto &, auto &io) { io.rows = v; });
        expect(2, ALL, -13, "io.n_actions", [v](auto &, auto &io) { io.n_actions = v; });
        expect(2, QMIX, -14, "io.obs_dim", [v](auto &, auto &io) { io.obs_dim = v; });
    }
    expect(2, ALL, -11, "io.rows", [](auto &, auto &io) { io.rows = 1; });
    expect(2, ALL, -13, "io.n_actions", [](auto &, auto &io) { io.n_actions = 33; });
    for (int n : {0, -1, 17, big, small}) expect(2, ALL, -12, "io.n_agents", [n](auto &w, auto &io) { w.m.n_agents = io.n_agents = n; });
    expect(2, QMIX, -14, "wider than 256", [](auto &w, auto &io) { io.obs_dim = 65, w.m.state_dim = 260; });
    for (int v : {6, 0, -1, small}) {
        expect(2, QMIX, -15, "io.obs_pitch", [v](auto &, auto &io) { io.obs_pitch = v; });
        expect(2, ALL, -16, "io.q_pitch", [v](auto &, auto &io) { io.q_pitch = v; });
        expect(1, QMIX, -18, "io.aux_pitch", [v](auto &, auto &io) { io.aux_pitch = v; });
    }
    for (int v : {5, 0, -1, small}) expect(2, ALL, -17, "io.out_pitch", [v](auto &, auto &io) { io.out_pitch = v; });
    expect(2, ALL, -20, "w.m.reserved", [](auto &w, auto &) { w.m.reserved = 2; });
    expect(2, ALL, -20, "io.reserved", [small](auto &, auto &io) { io.reserved = small; });
    expect(2, ALL, -21, "q_pitch * n_agents * n_actions", [](auto &, auto &io) { io.num_episodes = 1 << 24, io.q_pitch = 7; });        // 2^24 x 7 x 20
    expect(2, QMIX, -21, "obs_pitch * n_agents * obs_dim", [](auto &, auto &io) { io.n_actions = 1, io.num_episodes = 1 << 21, io.obs_pitch = 16; });   // 2^25 x 64
    expect(2, PLAIN, -21, "out_pitch * n_agents", [](auto &, auto &io) { io.n_actions = 1, io.num_episodes = 1 << 20, io.out_pitch = 1 << 10; });
    expect(1, QMIX, -21, "aux_pitch * (32 n_agents + 32)", [](auto &, auto &io) { io.n_actions = 1, io.obs_dim = 16, io.num_episodes = 1 << 16, io.aux_pitch = 1 << 8; });
    expect(2, ALL, -21, "exceeds 2^31 - 1", [big](auto &, auto &io) { io.num_episodes = io.rows = io.q_pitch = io.obs_pitch = io.out_pitch = io.aux_pitch = big; });

    // none / vdn read neither the weights nor obs nor the per-row arrays: a call without them passes, as given, to the launch
    int stream_tag = 0;
    struct Shape {
        int kind, B, rows, N, tiles;
    };
    const Shape shapes[] = {{2, 3, 7, 4, 1}, {2, 1, 2, 1, 1}, {2, 32, 2, 5, 1}, {2, 33, 2, 8, 2}, {2, 33, 14, 16, 14}, {2, 4096, 85, 4, 10752},
                            {1, 3, 7, 4, 1}, {0, 33, 14, 16, 2}, {1, 4096, 85, 4, 1344}, {0, 256, 2, 2, 1}, {1, 257, 2, 2, 2}};
    for (const Shape &s : shapes)
        for (int b = 0; b < 2; ++b) {
            rg_mixer_grad_weights w;
            rg_mixer_grad_io io;
            good(w, io, s.kind);
            io.num_episodes = s.B, io.rows = s.rows, io.q_pitch = s.rows, io.obs_pitch = s.rows + 2, io.out_pitch = s.rows - 1, io.aux_pitch = s.rows;
            io.n_agents = w.m.n_agents = s.N, io.obs_dim = 4, w.m.state_dim = 4 * s.N;
            if (b == 0) io.d_mixed = nullptr, io.d_q = nullptr, io.d_pre = nullptr, io.d_p2 = nullptr, io.g = nullptr, io.aux_pitch = -7, w.w1b = nullptr, w.wfb = nullptr;
            else io.mixed = nullptr;
            if (s.kind != 2) {
                rg_mixer_weights m;
                memset(&m, 0, sizeof(m));
                m.kind = s.kind, m.n_agents = s.N;
                w.m = m, w.w1b = nullptr, w.wfb = nullptr;
                io.obs = nullptr, io.d_pre = nullptr, io.d_p2 = nullptr, io.g = nullptr, io.obs_pitch = 0, io.aux_pitch = 0, io.obs_dim = 0;
                if (b == 1) io.q = nullptr;
            }
            const int before = g_launches;
            const int rc = ENTRY[b](&w, &io, &stream_tag);
            ++g_checked;
            const bool ok = rc == 0 && g_launches == before + 1 && memcmp(&g_seen_w, &w, sizeof(w)) == 0 && memcmp(&g_seen_io, &io, sizeof(io)) == 0 &&
                            g_seen_stream == &stream_tag && g_seen_backward == b && g_seen_tiles == s.tiles;
            if (!ok) ++g_failed, printf("FAIL: a good call (kind %d, B %d, rows %d, N %d, backward %d) returned %d '%s', %d tiles\n", s.kind, s.B, s.rows, s.N, b, rc, rg_mixer_grad_last_error(), g_seen_tiles);
        }
    for (int b = 0; b < 2; ++b) {   // a failed launch is -30 and says what the runtime says
        rg_mixer_grad_weights w;
        rg_mixer_grad_io io;
        good(w, io, 2);
        g_stub_result = hipErrorInvalidValue;
        const int rc = ENTRY[b](&w, &io, nullptr);
        g_stub_result = hipSuccess;
        ++g_checked;
        if (rc != -30 || !strstr(rg_mixer_grad_last_error(), "the launch failed")) ++g_failed, printf("FAIL: launch failure gave %d '%s'\n", rc, rg_mixer_grad_last_error());
    }
    if (rg_sizeof_mixer_grad_weights() != 104 || rg_sizeof_mixer_grad_io() != 120) ++g_failed, printf("FAIL: struct sizes\n");
    printf("mixer_host: %d checks, %d failed, %d launches reached the stub\n", g_checked, g_failed, g_launches);
    return g_failed ? 1 : 0;
}
