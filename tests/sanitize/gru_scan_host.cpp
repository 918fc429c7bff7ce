// gru_scan_host.cpp -- the host half of csrc/robogym_gru_scan.hip (compiled with -DRG_GRU_SCAN_HOST_ONLY, for the host alone, under
// ASan + UBSan) in a stand-alone program: its own main and its own launch stub.  It walks every refusal of rg_gru_scan_forward and
// rg_gru_scan_backward with pointers that are never dereferenced, then lets calls through to the stub and checks what arrives there,
// the number of workgroups included.  Built and run by tests/test_gru_scan_host_sanitized.py; test infrastructure only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>

#include "../../include/robogym_learn.h"

static int g_launches = 0;
static hipError_t g_stub_result = hipSuccess;
static rg_gru_scan_weights g_seen_w;
static rg_gru_scan_io g_seen_io;
static int g_seen_backward = -1, g_seen_tiles = -1;
static void *g_seen_stream = nullptr;

hipError_t rg_gru_scan_launch_stub(const rg_gru_scan_weights &w, const rg_gru_scan_io &io, int backward, int tiles, void *hip_stream) {
    ++g_launches;
    g_seen_w = w;
    g_seen_io = io;
    g_seen_backward = backward, g_seen_tiles = tiles;
    g_seen_stream = hip_stream;
    return g_stub_result;
}

template <class T>
static T *fake(uintptr_t a) { return reinterpret_cast<T *>(a); }

static void good(rg_gru_scan_weights &w, rg_gru_scan_io &io, int n_sets) {
    memset(&w, 0, sizeof(w));
    memset(&io, 0, sizeof(io));
    w.w_hh = fake<const float>(0x10000), w.b_hh = fake<const float>(0x20000), w.w_hh_t = nullptr, w.n_sets = n_sets, w.hidden_dim = 128;
    io.gi = fake<const float>(0x1000000), io.hidden_in = fake<const float>(0x1100000), io.h = fake<float>(0x1200000);
    io.gates = fake<float>(0x1300000), io.hidden_out = fake<float>(0x1400000), io.dh_ext = fake<const float>(0x1500000);
    io.d_hidden_out = fake<const float>(0x1600000), io.dgi = fake<float>(0x1700000), io.dghn = fake<float>(0x1800000);
    io.d_hidden_in = fake<float>(0x1900000);
    io.num_episodes = 3, io.n_agents = 4, io.rows = 7, io.gi_pitch = 9, io.save_pitch = 8, io.grad_pitch = 7;
}

static int g_failed = 0, g_checked = 0;
typedef int (*entry_t)(const rg_gru_scan_weights *, const rg_gru_scan_io *, void *);
static const entry_t ENTRY[2] = {rg_gru_scan_forward, rg_gru_scan_backward};
static const char *PREFIX[2] = {"rg_gru_scan_forward: ", "rg_gru_scan_backward: "};

// `which`: 0 forward, 1 backward, 2 both
static void expect(int which, int want, const char *word, const std::function<void(rg_gru_scan_weights &, rg_gru_scan_io &)> &change, int n_sets = 1) {
    for (int b = 0; b < 2; ++b) {
        if (which != 2 && which != b) continue;
        rg_gru_scan_weights w;
        rg_gru_scan_io io;
        good(w, io, n_sets);
        change(w, io);
        const int before = g_launches;
        const int rc = ENTRY[b](&w, &io, nullptr);
        const char *msg = rg_gru_scan_last_error();
        ++g_checked;
        if (rc != want || !strstr(msg, word) || strncmp(msg, PREFIX[b], strlen(PREFIX[b])) != 0 || g_launches != before) {
            ++g_failed;
            printf("FAIL (%s): wanted %d naming '%s', got %d '%s' (%d launches)\n", PREFIX[b], want, word, rc, msg, g_launches - before);
        }
    }
}

int main() {
    const int big = std::numeric_limits<int>::max(), small = std::numeric_limits<int>::min();
    for (int b = 0; b < 2; ++b) {
        rg_gru_scan_weights w;
        rg_gru_scan_io io;
        good(w, io, 1);
        ++g_checked;
        if (ENTRY[b](nullptr, &io, nullptr) != -1 || !strstr(rg_gru_scan_last_error(), "w is NULL")) ++g_failed, printf("FAIL: w NULL\n");
        ++g_checked;
        if (ENTRY[b](&w, nullptr, nullptr) != -2 || !strstr(rg_gru_scan_last_error(), "io is NULL")) ++g_failed, printf("FAIL: io NULL\n");
    }
    expect(0, -3, "io.gi is NULL", [](auto &, auto &io) { io.gi = nullptr; });
    expect(0, -3, "io.h is NULL", [](auto &, auto &io) { io.h = nullptr; });
    expect(1, -3, "io.h is NULL", [](auto &, auto &io) { io.h = nullptr; });
    expect(1, -3, "io.dh_ext is NULL", [](auto &, auto &io) { io.dh_ext = nullptr; });
    expect(1, -3, "io.dgi is NULL", [](auto &, auto &io) { io.dgi = nullptr; });
    expect(1, -3, "io.dghn is NULL", [](auto &, auto &io) { io.dghn = nullptr; });
    expect(2, -4, "w.w_hh is NULL", [](auto &w, auto &) { w.w_hh = nullptr; });
    expect(0, -4, "w.b_hh is NULL", [](auto &w, auto &) { w.b_hh = nullptr; });
    for (uintptr_t off : {4u, 8u, 12u}) {
        expect(2, -5, "w.w_hh must be 16-byte aligned", [off](auto &w, auto &) { w.w_hh = fake<const float>(0x700000 + off); });
        expect(0, -5, "w.b_hh must be 16-byte aligned", [off](auto &w, auto &) { w.b_hh = fake<const float>(0x700000 + off); });
        expect(0, -5, "w.w_hh_t must be 16-byte aligned", [off](auto &w, auto &) { w.w_hh_t = fake<const float>(0x700000 + off); });
    }
    for (uintptr_t off : {1u, 2u, 3u}) {
        expect(0, -5, "io.gi must be 4-byte aligned", [off](auto &, auto &io) { io.gi = fake<const float>(0x700000 + off); });
        expect(2, -5, "io.hidden_in must be 4-byte aligned", [off](auto &, auto &io) { io.hidden_in = fake<const float>(0x700000 + off); });
        expect(2, -5, "io.h must be 4-byte aligned", [off](auto &, auto &io) { io.h = fake<float>(0x700000 + off); });
        expect(2, -5, "io.gates must be 4-byte aligned", [off](auto &, auto &io) { io.gates = fake<float>(0x700000 + off); });
        expect(0, -5, "io.hidden_out must be 4-byte aligned", [off](auto &, auto &io) { io.hidden_out = fake<float>(0x700000 + off); });
        expect(1, -5, "io.dh_ext must be 4-byte aligned", [off](auto &, auto &io) { io.dh_ext = fake<const float>(0x700000 + off); });
        expect(1, -5, "io.d_hidden_out must be 4-byte aligned", [off](auto &, auto &io) { io.d_hidden_out = fake<const float>(0x700000 + off); });
        expect(1, -5, "io.dgi must be 4-byte aligned", [off](auto &, auto &io) { io.dgi = fake<float>(0x700000 + off); });
        expect(1, -5, "io.dghn must be 4-byte aligned", [off](auto &, auto &io) { io.dghn = fake<float>(0x700000 + off); });
        expect(1, -5, "io.d_hidden_in must be 4-byte aligned", [off](auto &, auto &io) { io.d_hidden_in = fake<float>(0x700000 + off); });
    }
    for (int h : {0, 32, 96, 256, -128, big, small}) expect(2, -6, "w.hidden_dim", [h](auto &w, auto &) { w.hidden_dim = h; });
    for (int s : {0, 2, 3, 5, -1, big, small}) expect(2, -7, "w.n_sets", [s](auto &w, auto &) { w.n_sets = s; });
    for (int n : {0, -1, 17, big, small}) expect(2, -8, "io.n_agents", [n](auto &, auto &io) { io.n_agents = n; });
    for (int v : {0, -3, small}) {
        expect(2, -9, "io.num_episodes", [v](auto &, auto &io) { io.num_episodes = v; });
        expect(2, -10, "io.rows must be >= 1", [v](auto &, auto &io) { io.rows = v; });
    }
    expect(2, -11, "io.rows is above 4096", [](auto &, auto &io) { io.rows = io.gi_pitch = io.save_pitch = io.grad_pitch = 4097; });
    expect(2, -11, "io.rows is above 4096", [big](auto &, auto &io) { io.rows = big; });
    for (int v : {6, 0, -1, small}) {
        expect(0, -12, "io.gi_pitch", [v](auto &, auto &io) { io.gi_pitch = v; });
        expect(2, -13, "io.save_pitch", [v](auto &, auto &io) { io.save_pitch = v; });
        expect(1, -14, "io.grad_pitch", [v](auto &, auto &io) { io.grad_pitch = v; });
    }
    expect(1, -15, "io.gates", [](auto &, auto &io) { io.gates = nullptr; });
    for (int k = 0; k < 2; ++k) {
        expect(2, -20, "w.reserved", [k](auto &w, auto &) { w.reserved[k] = 1; });
        expect(2, -20, "io.reserved", [k, small](auto &, auto &io) { io.reserved[k] = small; });
    }
    expect(0, -21, "gi_pitch * n_agents * 3 hidden_dim", [](auto &, auto &io) { io.gi_pitch = 1 << 21; });
    expect(2, -21, "save_pitch * n_agents * 4 hidden_dim", [](auto &, auto &io) { io.save_pitch = 1 << 21; });
    expect(1, -21, "grad_pitch * n_agents * 3 hidden_dim", [](auto &, auto &io) { io.grad_pitch = 1 << 21; });
    expect(2, -21, "exceeds 2^31 - 1", [big](auto &, auto &io) {   // every factor as large as an int gets: no overflow on the way
        io.num_episodes = io.gi_pitch = io.save_pitch = io.grad_pitch = big;
    });

    // calls that pass every check arrive at the launch exactly as given, with the number of tiles of 32 flat rows
    int stream_tag = 0;
    struct Shape {
        int B, N, n_sets, H, tiles;
    };
    const Shape shapes[] = {{3, 4, 1, 128, 1}, {8, 4, 1, 64, 1}, {33, 1, 1, 128, 2}, {13, 5, 1, 64, 3}, {13, 5, 5, 128, 5}, {33, 2, 2, 64, 4},
                            {4096, 4, 1, 128, 512}, {4096, 16, 16, 64, 2048}};
    for (const Shape &s : shapes)
        for (int b = 0; b < 2; ++b) {
            rg_gru_scan_weights w;
            rg_gru_scan_io io;
            good(w, io, s.n_sets);
            io.num_episodes = s.B, io.n_agents = s.N, w.hidden_dim = s.H;
            if (b == 0) io.gates = nullptr, io.hidden_in = nullptr, io.hidden_out = nullptr, io.dh_ext = nullptr, io.dgi = nullptr, io.dghn = nullptr, io.grad_pitch = 0;
            else io.gi = nullptr, w.b_hh = nullptr, io.d_hidden_out = nullptr, io.d_hidden_in = nullptr, io.gi_pitch = -5;
            const int before = g_launches;
            const int rc = ENTRY[b](&w, &io, &stream_tag);
            ++g_checked;
            const bool ok = rc == 0 && g_launches == before + 1 && memcmp(&g_seen_w, &w, sizeof(w)) == 0 && memcmp(&g_seen_io, &io, sizeof(io)) == 0 &&
                            g_seen_stream == &stream_tag && g_seen_backward == b && g_seen_tiles == s.tiles;
            if (!ok) ++g_failed, printf("FAIL: a good call (B %d, N %d, sets %d, backward %d) returned %d '%s', %d tiles\n", s.B, s.N, s.n_sets, b, rc, rg_gru_scan_last_error(), g_seen_tiles);
        }
    {   // the edges of what is accepted: 4096 rows at the minimum pitches, the most agents
        rg_gru_scan_weights w;
        rg_gru_scan_io io;
        good(w, io, 16);
        io.n_agents = 16, io.num_episodes = 1, io.rows = io.gi_pitch = io.save_pitch = io.grad_pitch = 4096, w.hidden_dim = 64;
        for (int b = 0; b < 2; ++b) {
            ++g_checked;
            if (ENTRY[b](&w, &io, nullptr) != 0 || g_seen_tiles != 16) ++g_failed, printf("FAIL: the widest call: %s\n", rg_gru_scan_last_error());
        }
    }
    for (int b = 0; b < 2; ++b) {   // a failed launch is -30 and says what the runtime says
        rg_gru_scan_weights w;
        rg_gru_scan_io io;
        good(w, io, 4);
        g_stub_result = hipErrorInvalidValue;
        const int rc = ENTRY[b](&w, &io, nullptr);
        g_stub_result = hipSuccess;
        ++g_checked;
        if (rc != -30 || !strstr(rg_gru_scan_last_error(), "the launch failed")) ++g_failed, printf("FAIL: launch failure gave %d '%s'\n", rc, rg_gru_scan_last_error());
    }
    if (rg_sizeof_gru_scan_weights() != 40 || rg_sizeof_gru_scan_io() != 112) ++g_failed, printf("FAIL: struct sizes\n");
    printf("gru_scan_host: %d checks, %d failed, %d launches reached the stub\n", g_checked, g_failed, g_launches);
    return g_failed ? 1 : 0;
}
