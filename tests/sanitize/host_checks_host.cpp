// host_checks_host.cpp -- csrc/host_checks.h alone (it includes nothing else of the library) under ASan + UBSan, in a stand-alone
// program: elements_fit against a 128-bit product on every tuple of 2 to 5 factors from a list that straddles every limit (UBSan's
// signed-overflow check is the point), the pointer tables on tables whose first offender is known, and the error text at the end
// of its buffer.  Built and run by tests/test_host_checks.py; test infrastructure only.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../marbler_amd/csrc/host_checks.h"

static int g_checked = 0, g_failed = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        ++g_checked;                      \
        if (!(cond)) {                    \
            ++g_failed;                   \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");                 \
        }                                 \
    } while (0)

static const int64_t FACTORS[] = {0, 1, 2, 3, 1 << 15, (1 << 16) - 1, 1 << 16, (1 << 16) + 1, (1ll << 31) - 2, (1ll << 31) - 1,
                                  1ll << 31, 1ll << 62, INT64_MAX};
constexpr int NF = sizeof(FACTORS) / sizeof(FACTORS[0]);

static bool fits128(const int64_t *f, int n) {   // (a running product of at most 2^31 - 1 times a factor below 2^63 is below 2^94)
    unsigned __int128 acc = 1;
    bool over = false;
    for (int i = 0; i < n; ++i) {
        if (f[i] == 0) return true;
        acc *= static_cast<unsigned __int128>(f[i]);
        if (acc > 0x7fffffffu) over = true, acc = 1;
    }
    return !over;
}

static void tuples(int64_t *f, int n, int at) {
    if (at < n) {
        for (int i = 0; i < NF; ++i) {
            f[at] = FACTORS[i];
            tuples(f, n, at + 1);
        }
        return;
    }
    const bool got = n == 2   ? rg::elements_fit(f[0], f[1])
                     : n == 3 ? rg::elements_fit(f[0], f[1], f[2])
                     : n == 4 ? rg::elements_fit(f[0], f[1], f[2], f[3])
                              : rg::elements_fit(f[0], f[1], f[2], f[3], f[4]);
    EXPECT(got == fits128(f, n), "elements_fit(%lld, %lld, %lld, %lld, %lld) of %d factors gave %d", (long long)f[0], (long long)f[1],
           (long long)(n > 2 ? f[2] : -1), (long long)(n > 3 ? f[3] : -1), (long long)(n > 4 ? f[4] : -1), n, got);
}

static const void *at(uintptr_t a) { return reinterpret_cast<const void *>(a); }   // (never dereferenced)

int main() {
    // ---- elements_fit
    int64_t f[5];
    for (int n = 2; n <= 5; ++n) tuples(f, n, 0);
    EXPECT(rg::elements_fit(1, 2, 3) && rg::elements_fit(46341, 46340) && !rg::elements_fit(46341, 46342), "int arguments");
    EXPECT(rg::elements_fit(int32_t(0x7fffffff)) && !rg::elements_fit(int32_t(0x7fffffff), int32_t(0x7fffffff)), "the largest int");

    // ---- the pointer tables: the first offender, and its index
    {
        const rg::NamedPtr good[] = {{at(0x1000), "a"}, {at(0x2000), "b"}, {at(0x3000), "c"}, {at(0x4000), "d"}};
        EXPECT(!rg::first_null(good) && !rg::first_misaligned(good, 16) && !rg::first_misaligned(good), "a table without a fault");
        for (int first : {0, 2, 3}) {   // a NULL first, in the middle, last; a later one must not be reported
            rg::NamedPtr t[] = {{at(0x1000), "a"}, {at(0x2000), "b"}, {at(0x3000), "c"}, {at(0x4000), "d"}};
            t[first].p = nullptr;
            if (first == 0) t[2].p = nullptr;
            const rg::NamedPtr *got = rg::first_null(t);
            EXPECT(got && got - t == first && !strcmp(got->name, good[first].name), "first_null: NULL at %d", first);
            EXPECT(rg::first_null(t, first) == nullptr, "first_null over the %d entries in front of the NULL", first);
            EXPECT(!rg::first_misaligned(t, 16), "a NULL pointer is aligned");
        }
    }
    for (size_t off : {1u, 4u, 8u})
        for (size_t align : {1u, 4u, 16u}) {
            const bool bad = (off & (align - 1)) != 0;
            // the alignment as the call's, then as the entry's own; entry 1 is the first offender, entry 3 a later one
            const rg::NamedPtr t[] = {{at(0x1000), "a", 1}, {at(0x2000 + off), "b", align}, {at(0x3000), "c", 16}, {at(0x4000 + off), "d", align}};
            for (const rg::NamedPtr *got : {rg::first_misaligned(t, align), rg::first_misaligned(t)})
                EXPECT(bad ? (got && got - t == 1 && !strcmp(got->name, "b")) : got == nullptr, "first_misaligned: offset %zu against %zu", off, align);
            EXPECT(rg::all_aligned(align, t[0].p, t[1].p, t[2].p) == !bad && rg::all_aligned(align, t[0].p, t[2].p), "all_aligned: offset %zu against %zu", off, align);
        }

    // ---- the error text: cut at the buffer's size, terminated, nothing behind the buffer touched
    {
        struct {
            char buf[256];
            char after[8];
        } m;
        char what[301], msg[301];
        memset(what, 'w', 300), memset(msg, 'm', 300);
        what[300] = msg[300] = 0;
        memset(&m, 0x5a, sizeof(m));
        const rg::Fail fail{m.buf, sizeof(m.buf), "rg_entry"};
        EXPECT(fail(-7, what, msg) == -7, "the code comes back");
        char want[1024];
        snprintf(want, sizeof(want), "rg_entry: %s %s", what, msg);
        EXPECT(strlen(m.buf) == 255 && !strncmp(m.buf, want, 255) && m.after[0] == 0x5a && m.after[7] == 0x5a, "three-part text cut at 255");
        memset(&m, 0x5a, sizeof(m));
        EXPECT(fail(-8, msg) == -8 && strlen(m.buf) == 255 && !strncmp(m.buf, "rg_entry: mmmm", 14) && m.after[0] == 0x5a, "two-part text cut at 255");
        EXPECT(fail(-9, "io.obs", "is NULL") == -9 && !strcmp(m.buf, "rg_entry: io.obs is NULL"), "what msg: '%s'", m.buf);
        EXPECT(fail(-9, "rgb is NULL") == -9 && !strcmp(m.buf, "rg_entry: rgb is NULL"), "msg: '%s'", m.buf);
        const rg::Fail bare{m.buf, sizeof(m.buf), nullptr};
        EXPECT(bare(-1, "handle is NULL") == -1 && !strcmp(m.buf, "handle is NULL"), "no entry: '%s'", m.buf);
        EXPECT(bare.text(-15, "rps constant %s is outside", "time_step") == -15 && !strcmp(m.buf, "rps constant time_step is outside"), "text: '%s'", m.buf);
        // an entry name that fills the buffer by itself
        memset(&m, 0x5a, sizeof(m));
        const rg::Fail wide{m.buf, sizeof(m.buf), what};
        EXPECT(wide(-2, "x") == -2 && strlen(m.buf) == 255 && m.buf[254] == 'w' && m.after[0] == 0x5a, "an entry name longer than the buffer");
        memset(&m, 0x5a, sizeof(m));
        const rg::Fail tiny{m.buf, 10, "rg_entry"};   // "rg_entry: " is ten characters: the prefix alone is cut
        EXPECT(tiny(-3, "x") == -3 && !strcmp(m.buf, "rg_entry:") && m.buf[10] == 0x5a, "a buffer the prefix fills: '%s'", m.buf);
    }
    printf("host_checks_host: %d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
