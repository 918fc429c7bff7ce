// host_checks.h -- what the C entry points' argument checks share: the last-error text, tables of named pointers, the
// element-count limit.  A new entry point uses these and writes none of them again; which code and which message a refusal
// gets stays with the entry.  Plain host C++ (no HIP runtime call, no device code: a host compiler builds it alone,
// tests/sanitize/host_checks_host.cpp does), and only what at least two units use.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace rg {

// The last-error text of one entry, written into the unit's own thread_local buffer (every unit keeps its buffer and its
// exported *_last_error()).  `entry` is the prefix "<entry>: " of every text, or null for none.  An entry names its holder `fail`:
//     const rg::Fail fail{g_err, sizeof(g_err), "rg_entry"};  ...  return fail(-3, "io.obs", "is NULL");
// A text longer than the buffer is cut and terminated as snprintf does it.  text(): `fmt` holds at most two %s.
struct Fail {
    char *buf;
    size_t size;
    const char *entry;
    int text(int code, const char *fmt, const char *a = "", const char *b = "") const {
        const int n = entry ? snprintf(buf, size, "%s: ", entry) : 0;
        if (n >= 0 && static_cast<size_t>(n) < size) snprintf(buf + n, size - n, fmt, a, b);
        return code;
    }
    int operator()(int code, const char *what, const char *msg) const { return text(code, "%s %s", what, msg); }
    int operator()(int code, const char *msg) const { return text(code, "%s", msg); }
};

// A table of named pointers; `align` (a power of two) where the entries of one table differ in it.  first_null and
// first_misaligned return the first offender, or null: its index is `found - table`.  A NULL pointer is aligned.
struct NamedPtr {
    const void *p;
    const char *name;
    size_t align = 1;
};
template <class... P>
inline bool all_aligned(size_t align, const P *...p) { return ((reinterpret_cast<uintptr_t>(p) | ... | uintptr_t(0)) & (align - 1)) == 0; }
template <size_t N>
inline const NamedPtr *first_null(const NamedPtr (&table)[N], size_t n = N) {   // among the first n entries
    for (size_t i = 0; i < n; ++i)
        if (!table[i].p) return &table[i];
    return nullptr;
}
template <size_t N>
inline const NamedPtr *first_misaligned(const NamedPtr (&table)[N], size_t align = 0) {   // align 0: each entry's own
    for (const NamedPtr &f : table)
        if (!all_aligned(align ? align : f.align, f.p)) return &f;
    return nullptr;
}

// The kernels index their arrays with 32-bit integers: true iff the product of the factors (each >= 0) is at most 2^31 - 1.
// Nothing is multiplied, so nothing overflows whatever the inputs: the limit is divided by every factor in turn, and
// floor(floor(x / a) / b) = floor(x / (a b)), so what is left is >= 1 exactly when the product is within the limit.  A zero factor
// makes the product 0, which fits.  The entries check every factor to be >= 1 before they ask; then "every prefix of the product
// is within the limit, and the whole is" -- how each of them used to write it -- says no more than "the whole is".
template <class... F>
inline bool elements_fit(F... factors) {
    const int64_t f[] = {static_cast<int64_t>(factors)...};
    int64_t room = 0x7fffffff;
    for (int64_t v : f)
        if (v == 0) return true;
    for (int64_t v : f) room /= v;
    return room >= 1;
}

}  // namespace rg
