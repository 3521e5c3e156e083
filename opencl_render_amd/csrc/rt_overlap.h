// rt_overlap.h -- the arrays of a call that takes device pointers, and which of them overlaps one the call writes.  No HIP in here:
// tests/overlap_host.cpp compiles it for the host on its own.
#pragma once
#include <cstdint>

struct RtArray {
    const void *p;        // null: an optional array that was not given
    uint64_t bytes, align;
    const char *what;     // its name in error texts
    bool written = false; // the call writes it: it may overlap no other array
};

// The first pair "entry i, written entry k" (i != k, both given) whose byte ranges overlap, going through every entry and, for each, through
// every written entry, both in table order; false when there is none.
inline bool rt_first_overlap(const RtArray *a, int n, int *entry, int *written)
{
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < n; ++k) {
            if (i == k || !a[k].written || !a[i].p || !a[k].p) continue;
            const uintptr_t x = (uintptr_t)a[i].p, y = (uintptr_t)a[k].p;
            if (x < y + a[k].bytes && y < x + a[i].bytes) { *entry = i; *written = k; return true; }
        }
    return false;
}
