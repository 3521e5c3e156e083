// The overlap check of csrc/rt_overlap.h -- what the filters' device entry points refuse arrays with (rt_filters.cpp,
// checked_device_arrays) -- for ctypes.  The addresses are only compared, never read.
#include "rt_overlap.h"

// pair[0], pair[1]: the entry and the written entry of the first overlap; returns 1 when there is one, 0 when none, -1 for n > 16.
extern "C" int overlap_host(int n, const uint64_t *address, const uint64_t *bytes, const int *written, int *pair)
{
    RtArray a[16];
    if (n < 0 || n > 16) return -1;
    for (int i = 0; i < n; ++i) a[i] = RtArray{ (const void *)(uintptr_t)address[i], bytes[i], 4, "", written[i] != 0 };
    return rt_first_overlap(a, n, &pair[0], &pair[1]) ? 1 : 0;
}
