// The ring allocation's two layouts (opencl_render_amd/csrc/rt_path_state.h) on the host, as a program of its own.  For each capacity given
// (default 65536 and 131072) it walks every path id and checks that the class layout's four quads per path -- (slot 0, quad 1) and (slot 1,
// quads 0..2) -- lie inside the RT_PATH_RING_QUADS * capacity quads of the allocation, that no two of them over all paths share a quad, and
// that a path's bounce record lies inside one 128-byte line; and that the general layout is a * 36 + slot * 3 + quad for every slot and quad
// (and so inside the allocation and distinct as well).  Prints one summary line and exits 0, or prints what went wrong and exits 1.
//   path_state_host [capacity ...]
#include "rt_path_state.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

int failures = 0;
void fail(const char *what, uint32_t capacity, uint32_t a, uint32_t slot, uint32_t quad, size_t at)
{
    if (++failures <= 20) std::printf("capacity %u path %u slot %u quad %u -> quad index %zu: %s\n", capacity, a, slot, quad, at, what);
}

void check(uint32_t capacity)
{
    const size_t quads = (size_t)RT_PATH_RING_QUADS * capacity;
    const size_t lineQuads = 128 / 16;
    std::vector<uint8_t> used(quads, 0); // one mark per quad of the allocation
    auto claim = [&](uint32_t a, uint32_t slot, uint32_t quad) -> size_t {
        const size_t at = rt_path_class_quad(capacity, a, slot, quad);
        if (at >= quads) { fail("outside the allocation", capacity, a, slot, quad, at); return at; }
        if (used[at]) fail("quad used twice", capacity, a, slot, quad, at);
        used[at] = 1;
        return at;
    };
    for (uint32_t a = 0; a < capacity; ++a) {
        claim(a, 0u, 1u);
        const size_t b0 = claim(a, RT_PATH_CLASS_BOUNCE_SLOT, 0u), b1 = claim(a, RT_PATH_CLASS_BOUNCE_SLOT, 1u), b2 = claim(a, RT_PATH_CLASS_BOUNCE_SLOT, 2u);
        if (b1 != b0 + 1 || b2 != b0 + 2) fail("bounce record not contiguous", capacity, a, RT_PATH_CLASS_BOUNCE_SLOT, 0u, b0);
        if (b0 / lineQuads != b2 / lineQuads) fail("bounce record straddles a 128-byte line", capacity, a, RT_PATH_CLASS_BOUNCE_SLOT, 0u, b0);
    }
    for (uint32_t a = 0; a < capacity; ++a)
        for (uint32_t slot = 0; slot < RT_PATH_RING_SLOTS; ++slot)
            for (uint32_t quad = 0; quad < 3; ++quad) {
                const size_t at = rt_path_ring_quad(a, slot, quad);
                if (at != (size_t)a * 36 + slot * 3 + quad) fail("general layout is not a * 36 + slot * 3 + quad", capacity, a, slot, quad, at);
                if (at >= quads) fail("general layout outside the allocation", capacity, a, slot, quad, at);
            }
}

} // namespace

int main(int argc, char **argv)
{
    std::vector<uint32_t> capacities;
    for (int i = 1; i < argc; ++i) capacities.push_back((uint32_t)std::strtoul(argv[i], nullptr, 10));
    if (capacities.empty()) capacities = { 65536u, 131072u };
    for (uint32_t c : capacities) check(c);
    std::printf("capacities %zu failures %d\n", capacities.size(), failures);
    return failures ? 1 : 0;
}
