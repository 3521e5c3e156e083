// The owner types of csrc/rt_owned.h on the host alone: this file DEFINES the few HIP calls the header makes, as counting stand-ins over
// malloc, so nothing links against the HIP runtime and nothing touches a device.  tests/test_owned.py drives the exported scenarios;
// with -DOWNED_HOST_MAIN the file is a program that walks the same scenarios itself (for a sanitizer build).
#include "rt_owned.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>

using namespace rthost;

namespace {

enum { K_DEVICE = 0, K_EVENT, K_PINNED, K_STREAM, KINDS };

struct Fake {
    uint64_t made[KINDS] = {}, gone[KINDS] = {}, badFrees = 0, errorReads = 0;
    uint64_t seq = 0, lastMade = 0, lastGone = 0; // device blocks: when the last one was allocated / freed
    uint64_t calls[KINDS] = {}, failAt[KINDS] = {}; // the failAt-th create call of a kind fails (0: none)
    std::map<void *, int> live;
} F;

hipError_t fake_make(int kind, void **out, size_t bytes)
{
    if (++F.calls[kind] == F.failAt[kind]) { *out = nullptr; return hipErrorOutOfMemory; }
    *out = malloc(bytes ? bytes : 1);
    F.live[*out] = kind;
    ++F.made[kind];
    if (kind == K_DEVICE) F.lastMade = ++F.seq;
    return hipSuccess;
}

hipError_t fake_free(int kind, void *p)
{
    auto it = F.live.find(p);
    if (it == F.live.end() || it->second != kind) { ++F.badFrees; return hipErrorInvalidValue; }
    F.live.erase(it);
    free(p);
    ++F.gone[kind];
    if (kind == K_DEVICE) F.lastGone = ++F.seq;
    return hipSuccess;
}

// a -> b by move construction, then b over a held c by move assignment.  out: a empty after the move | b holds a's handle | owners of
// the kind released when the assignment returns (c's own) | c holds a's handle | b empty | (device) b's size | c's size
template <class O, class Make> void move_case(Make make, uint64_t out[7])
{
    O a, c;
    make(a); make(c);
    const void *first = (const void *)a;
    O b(std::move(a));
    out[0] = !(const void *)a; out[1] = (const void *)b == first;
    const uint64_t before = F.gone[0] + F.gone[1] + F.gone[2] + F.gone[3];
    c = std::move(b);
    out[2] = F.gone[0] + F.gone[1] + F.gone[2] + F.gone[3] - before;
    out[3] = (const void *)c == first; out[4] = !(const void *)b;
}

} // namespace

extern "C" {

hipError_t hipMalloc(void **p, size_t bytes) { return fake_make(K_DEVICE, p, bytes); }
hipError_t hipFree(void *p) { return fake_free(K_DEVICE, p); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return fake_make(K_PINNED, p, bytes); }
hipError_t hipHostFree(void *p) { return fake_free(K_PINNED, p); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return fake_make(K_EVENT, (void **)e, 1); }
hipError_t hipEventDestroy(hipEvent_t e) { return fake_free(K_EVENT, e); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return fake_make(K_STREAM, (void **)s, 1); }
hipError_t hipStreamDestroy(hipStream_t s) { return fake_free(K_STREAM, s); }
hipError_t hipGetLastError(void) { ++F.errorReads; return hipSuccess; }

void owned_reset(void) { F = Fake(); }
void owned_fail(int kind, uint64_t nth) { F.calls[kind] = 0; F.failAt[kind] = nth; }
// made[4] | gone[4] | live | bad frees | sequence number of the last device allocation | of the last device free
void owned_counts(uint64_t out[12])
{
    for (int k = 0; k < KINDS; ++k) { out[k] = F.made[k]; out[4 + k] = F.gone[k]; }
    out[8] = F.live.size(); out[9] = F.badFrees; out[10] = F.lastMade; out[11] = F.lastGone;
}

// An owner of `kind` goes out of scope, holding something or empty.  Returns what make() returned.
int owned_scope(int kind, int hold)
{
    uint64_t total = 0;
    hipError_t e = hipSuccess;
    if (kind == K_DEVICE) { Dev<float> b; if (hold) e = b.make(64, total); }
    if (kind == K_EVENT) { Event v; if (hold) e = v.make(); if (hold && e == hipSuccess) e = v.make(); } // (the second make keeps the first event)
    if (kind == K_PINNED) { Pinned<uint32_t> h; if (hold) e = h.make(64, 0); }
    if (kind == K_STREAM) { Stream s; if (hold) e = s.make(0); }
    return (int)e;
}

void owned_move(int kind, uint64_t out[7])
{
    uint64_t total = 0;
    memset(out, 0, 7 * sizeof *out);
    if (kind == K_DEVICE) {
        Dev<> a, c;
        (void)a.make(48, total); (void)c.make(80, total);
        const void *first = a.p;
        Dev<> b(std::move(a));
        out[0] = !a.p && !a.size; out[1] = b.p == first;
        const uint64_t before = F.gone[K_DEVICE];
        c = std::move(b);
        out[2] = F.gone[K_DEVICE] - before; out[3] = c.p == first; out[4] = !b.p; out[5] = b.size; out[6] = c.size;
    }
    if (kind == K_EVENT) move_case<Event>([](Event &v) { (void)v.make(); }, out);
    if (kind == K_PINNED) move_case<Pinned<char>>([](Pinned<char> &h) { (void)h.make(32, 0); }, out);
    if (kind == K_STREAM) move_case<Stream>([](Stream &s) { (void)s.make(0); }, out);
}

// out: total after make | after drop | after a second block was made and destroyed without a drop | size while held | empty after drop
int owned_make_drop(uint64_t bytes, uint64_t total, uint64_t out[5])
{
    Dev<> b;
    const hipError_t e = b.make(bytes, total);
    out[0] = total; out[3] = b.size;
    b.drop(total);
    out[1] = total; out[4] = !b.p && !b.size;
    { Dev<> d; (void)d.make(bytes, total); }
    out[2] = total;
    return (int)e;
}

// A block of `held` bytes (0: none) is fitted to `need` the way the geometry buffers are: an eighth more, or exact, at least 64 bytes.
// out: same pointer as before | size | total (it starts at held + 1000) | want
int owned_fit(uint64_t held, uint64_t need, int exact, uint64_t out[4])
{
    uint64_t total = 1000;
    Dev<> b;
    if (held) (void)b.make(held, total);
    const void *before = b.p;
    const uint64_t grown = exact ? need : need + need / 8, want = grown > 64 ? grown : 64;
    const hipError_t e = b.fit(need, want, total);
    out[0] = b.p == before; out[1] = b.size; out[2] = total; out[3] = want;
    return (int)e;
}

// One block, four blocks, four events made locally and handed over when all are there (rtHipSceneSetCamera's first call).
// out: the scene's total | blocks the scene holds | events it holds
int owned_compound(uint64_t out[3])
{
    struct { Dev<> scratch; Dev<uint32_t> range[4]; Event ev[4]; uint64_t bytes = 0; } scene;
    const auto report = [&] {
        out[0] = scene.bytes; out[1] = (scene.scratch.p != nullptr); out[2] = 0;
        for (int i = 0; i < 4; ++i) { out[1] += scene.range[i].p != nullptr; out[2] += (hipEvent_t)scene.ev[i] != nullptr; }
    };
    Dev<> block;
    Dev<uint32_t> r[4];
    Event ev[4];
    uint64_t uncounted = 0;
    hipError_t e = block.make(4096, uncounted);
    for (int i = 0; e == hipSuccess && i < 4; ++i) e = r[i].make(256, uncounted);
    for (int i = 0; e == hipSuccess && i < 4; ++i) e = ev[i].make();
    if (e != hipSuccess) { report(); return (int)e; }
    scene.scratch.adopt(std::move(block), scene.bytes);
    for (int i = 0; i < 4; ++i) { scene.range[i].adopt(std::move(r[i]), scene.bytes); scene.ev[i] = std::move(ev[i]); }
    report();
    return 0;
}

// ---- DevPart: a list of blocks and their byte sum ---------------------------------------------------------------------------------
// block i of a test part has PART_BLOCK(i) bytes
#define PART_BLOCK(i) (uint64_t)(16 * ((i) + 1))

// `k` blocks are added to a part (the stand-in may have been told to fail one of the adds), then the part goes out of scope.
// out: blocks held when the adding stopped | the part's sum then | device blocks alive then | the earlier blocks kept pointer and size |
// *out was left alone by the failed add.  Returns the first failure.
int owned_part_fill(int k, uint64_t out[5])
{
    DevPart part;
    void *got[16] = {};
    hipError_t e = hipSuccess;
    void *sentinel = &part, *p = sentinel;
    for (int i = 0; i < k && i < 16 && e == hipSuccess; ++i) {
        p = sentinel;
        e = part.get(&p, PART_BLOCK(i));
        if (e == hipSuccess) got[i] = p;
    }
    out[0] = part.blocks.size(); out[1] = part.bytes; out[2] = F.live.size(); out[3] = 1;
    for (size_t i = 0; i < part.blocks.size(); ++i) out[3] = out[3] && part.blocks[i].p == got[i] && part.blocks[i].size == PART_BLOCK(i);
    out[4] = (e == hipSuccess) || p == sentinel;
    return (int)e;
}

// a (3 blocks) -> b by move construction, then b over a held c (1 block) by move assignment.  out: a empty with sum 0 | b's sum | blocks
// freed when the assignment returns (c's own) | c's sum | b empty with sum 0 | c's first block is a's first
void owned_part_move(uint64_t out[6])
{
    DevPart a, c;
    void *p = nullptr, *first = nullptr;
    for (int i = 0; i < 3; ++i) { (void)a.get(&p, PART_BLOCK(i)); if (!i) first = p; }
    (void)c.get(&p, 1000);
    DevPart b(std::move(a));
    out[0] = a.empty() && a.bytes == 0; out[1] = b.bytes;
    const uint64_t before = F.gone[K_DEVICE];
    c = std::move(b);
    out[2] = F.gone[K_DEVICE] - before; out[3] = c.bytes; out[4] = b.empty() && b.bytes == 0;
    out[5] = c.blocks.size() == 3 && c.blocks[0].p == first;
}

// A block of `bytes` made elsewhere is adopted by a part that holds one block.
// out: sum before | sum after | the part's last block is that block, pointer and size | the source is empty | what the maker counted
void owned_part_adopt(uint64_t bytes, uint64_t out[5])
{
    DevPart part;
    void *p = nullptr;
    (void)part.get(&p, PART_BLOCK(0));
    Dev<float> made;
    uint64_t uncounted = 0;
    (void)made.make(bytes, uncounted);
    const void *at = made.p;
    out[0] = part.bytes;
    part.adopt(std::move(made));
    out[1] = part.bytes; out[2] = part.blocks.size() == 2 && part.blocks[1].p == at && part.blocks[1].size == bytes;
    out[3] = !made.p && !made.size; out[4] = uncounted;
}

namespace {
// what rtHipScene (rt_host.h) does with its parts, without its stream
struct PartScene {
    DevPart parts[2];
    uint64_t bytes = 0;
    void drop_part(int part) { bytes -= parts[part].bytes; parts[part].clear(); }
    void install(int part, DevPart &&fresh) { drop_part(part); bytes += fresh.bytes; parts[part] = std::move(fresh); }
};
bool part_of(DevPart &part, int first, int count)
{
    void *p = nullptr;
    for (int i = first; i < first + count; ++i)
        if (part.get(&p, PART_BLOCK(i)) != hipSuccess) return false;
    return true;
}
} // namespace

// A scene holds part 0 (blocks 0, 1) and part 1 (block 2).  A part of blocks 3, 4, 5 is built beside part 0 and installed over it --
// unless one of its adds fails (the stand-in is told by the caller; the scene's three are made before the count starts at `failAt`),
// in which case the build returns before install.  Then part 1 is dropped.
// out: total before | total after the install or the refusal | blocks freed by install | part 0 kept its first block's pointer |
// blocks alive after the install or the refusal | total after the drop | blocks freed by the drop | installed (1) or refused (0)
void owned_scene_handover(uint64_t failAt, uint64_t out[8])
{
    PartScene scene;
    DevPart a, b;
    (void)part_of(a, 0, 2); (void)part_of(b, 2, 1);
    scene.install(0, std::move(a)); scene.install(1, std::move(b));
    const void *held = scene.parts[0].blocks[0].p;
    out[0] = scene.bytes;
    owned_fail(K_DEVICE, failAt);
    uint64_t before = F.gone[K_DEVICE];
    out[7] = [&] {
        DevPart fresh;
        if (!part_of(fresh, 3, 3)) return 0;
        scene.install(0, std::move(fresh));
        out[2] = F.gone[K_DEVICE] - before; // (when install returns: before `fresh` goes out of scope)
        return 1;
    }();
    if (!out[7]) out[2] = 0;
    out[1] = scene.bytes; out[3] = scene.parts[0].blocks[0].p == held; out[4] = F.live.size();
    before = F.gone[K_DEVICE];
    scene.drop_part(1);
    out[5] = scene.bytes; out[6] = F.gone[K_DEVICE] - before;
}

// The lights edit's growth: two blocks made locally, counted nowhere, are adopted by the installed part 1 and their bytes counted.
// out: total before | total after | part 1's sum after | blocks of part 1 | both sources empty
void owned_scene_grow(uint64_t first, uint64_t second, uint64_t out[5])
{
    PartScene scene;
    DevPart a, b;
    (void)part_of(a, 0, 2); (void)part_of(b, 2, 1);
    scene.install(0, std::move(a)); scene.install(1, std::move(b));
    out[0] = scene.bytes;
    Dev<float> x;
    Dev<unsigned long long> y;
    uint64_t uncounted = 0;
    (void)x.make(first, uncounted); (void)y.make(second, uncounted);
    scene.parts[1].adopt(std::move(x)); scene.parts[1].adopt(std::move(y));
    scene.bytes += uncounted;
    out[1] = scene.bytes; out[2] = scene.parts[1].bytes; out[3] = scene.parts[1].blocks.size(); out[4] = !x.p && !x.size && !y.p && !y.size;
}

} // extern "C"

#ifdef OWNED_HOST_MAIN
static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { ++g_bad; fprintf(stderr, "line %d: %s\n", __LINE__, #x); } } while (0)
static bool settled() { return F.live.empty() && !F.badFrees && F.made[0] == F.gone[0] && F.made[1] == F.gone[1] && F.made[2] == F.gone[2] && F.made[3] == F.gone[3]; }

int main()
{
    uint64_t o[7];
    for (int kind = 0; kind < KINDS; ++kind) {
        owned_reset(); CHECK(owned_scope(kind, 0) == 0 && F.made[kind] == 0 && F.gone[kind] == 0 && settled());
        owned_reset(); CHECK(owned_scope(kind, 1) == 0 && F.made[kind] == 1 && F.gone[kind] == 1 && settled());
        owned_reset(); owned_move(kind, o);
        CHECK(o[0] && o[1] && o[2] == 1 && o[3] && o[4] && F.made[kind] == 2 && settled());
        if (kind == K_DEVICE) CHECK(o[5] == 0 && o[6] == 48);
        owned_reset(); owned_fail(kind, 1); CHECK(owned_scope(kind, 1) != 0 && F.made[kind] == 0 && settled());
    }
    owned_reset();
    CHECK(owned_make_drop(96, 500, o) == 0 && o[0] == 596 && o[1] == 500 && o[2] == 596 && o[3] == 96 && o[4] && settled());
    owned_reset(); owned_fail(K_DEVICE, 1);
    CHECK(owned_make_drop(96, 500, o) != 0 && o[0] == 500 && o[3] == 0 && settled());
    for (uint64_t held : { (uint64_t)0, (uint64_t)4096 })
        for (uint64_t need : { held ? held - 1 : 0, held, held + 1 })
            for (int exact = 0; exact < 2; ++exact) {
                owned_reset();
                CHECK(owned_fit(held, need, exact, o) == 0 && settled());
                const bool keep = held && held >= need;
                CHECK(o[0] == (keep ? 1u : 0u) && o[1] == (keep ? held : o[3]) && o[2] == 1000 + o[1]);
                uint64_t c[12];
                owned_counts(c);
                if (!keep && held) CHECK(c[10] < c[11] && c[0] == 2); // the new block was there before the old one went
                owned_reset(); owned_fail(K_DEVICE, held ? 2 : 1);
                const int rc = owned_fit(held, need, exact, o);
                CHECK(keep ? rc == 0 : (rc != 0 && o[0] && o[1] == held && o[2] == 1000 + held));
                CHECK(settled());
            }
    for (int kind : { K_DEVICE, K_EVENT })
        for (uint64_t nth = 0; nth <= (kind == K_DEVICE ? 5u : 4u); ++nth) {
            owned_reset(); owned_fail(kind, nth);
            const int rc = owned_compound(o);
            CHECK(nth ? (rc != 0 && o[0] == 0 && o[1] == 0 && o[2] == 0) : (rc == 0 && o[0] == 4096 + 4 * 256 && o[1] == 5 && o[2] == 4));
            CHECK(settled());
        }
    // DevPart
    uint64_t q[8];
    const auto sum = [](int n) { uint64_t s = 0; for (int i = 0; i < n; ++i) s += PART_BLOCK(i); return s; };
    for (int k : { 0, 1, 4 }) {
        owned_reset();
        CHECK(owned_part_fill(k, q) == 0 && q[0] == (uint64_t)k && q[1] == sum(k) && q[2] == (uint64_t)k && q[3]);
        CHECK(F.made[K_DEVICE] == (uint64_t)k && settled());
    }
    for (int n = 1; n <= 4; ++n) {
        owned_reset(); owned_fail(K_DEVICE, n);
        CHECK(owned_part_fill(4, q) != 0 && q[0] == (uint64_t)n - 1 && q[1] == sum(n - 1) && q[2] == (uint64_t)n - 1 && q[3] && q[4]);
        CHECK(F.made[K_DEVICE] == (uint64_t)n - 1 && settled());
    }
    owned_reset(); owned_part_move(q);
    CHECK(q[0] && q[1] == sum(3) && q[2] == 1 && q[3] == sum(3) && q[4] && q[5] && F.made[K_DEVICE] == 4 && settled());
    owned_reset(); owned_part_adopt(4000, q);
    CHECK(q[0] == 16 && q[1] == 4016 && q[2] && q[3] && q[4] == 4000 && F.made[K_DEVICE] == 2 && settled());
    for (uint64_t failAt = 0; failAt <= 3; ++failAt) {
        owned_reset(); owned_scene_handover(failAt, q);
        CHECK(q[0] == 96 && q[5] == q[1] - 48 && q[6] == 1);
        if (failAt) CHECK(!q[7] && q[1] == 96 && q[2] == 0 && q[3] && q[4] == 3 && F.made[K_DEVICE] == 3 + failAt - 1);
        else CHECK(q[7] && q[1] == 96 - 48 + 240 && q[2] == 2 && !q[3] && q[4] == 4 && F.made[K_DEVICE] == 6);
        CHECK(settled());
    }
    owned_reset(); owned_scene_grow(4096, 2048, q);
    CHECK(q[0] == 96 && q[1] == 96 + 6144 && q[2] == 48 + 6144 && q[3] == 3 && q[4] && F.made[K_DEVICE] == 5 && settled());
    printf(g_bad ? "owned_host: %d checks FAILED\n" : "owned_host: all checks passed\n", g_bad);
    return g_bad ? 1 : 0;
}
#endif
