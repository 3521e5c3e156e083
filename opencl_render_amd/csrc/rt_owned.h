// rt_owned.h -- owners of what the host library holds on a device: memory, pinned host memory, events, streams.  Move-only; the destructor
// releases what is held, so a struct made of them (rtHipScene, rt_host.h) has no list of things to free.  Only the HIP runtime's API header
// and the standard library: tests/owned_host.cpp compiles this against counting stand-ins for the calls below, without a GPU.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace rthost {

// A runtime handle (a pointer type) and the call that releases it.
template <class H, hipError_t (*Release)(H)> struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle &&o) noexcept : h(o.h) { o.h = nullptr; }
    Handle &operator=(Handle &&o) noexcept
    {
        if (this != &o) { reset(); h = o.h; o.h = nullptr; }
        return *this;
    }
    ~Handle() { reset(); }
    void reset()
    {
        if (h) (void)Release(h);
        h = nullptr;
    }
};

// make(): created on first use, kept afterwards
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    hipError_t make(unsigned flags = hipEventDefault) { return h ? hipSuccess : hipEventCreateWithFlags(&h, flags); }
    operator hipEvent_t() const { return h; }
};

struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    hipError_t make(unsigned flags) { return h ? hipSuccess : hipStreamCreateWithFlags(&h, flags); }
    operator hipStream_t() const { return h; }
};

// pinned host memory (hipHostMalloc), as an array of T
template <class T> struct Pinned : Handle<void *, hipHostFree> {
    hipError_t make(size_t bytes, unsigned flags) { reset(); return hipHostMalloc(&h, bytes, flags); }
    operator T *() const { return (T *)h; }
};

// A block of device memory and its size.  make, fit and drop adjust the running total the block is counted in (a scene's
// rtHipSceneBytes) -- nothing else in the library does; the destructor and moves free without counting.
struct DevBlock {
    void *p = nullptr;
    uint64_t size = 0;
    DevBlock() = default;
    DevBlock(DevBlock &&o) noexcept : p(o.p), size(o.size) { o.p = nullptr; o.size = 0; }
    DevBlock &operator=(DevBlock &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; size = o.size; o.p = nullptr; o.size = 0; }
        return *this;
    }
    ~DevBlock() { release(); }
    template <class T> T *as() const { return (T *)p; }
    void drop(uint64_t &total) { total -= size; release(); }
    // Kept when it holds at least `need` bytes; otherwise a block of `want` bytes is allocated FIRST and the old one freed then, so a
    // growth that fails leaves the old block, its size and the total as they were.  Contents are not carried over.
    hipError_t fit(uint64_t need, uint64_t want, uint64_t &total)
    {
        if (p && size >= need) return hipSuccess;
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, want);
        if (e != hipSuccess) { (void)hipGetLastError(); return e; }
        drop(total);
        p = q; size = want;
        total += want;
        return hipSuccess;
    }
    // the old block, if any, is freed first (the two need not fit side by side); empty on failure
    hipError_t make(uint64_t bytes, uint64_t &total) { drop(total); return fit(bytes, bytes, total); }
    // a block made elsewhere (and not counted there) takes this one's place
    void adopt(DevBlock &&o, uint64_t &total) { drop(total); *this = static_cast<DevBlock &&>(o); total += size; }

private:
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; size = 0;
    }
};

// the same, read as an array of T
template <class T = char> struct Dev : DevBlock {
    operator T *() const { return (T *)p; }
};

// Device blocks in the order they were made and the sum of their bytes: one PART of a scene (rt_host.h), or scratch that goes when the
// scope ends.  A part counts into its own sum only; rtHipScene::install and drop_part count that sum into the scene's total.
struct DevPart {
    std::vector<DevBlock> blocks;
    uint64_t bytes = 0;
    DevPart() = default;
    DevPart(DevPart &&o) noexcept : blocks(std::move(o.blocks)), bytes(o.bytes) { o.clear(); }
    DevPart &operator=(DevPart &&o) noexcept
    {
        if (this != &o) { blocks = std::move(o.blocks); bytes = o.bytes; o.clear(); }
        return *this;
    }
    bool empty() const { return blocks.empty(); }
    // a new last block of `n` bytes (one at least), its start in *out; a failure leaves the part as it was
    hipError_t get(void **out, uint64_t n)
    {
        blocks.emplace_back();
        const hipError_t e = blocks.back().make(n ? n : 1, bytes);
        if (e != hipSuccess) blocks.pop_back();
        else *out = blocks.back().p;
        return e;
    }
    // a block made elsewhere (and not counted there) becomes the last one
    void adopt(DevBlock &&b)
    {
        blocks.emplace_back();
        blocks.back().adopt(std::move(b), bytes);
    }
    void clear() { blocks.clear(); bytes = 0; }
};

} // namespace rthost
