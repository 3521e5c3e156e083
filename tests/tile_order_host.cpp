// The tile orders of csrc/rt_tile_order.h on the CPU: both host walkers against a restatement that does not use the header -- every image
// pixel finds its tile and its index in the tile by division -- over image sizes with partial tiles and tile lists in and out of image
// order, and the block-order map as a bijection.  A program of its own (tests/test_tile_order_host.py builds it as-is and under the
// address and undefined-behaviour sanitizers): prints "failures N" and exits non-zero if N > 0.
#include "rt_tile_order.h"

#include <cstdio>
#include <vector>

static int g_failures = 0;
static void fail_at(int line, const char *what, unsigned long long a, unsigned long long b)
{
    if (++g_failures <= 20) printf("line %d: %s (%llu, %llu)\n", line, what, a, b);
}
#define CHECK(cond, what, a, b) do { if (!(cond)) fail_at(__LINE__, what, (unsigned long long)(a), (unsigned long long)(b)); } while (0)

static const uint32_t EDGE = 128, NONE = 0xffffffffu;

// For each image pixel the index of its value in a tile-major plane (slot * EDGE * EDGE + index in the tile), or NONE where its tile is
// not listed: by division, pixel by pixel.  `blocks`: 8 x 8 blocks, 16 per row of blocks, instead of rows.
static std::vector<uint32_t> expected(const std::vector<uint32_t> &ids, uint32_t W, uint32_t H, bool blocks)
{
    const uint32_t tilesX = (W + EDGE - 1) / EDGE;
    std::vector<uint32_t> want((size_t)W * H, NONE);
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint32_t tile = (y / EDGE) * tilesX + x / EDGE, lx = x % EDGE, ly = y % EDGE;
            const uint32_t inTile = blocks ? ((ly / 8) * (EDGE / 8) + lx / 8) * 64 + (ly % 8) * 8 + lx % 8 : ly * EDGE + lx;
            for (size_t s = 0; s < ids.size(); ++s)
                if (ids[s] == tile) want[(size_t)y * W + x] = (uint32_t)(s * EDGE * EDGE + inTile);
        }
    return want;
}

// What a walker stored: every offset inside the image, every listed pixel once with its own index, no other pixel at all.
struct Image {
    std::vector<uint32_t> got, times;
    explicit Image(size_t pixels) : got(pixels, NONE), times(pixels, 0) {}
    void store(size_t at, size_t src)
    {
        if (at >= got.size()) { fail_at(__LINE__, "a store outside the image", at, got.size()); return; }
        got[at] = (uint32_t)src;
        ++times[at];
    }
    void compare(const std::vector<uint32_t> &want, uint32_t W) const
    {
        for (size_t at = 0; at < want.size(); ++at) {
            CHECK(times[at] == (want[at] == NONE ? 0u : 1u), "pixel visited a wrong number of times (x, y)", at % W, at / W);
            CHECK(got[at] == want[at], "pixel read from the wrong index (got, expected)", got[at], want[at]);
        }
    }
};

static void check_case(uint32_t W, uint32_t H, const std::vector<uint32_t> &ids)
{
    const uint32_t tilesX = (W + RT_TILE - 1) / RT_TILE;
    Image rows((size_t)W * H), blocks((size_t)W * H);
    std::vector<uint32_t> rowCalls(ids.size() * RT_TILE, 0);
    rt_tile_walk_rows(ids.data(), ids.size(), tilesX, W, H, [&](size_t s, uint32_t ly, size_t at, uint32_t n) {
        CHECK(s < ids.size() && ly < RT_TILE, "a row outside the slots (slot, row)", s, ly);
        if (s >= ids.size() || ly >= RT_TILE) return;
        CHECK(n >= 1 && n <= RT_TILE, "a row of a wrong length", n, 0);
        ++rowCalls[s * RT_TILE + ly];
        for (uint32_t i = 0; i < n; ++i) rows.store(at + i, s * RT_TILE_PIXELS + (size_t)ly * RT_TILE + i);
    });
    for (uint32_t c : rowCalls) CHECK(c <= 1, "a row called back more than once", c, 0);
    rows.compare(expected(ids, W, H, false), W);
    rt_tile_walk_block_pixels(ids.data(), ids.size(), tilesX, W, H, [&](size_t lp, size_t at) {
        CHECK(lp < ids.size() * RT_TILE_PIXELS, "an index outside the slots", lp, ids.size());
        blocks.store(at, lp);
    });
    blocks.compare(expected(ids, W, H, true), W);
}

int main()
{
    static_assert(RT_TILE == EDGE && RT_TILE_PIXELS == EDGE * EDGE, "the restatement is written for the header's tile");
    const uint32_t sizes[][2] = { { 1, 1 }, { 128, 128 }, { 127, 129 }, { 129, 127 }, { 257, 1 }, { 300, 200 } };
    int cases = 0;
    for (const auto &size : sizes) {
        const uint32_t W = size[0], H = size[1], tiles = ((W + EDGE - 1) / EDGE) * ((H + EDGE - 1) / EDGE);
        std::vector<uint32_t> all, reversed, everyOther, last, none;
        for (uint32_t t = 0; t < tiles; ++t) {
            all.push_back(t);
            reversed.push_back(tiles - 1 - t);
            if (t % 2 == 0) everyOther.push_back(t);
        }
        last.push_back(tiles - 1);
        for (const auto *ids : { &all, &reversed, &everyOther, &last, &none }) { check_case(W, H, *ids); ++cases; }
    }
    // the block order is a bijection of 0 .. RT_TILE_PIXELS - 1 onto the tile's pixels
    std::vector<uint32_t> seen(RT_TILE_PIXELS, 0);
    for (uint32_t q = 0; q < RT_TILE_PIXELS; ++q) {
        uint32_t lx = NONE, ly = NONE;
        rt_tile_block_xy(q, lx, ly);
        CHECK(lx < RT_TILE && ly < RT_TILE, "a block-order pixel outside the tile", lx, ly);
        if (lx < RT_TILE && ly < RT_TILE) ++seen[ly * RT_TILE + lx];
    }
    for (uint32_t p = 0; p < RT_TILE_PIXELS; ++p) CHECK(seen[p] == 1, "a tile pixel without exactly one block-order index", p, seen[p]);
    // a tile's origin
    uint32_t x0 = NONE, y0 = NONE;
    rt_tile_origin(5, 3, x0, y0);
    CHECK(x0 == 2 * EDGE && y0 == 1 * EDGE, "tile 5 of an image 3 tiles wide starts elsewhere", x0, y0);
    printf("cases %d, failures %d\n", cases, g_failures);
    return g_failures ? 1 : 0;
}
