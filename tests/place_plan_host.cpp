// place_plan_host.cpp -- direct placement's host arithmetic (csrc/rt_frame_plan.h) without a GPU: round_goes_direct over the product of
// its inputs against the rule written out condition by condition, and place_table against a plain re-implementation (sort the cells'
// keys, add up).  A program of its own: test_place_plan_host.py builds it as it is and under the address and undefined-behaviour
// sanitizers, and runs it.
#include "rt_frame_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace rthost;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; if (failures < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static void decision()
{
    const uint32_t rounds[] = { 0, 1, 2, RT_WF_PLACE_ROUNDS, RT_WF_PLACE_ROUNDS + 1, 63 };
    const uint32_t segs[] = { 16, 384, 4095, 4096, 5000 }, slices[] = { 1, 16, 32, 64, 256 };
    const uint32_t classes[] = { RT_PATH_CLASS_GENERAL, RT_PATH_CLASS_OPAQUE_DIFFUSE };
    unsigned long cases = 0, direct = 0;
    for (int planned = 0; planned < 2; ++planned)
    for (uint32_t r : rounds)
    for (uint32_t ordered = 0; ordered < 2; ++ordered)
    for (uint32_t seg : segs)
    for (uint32_t sl : slices)
    for (uint32_t pc : classes)
    for (uint32_t place = 0; place < 2; ++place)
    for (uint32_t visit = 0; visit < 2; ++visit)
    for (uint32_t batches = 1; batches < 4; ++batches)
    for (int stamp = 0; stamp < 6; ++stamp) {
        RtRoundMode m{ ordered, seg, 64u, sl };
        // 0: the round's stamp; 1: not valid; 2: other slices; 3: other segLen; 4: another window's total; 5: another window's first
        PlaceStamp st{ sl, seg, 8u, 2u, true };
        if (stamp == 1) st.valid = false;
        if (stamp == 2) st.slices = sl == 256u ? 128u : sl * 2u;
        if (stamp == 3) st.segLen = seg + 1u;
        if (stamp == 4) st.windowTotal = 4u;
        if (stamp == 5) st.windowFirst = 0u;
        bool want = true;
        if (!place || !planned || !ordered) want = false;
        if (r < 1u || r > RT_WF_PLACE_ROUNDS) want = false;
        if (seg < 4096u) want = false;           // a cut round patches entries by position
        if (sl < 32u) want = false;              // the histogram copy is a function of the shard only from 32 slices on
        if (pc != RT_PATH_CLASS_OPAQUE_DIFFUSE) want = false;
        if (visit || batches != 1u) want = false;
        if (stamp != 0) want = false;
        const bool got = round_goes_direct(planned != 0, r, m, pc, place, visit, batches, st, 8u, 2u);
        CHECK(got == want, "round_goes_direct(planned %d, r %u, ordered %u, seg %u, slices %u, class %u, place %u, visit %u, batches %u, stamp %d) = %d",
              planned, r, ordered, seg, sl, pc, place, visit, batches, stamp, (int)got);
        ++cases; direct += got;
    }
    CHECK(direct > 0 && direct * 50 < cases, "%lu of %lu cases go direct", direct, cases);
    // a default stamp (a scene's first frames, a clone) never admits a round, whatever the mode
    CHECK(!round_goes_direct(true, 1, RtRoundMode{ 1u, 4096u, 64u, 256u }, RT_PATH_CLASS_OPAQUE_DIFFUSE, 1, 0, 1, PlaceStamp(), 0u, 0u), "a default stamp went direct");
    std::printf("decision: %lu cases, %lu direct\n", cases, direct);
}

static void table(uint32_t seed, uint32_t most, uint32_t emptyShare)
{
    std::mt19937 rng(seed);
    std::vector<uint32_t> hist(RT_WF_SORT_COPIES * RT_WF_SORT_BINS), cells(2 * RT_WF_PLACE_CELLS, 0xdeadbeefu);
    for (uint32_t &h : hist) h = (rng() % 100u < emptyShare) ? 0u : rng() % (most + 1u);
    const uint32_t total = place_table(hist.data(), cells.data());
    // plainly: the cells in the order (class, copy), class 0 -- the longest walks -- first; each starts where those before it end
    uint64_t sum = 0;
    for (uint32_t key = 0; key < RT_WF_PLACE_CELLS; ++key) {
        const uint32_t bin = key / RT_WF_SORT_COPIES, copy = key % RT_WF_SORT_COPIES, n = hist[copy * RT_WF_SORT_BINS + bin];
        uint64_t before = 0;
        for (uint32_t b = 0; b < RT_WF_SORT_BINS; ++b)
            for (uint32_t c = 0; c < RT_WF_SORT_COPIES; ++c)
                if (b < bin || (b == bin && c < copy)) before += hist[c * RT_WF_SORT_BINS + b];
        CHECK(cells[2 * key] == before && cells[2 * key + 1] == n, "seed %u cell (%u, %u): {%u, %u}, expected {%llu, %u}", seed, bin, copy, cells[2 * key],
              cells[2 * key + 1], (unsigned long long)before, n);
        sum += n;
    }
    CHECK(total == sum, "seed %u: total %u, the counts add up to %llu", seed, total, (unsigned long long)sum);
    // the runs tile [0, total): no two cells share a position and none is left out
    std::vector<uint8_t> used(total, 0);
    for (uint32_t key = 0; key < RT_WF_PLACE_CELLS; ++key)
        for (uint32_t i = 0; i < cells[2 * key + 1]; ++i) {
            const uint32_t at = cells[2 * key] + i;
            CHECK(at < total && !used[at], "seed %u: position %u is outside [0, %u) or taken twice", seed, at, total);
            if (at < total) used[at] = 1;
        }
}

int main()
{
    static_assert(RT_WF_PLACE_WORDS == 2 * RT_WF_PLACE_CELLS + 4 && RT_WF_PLACE_TOTAL == 2 * RT_WF_PLACE_CELLS, "the table's tail follows its cells");
    static_assert((3 * RT_WF_CTL_WORDS) % 2 == 0 && RT_WF_PLACE_WORDS % 2 == 0, "the cells are read as 8-byte pairs");
    decision();
    table(1, 0, 0);       // an empty round
    table(2, 1, 90);      // nearly empty shards: most cells hold nothing
    table(3, 40, 10);
    table(4, 5000, 50);
    std::printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
