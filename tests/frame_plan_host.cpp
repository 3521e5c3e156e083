// The frame scheduler's arithmetic (csrc/rt_frame_plan.h) on the CPU: known answers worked out by hand from the rules (default tuning,
// RT_WF_SHARDS = 256), then invariants over random inputs.  A program of its own (tests/test_frame_plan_host.py builds it as-is and under
// the address and undefined-behaviour sanitizers): prints "failures N" and exits non-zero if N > 0.
//   usage: frame_plan_host [seed] [random cases]
#include "rt_frame_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace rthost;

static int g_failures = 0;
#define CHECK_EQ(got, want)                                                                                               \
    do {                                                                                                                  \
        const unsigned long long g_ = (unsigned long long)(got), w_ = (unsigned long long)(want);                         \
        if (g_ != w_) { ++g_failures; printf("line %d: %s = %llu, expected %llu\n", __LINE__, #got, g_, w_); }            \
    } while (0)

static void test_mode_for()
{
    static_assert(RT_WF_SHARDS == 256, "the known answers assume 256 shards");
    const Tuning D;
    RtRoundMode m = mode_for(D, 1, 50000, 256);
    CHECK_EQ(m.ordered, 1); CHECK_EQ(m.segLen, 64); CHECK_EQ(m.slices, 256); CHECK_EQ(m.groupRays, 48);
    CHECK_EQ(mode_for(D, 2, 50000, 256).ordered, 0);
    m = mode_for(D, 2, 300000, 256);
    CHECK_EQ(m.ordered, 1); CHECK_EQ(m.segLen, 384); CHECK_EQ(m.groupRays, 64);
    m = mode_for(D, 3, 29999, 256);
    CHECK_EQ(m.segLen, 16); CHECK_EQ(m.groupRays, 32); CHECK_EQ(m.ordered, 0);
    // the other tiers of the cut: >= 700 k never cut, >= 100 k in 96s; round 0's rule is round 1's
    CHECK_EQ(mode_for(D, 2, 700000, 256).segLen, 4096);
    CHECK_EQ(mode_for(D, 2, 100000, 256).segLen, 96);
    CHECK_EQ(mode_for(D, 0, 1, 256).ordered, 1);
    CHECK_EQ(mode_for(D, 2, 0, 256).groupRays, 16);
    { Tuning T; T.orderedFirst = 0; CHECK_EQ(mode_for(T, 1, 299999, 256).ordered, 0); CHECK_EQ(mode_for(T, 1, 300000, 256).ordered, 1); }
    { Tuning T; T.segLen[4] = 0; CHECK_EQ(mode_for(T, 3, 10, 256).segLen, 1); }
    {
        Tuning T; T.sliceRays = 1000; T.smallSlices = 3; // (3 is no power of two: 16)
        CHECK_EQ(mode_for(T, 2, 999, 256).slices, 16);
        CHECK_EQ(mode_for(T, 2, 999, 8).slices, 8);
        CHECK_EQ(mode_for(T, 2, 1000, 256).slices, 256);
        T.smallSlices = 4; CHECK_EQ(mode_for(T, 2, 999, 256).slices, 4);
        T.smallSlices = 512; CHECK_EQ(mode_for(T, 2, 999, 256).slices, 16);
        T.smallSlices = 0; CHECK_EQ(mode_for(T, 2, 999, 256).slices, 16);
    }
    { Tuning T; T.groupRays = 128; CHECK_EQ(mode_for(T, 3, 29999, 256).groupRays, 128); }
    { Tuning T; T.groupRays = 129; CHECK_EQ(mode_for(T, 3, 29999, 256).groupRays, 32); }
}

static void test_trace_blocks()
{
    const RtRoundMode ordered{ 1u, 64u, 48u, 256u }, loose{ 0u, 64u, 16u, 256u };
    const uint32_t traceBlocks = 100000, capacity = 1u << 20, extraCap = 6u << 20;
    RoundPlan P; P.rays = 1000; P.extra = 0; P.extraSegLen = 64;
    CHECK_EQ(trace_blocks(true, 2, ordered, P, traceBlocks, capacity, extraCap, false), 13);  // (1100 + 255) / 256 + 8
    CHECK_EQ(trace_blocks(true, 2, loose, P, traceBlocks, capacity, extraCap, false), 589);   // (1100 + 15) / 16 + 512 + 8
    // capped by the worst case: traceBlocks, or 2 * capacity / groupRays + 2 * slices
    CHECK_EQ(trace_blocks(true, 2, ordered, P, 7, capacity, extraCap, false), 7);
    CHECK_EQ(trace_blocks(true, 2, loose, P, traceBlocks, 256, extraCap, false), 2 * 256 / 16 + 512);
    CHECK_EQ(trace_blocks(true, 2, ordered, P, traceBlocks, capacity, extraCap, true), 1);
    CHECK_EQ(trace_blocks(true, 2, loose, P, traceBlocks, capacity, extraCap, true), 1);
    // round >= 64 or not planned: the worst case, at most 0x7fffffff
    CHECK_EQ(trace_blocks(true, 64, ordered, P, traceBlocks, capacity, extraCap, true), traceBlocks);
    CHECK_EQ(trace_blocks(false, 2, ordered, P, traceBlocks, capacity, extraCap, true), traceBlocks);
    CHECK_EQ(trace_blocks(false, 2, loose, P, traceBlocks, capacity, extraCap, false), 2 * capacity / 16 + 512);
    CHECK_EQ(trace_blocks(false, 2, ordered, P, 0xfffffff0u, capacity, extraCap, false), 0x7fffffffu);
    { RtRoundMode one = loose; one.groupRays = 1; CHECK_EQ(trace_blocks(false, 2, one, P, traceBlocks, 0x7ffffff0u, extraCap, false), 0x7fffffffu); }
    // the plan's further segments: as logged under the same cut ...
    { RoundPlan Q = P; Q.extra = 3000; CHECK_EQ(trace_blocks(true, 2, ordered, Q, traceBlocks, capacity, extraCap, false), 26); } // (4400 + 255) / 256 + 8
    { RoundPlan Q = P; Q.extra = 3000; CHECK_EQ(trace_blocks(true, 2, ordered, Q, traceBlocks, capacity, 1000, false), 17); }     // (2200 + 255) / 256 + 8
    // ... under another cut none where rays are never cut, else min(extraCap, 11 * rays)
    RoundPlan Q = P; Q.extraSegLen = 96; Q.extra = 5;
    { RtRoundMode whole = ordered; whole.segLen = 4096; CHECK_EQ(trace_blocks(true, 2, whole, Q, traceBlocks, capacity, extraCap, false), 13); }
    CHECK_EQ(trace_blocks(true, 2, ordered, Q, traceBlocks, capacity, extraCap, false), 60);  // (12000 * 11 / 10 + 255) / 256 + 8
    CHECK_EQ(trace_blocks(true, 2, ordered, Q, traceBlocks, capacity, 5000, false), 34);      // (6000 * 11 / 10 + 255) / 256 + 8
    Q.extraSegLen = 0xffffffffu;
    CHECK_EQ(trace_blocks(true, 2, ordered, Q, traceBlocks, capacity, extraCap, false), 60);
    CHECK_EQ(trace_blocks(true, 2, loose, Q, traceBlocks, capacity, extraCap, false), 589);   // (a round that is not ordered has no region B)
    CHECK_EQ(trace_blocks(true, 2, ordered, RoundPlan(), traceBlocks, capacity, extraCap, false), 8);
}

static void test_shade_blocks()
{
    const RtRoundMode m{ 0u, 64u, 16u, 256u };
    RoundPlan P;
    CHECK_EQ(shade_blocks(true, 1, m, P, 2048, false), 0);
    P.shade = 1000;   CHECK_EQ(shade_blocks(true, 1, m, P, 2048, false), 64);   // 13 per slice: a wave each, 256 waves = 64 workgroups
    P.shade = 100000; CHECK_EQ(shade_blocks(true, 1, m, P, 2048, false), 448);  // 438 per slice: 7 waves each, 1792 waves
    CHECK_EQ(shade_blocks(true, 1, m, P, 128, false), 128);
    P.shade = 1000;   CHECK_EQ(shade_blocks(true, 1, m, P, 0, false), 0);
    CHECK_EQ(shade_blocks(true, 1, m, P, 2048, true), 0);
    CHECK_EQ(shade_blocks(false, 1, m, P, 2048, true), 2048);
    CHECK_EQ(shade_blocks(true, 64, m, P, 2048, true), 2048);
    { RtRoundMode few = m; few.slices = 16; CHECK_EQ(shade_blocks(true, 1, few, P, 2048, false), 64); } // 77 per slice: 2 waves each, 32 waves, one unit
}

static void test_round_runs_split()
{
    CHECK_EQ(round_runs_split(1, 1, 1, RT_PATH_CLASS_OPAQUE_DIFFUSE), 1);
    CHECK_EQ(round_runs_split(0, 1, 1, RT_PATH_CLASS_OPAQUE_DIFFUSE), 0);
    CHECK_EQ(round_runs_split(1, 0, 1, RT_PATH_CLASS_OPAQUE_DIFFUSE), 0);
    CHECK_EQ(round_runs_split(1, 1, 0, RT_PATH_CLASS_OPAQUE_DIFFUSE), 0);
    CHECK_EQ(round_runs_split(1, 1, 1, RT_PATH_CLASS_GENERAL), 0);
}

static void test_fold_and_adopt()
{
    std::vector<uint4> log(RT_WF_ROUND_LOG, uint4{ 0, 0, 0, 0 });
    log[1] = uint4{ 5000, 40, 700, 90 };
    log[2] = uint4{ 300, 9, 20, 0 };
    std::vector<RtRoundMode> modes(7, RtRoundMode{ 0u, 64u, 16u, 256u });
    modes[1].segLen = 96;
    std::vector<RoundPlan> next(RT_WF_ROUND_LOG), plan(RT_WF_ROUND_LOG);
    uint32_t needed = 0;
    fold_round_log(log.data(), modes.data(), modes.size(), 6, next.data(), &needed);
    CHECK_EQ(needed, 3);
    CHECK_EQ(next[1].rays, 5000); CHECK_EQ(next[1].extra, 700); CHECK_EQ(next[1].extraSegLen, 96); CHECK_EQ(next[1].shade, 90);
    CHECK_EQ(next[2].rays, 300); CHECK_EQ(next[2].extra, 20); CHECK_EQ(next[2].extraSegLen, 64);
    CHECK_EQ(next[7].extraSegLen, 4096); CHECK_EQ(next[7].rays, 0); // (a round the batch never laid out)
    // a second, smaller batch cut the same: the maximum stays, and so does the rounds figure
    std::vector<uint4> log2 = log;
    log2[1] = uint4{ 4000, 30, 900, 10 }; log2[2] = uint4{ 0, 0, 0, 0 };
    fold_round_log(log2.data(), modes.data(), modes.size(), 3, next.data(), &needed);
    CHECK_EQ(needed, 3);
    CHECK_EQ(next[1].rays, 5000); CHECK_EQ(next[1].extra, 900); CHECK_EQ(next[1].shade, 90);
    // a third cut round 1 differently: no figure for its further segments, the one logged is left alone
    modes[1].segLen = 384;
    log2[1] = uint4{ 6000, 30, 5000, 10 };
    fold_round_log(log2.data(), modes.data(), modes.size(), 3, next.data(), &needed);
    CHECK_EQ(next[1].extraSegLen, 0xffffffffu); CHECK_EQ(next[1].extra, 900); CHECK_EQ(next[1].rays, 6000);
    fold_round_log(log2.data(), modes.data(), modes.size(), 3, next.data(), &needed);
    CHECK_EQ(next[1].extraSegLen, 0xffffffffu); CHECK_EQ(next[1].extra, 900);
    // rounds beyond the log: every one of them
    { uint32_t n = 0; std::vector<RoundPlan> tmp(RT_WF_ROUND_LOG); fold_round_log(log.data(), modes.data(), modes.size(), 70, tmp.data(), &n); CHECK_EQ(n, 70); }
    { uint32_t n = 0; std::vector<RoundPlan> tmp(RT_WF_ROUND_LOG); fold_round_log(log.data(), modes.data(), modes.size(), 2, tmp.data(), &n); CHECK_EQ(n, 2); } // (round 2 never ran)
    { uint32_t n = 9; std::vector<RoundPlan> tmp(RT_WF_ROUND_LOG); fold_round_log(log.data(), modes.data(), modes.size(), 6, tmp.data(), &n); CHECK_EQ(n, 9); }

    // for the frame's further batches: a tenth more, the figures stay for the batches to come, one spare round
    const uint32_t need = adopt_plan(plan.data(), next.data(), &needed, true);
    CHECK_EQ(need, 3); CHECK_EQ(needed, 3);
    CHECK_EQ(plan[1].rays, 6600); CHECK_EQ(plan[1].extra, 990); CHECK_EQ(plan[1].shade, 99); CHECK_EQ(plan[1].extraSegLen, 0xffffffffu);
    CHECK_EQ(plan[2].rays, 330); CHECK_EQ(plan[2].extra, 22);
    CHECK_EQ(next[1].rays, 6000);
    CHECK_EQ(plan_rounds(need, true, 0), 4);
    // at the frame's end: as logged, and the next watched frame starts from nothing
    CHECK_EQ(adopt_plan(plan.data(), next.data(), &needed, false), 3);
    CHECK_EQ(needed, 0);
    CHECK_EQ(plan[1].rays, 6000); CHECK_EQ(plan[1].extra, 900); CHECK_EQ(plan[1].shade, 90);
    CHECK_EQ(next[1].rays, 0); CHECK_EQ(next[1].extraSegLen, 0); CHECK_EQ(next[2].extra, 0);
    CHECK_EQ(plan_rounds(3, false, 0), 3);
    CHECK_EQ(plan_rounds(3, true, 0), 4);
    CHECK_EQ(plan_rounds(3, false, 1), 1);
    CHECK_EQ(plan_rounds(3, true, 1), 1);
    CHECK_EQ(plan_rounds(1, false, 5), 1);
}

static void test_random(uint32_t seed, int cases)
{
    std::mt19937 rng(seed);
    auto upto = [&](uint32_t hi) { return (uint32_t)(rng() % ((uint64_t)hi + 1)); };
    for (int i = 0; i < cases; ++i) {
        Tuning T;
        if (i & 1) { T.groupRays = upto(130); T.sliceRays = upto(100000); T.smallSlices = 1u << upto(9); T.orderedFirst = upto(1); T.segLen[upto(4)] = upto(5000); }
        const uint32_t round = 1 + upto(70), capacity = 256u * (1 + upto(1u << 14)), extraCap = capacity * (1 + upto(15));
        const uint32_t traceBlocks = (2 * capacity + extraCap) / 256;
        const uint64_t rays = upto(1) ? upto(2 * capacity) : upto(3000);
        const RtRoundMode m = mode_for(T, round, rays, 1u << upto(8));
        RoundPlan P;
        P.rays = (uint32_t)rays; P.extra = upto(extraCap); P.shade = upto(capacity);
        P.extraSegLen = upto(2) == 0 ? m.segLen : (upto(1) ? 0xffffffffu : upto(5000));
        const uint64_t worst = trace_blocks(false, round, m, P, traceBlocks, capacity, extraCap, false);
        const uint64_t got = trace_blocks(true, round, m, P, traceBlocks, capacity, extraCap, false);
        if (got < 1 || got > worst) { ++g_failures; printf("case %d: trace grid %llu outside 1 .. %llu\n", i, (unsigned long long)got, (unsigned long long)worst); }
        RoundPlan Q = P; Q.rays += upto(5000);
        const uint64_t more = trace_blocks(true, round, m, Q, traceBlocks, capacity, extraCap, false);
        if (more < got) { ++g_failures; printf("case %d: trace grid falls from %llu to %llu with more rays\n", i, (unsigned long long)got, (unsigned long long)more); }
        const uint32_t logicBlocks = 64 * (1 + upto(40)), r = round % RT_WF_ROUND_LOG; // (a planned round: below RT_WF_ROUND_LOG)
        const uint32_t shade = shade_blocks(true, r, m, P, logicBlocks, false);
        if (shade % 64 || shade > logicBlocks || (shade == 0) != (P.shade == 0)) { ++g_failures; printf("case %d: shade grid %u (listed %u, logic grid %u)\n", i, shade, P.shade, logicBlocks); }
        Q = P; Q.shade += upto(5000);
        if (shade_blocks(true, r, m, Q, logicBlocks, false) < shade) { ++g_failures; printf("case %d: shade grid falls with a longer list\n", i); }
        if (m.segLen < 1 || m.groupRays < 1 || m.groupRays > 128 || m.slices < 1 || m.slices > RT_WF_SHARDS || (m.slices & (m.slices - 1))) { ++g_failures; printf("case %d: mode out of range\n", i); }
    }
}

int main(int argc, char **argv)
{
    const uint32_t seed = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 10) : 1u;
    const int cases = argc > 2 ? atoi(argv[2]) : 4000;
    test_mode_for();
    test_trace_blocks();
    test_shade_blocks();
    test_round_runs_split();
    test_fold_and_adopt();
    test_random(seed, cases);
    printf("failures %d\n", g_failures);
    return g_failures ? 1 : 0;
}
