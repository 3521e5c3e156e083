// rt_frame_plan.h -- the arithmetic of the frame scheduler (rt_frame.cpp, render_wavefront): how a round is laid out, how large a planned
// round's launches are, and how a watched batch's round log becomes the plan of the batches and frames to come.  Plain functions of their
// arguments: no HIP runtime call, no scene, no globals -- tests/frame_plan_host.cpp checks them on the CPU (test_frame_plan_host.py), since
// a mistake here otherwise shows only on the device, as RT_WF_ERR_GRID or a frame rendered twice.
#pragma once
#include "rt_device.h"
#include "rt_tuning.h"

#include <algorithm>
#include <stddef.h>
#include <stdint.h>

namespace rthost {

// per round: rays (entries in region A), the longest queue slice, entries in region B -- the maximum over the watched batches
// rays of the round, and -- an ordered round -- the further segments of its cut rays under the cut it was logged with
// and -- a split logic round -- the paths it listed for its shade pass
struct RoundPlan { uint32_t rays = 0, extra = 0, extraSegLen = 0, shade = 0; };

// How a round with `rays` rays is laid out (RtRoundMode, rt_device.h): big rounds are ordered by predicted walk length and spread
// their appends over all queue slices, small ones are cut into segments and keep their entries dense.
inline RtRoundMode mode_for(const Tuning &T, uint32_t round, uint64_t rays, uint32_t slicesBefore)
{
    RtRoundMode m;
    // planned where the rays are made (and ordered) when most paths make one: the round behind the primary hits, and any big round
    m.ordered = (round <= 1u || rays >= T.appendRays) ? 1u : 0u;
    if (T.orderedFirst == 0u && rays < T.appendRays) m.ordered = 0u;
    m.segLen = rays >= T.segRays[0] ? T.segLen[0] : (rays >= T.segRays[1] ? T.segLen[1] : (rays >= T.segRays[2] ? T.segLen[2] : (rays >= T.segRays[3] ? T.segLen[3] : T.segLen[4])));
    if (m.segLen < 1u) m.segLen = 1u;
    uint32_t small = T.smallSlices;
    if (small < 1u || small > RT_WF_SHARDS || (small & (small - 1u))) small = 16u;
    m.slices = rays >= T.sliceRays ? (uint32_t)RT_WF_SHARDS : small;
    if (m.slices > slicesBefore) m.slices = slicesBefore; // a slice holds at most the paths of its shards: slices only ever merge
    // rays per workgroup of the trace kernel: about 256 lanes / the segments a ray of this round is expected to be cut into ...
    // ... and few enough workgroups for all of them to run at once (5 per CU): the round lasts as long as its slowest workgroup
    // (at most 64: with 128 -- two segments per ray on average fill the 256 lanes -- every second workgroup has to cut coarser, and its
    // longer segments are the round's duration: 4K, 232 k rays, 403 us against 273)
    m.groupRays = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(16, ((rays + 1099) / 1100 + 15) / 16 * 16));
    if (T.groupRays >= 1u && T.groupRays <= 128u) m.groupRays = T.groupRays;
    return m;
}

// Workgroups of round r's trace launch.  `planned`: the batch is issued from a plan, whose entry for the round is P (rounds from
// RT_WF_ROUND_LOG on have none); traceBlocks, capacity, extraCap: the tile group's (rtHipScene::Group, RtWavefront).
inline uint32_t trace_blocks(bool planned, uint32_t r, const RtRoundMode &m, const RoundPlan &P, uint32_t traceBlocks, uint32_t capacity, uint32_t extraCap,
                             bool planGridTiny)
{
    // worst case: every queue slot in use -- an ordered round takes 256 entries per workgroup, any other mode.groupRays rays of
    // one queue slice (every slice's last piece may be a partial one)
    const uint64_t worst = m.ordered ? traceBlocks : 2ull * capacity / m.groupRays + 2ull * m.slices;
    if (!planned || r >= RT_WF_ROUND_LOG) return (uint32_t)std::min<uint64_t>(worst, 0x7fffffffu);
    if (planGridTiny) return 1;
    // the same frame gave this many rays last time: a tenth more plus a few, never more than the worst case
    // (an ordered round's further segments: as many as last time if the cut is the same -- a watched frame guesses the round's size
    // and with it the cut -- and at most RT_WF_MAXSEG - 1 per ray whatever the cut)
    const uint64_t rays = P.rays;
    const uint64_t extra = std::min<uint64_t>(extraCap, P.extraSegLen == m.segLen ? P.extra : (m.segLen >= 4096u ? 0 : rays * 11));
    const uint64_t want = m.ordered ? ((rays + extra) * 11 / 10 + 255) / 256 + 8 : (rays * 11 / 10 + m.groupRays - 1) / m.groupRays + 2ull * m.slices + 8;
    return (uint32_t)std::max<uint64_t>(std::min<uint64_t>(want, worst), 1);
}

// workgroups of a split round's shade pass (0: not launched).  Its waves stride over their slice's list, so any whole number of waves
// per slice is enough; a planned frame launches as many as the list the plan logged fills once -- a tenth more plus a few, like a
// round's rays, spread over the slices -- and a watched one the logic kernel's grid.
inline uint32_t shade_blocks(bool planned, uint32_t r, const RtRoundMode &m, const RoundPlan &P, uint32_t logicBlocks, bool planShadeSkip)
{
    if (!planned || r >= RT_WF_ROUND_LOG) return logicBlocks;
    const uint64_t listed = planShadeSkip ? 0 : P.shade;
    if (listed == 0) return 0;
    const uint64_t perSlice = (listed * 11 / 10 + m.slices - 1) / m.slices + 8;
    const uint64_t waves = (perSlice + 63) / 64 * m.slices, unit = RT_WF_SHARDS / 4;
    return (uint32_t)std::min<uint64_t>(logicBlocks, ((waves + 3) / 4 + unit - 1) / unit * unit);
}

// A later round of the opaque-diffuse class with look-ahead on (Tuning::logicSplit): the answers as a stream (wf_answer_kernel), then the
// paths whose bounce hit something shaded by dense waves (wf_shade_kernel).
inline bool round_runs_split(uint32_t r, uint32_t logicSplit, uint32_t lookAhead, uint32_t pathClass)
{
    return r > 0 && logicSplit && lookAhead && pathClass == RT_PATH_CLASS_OPAQUE_DIFFUSE;
}

// What the host knows of a round's placement table (rt_device.h, RT_WF_PLACE_*) without reading it: the layout wf_scatter_kernel last
// recorded it under, and whether that launch belongs to the scene state, sample window and plan in force -- a watched frame, which
// everything that changes a frame's rays forces, forgets every stamp before its own scatter launches make new ones.
// windowTotal, windowFirst: the sample window of the frame that recorded it (rtHipSampleWindow: N and f name the frame's sample ids, and
// with them its rays).  A set window keeps the launch plan, so the next frame is a planned one: it scatters, and records anew.
struct PlaceStamp { uint32_t slices = 0, segLen = 0, windowTotal = 0, windowFirst = 0; bool valid = false; };

// Round r's entries are written at their sorted positions by the logic kernel that makes them, from the round's placement table, and the
// round runs no scatter launch (RT_ROUND_DIRECT).  Only where the table is known to be this frame's and nothing reads entries by queue slot:
//   planned, ordered, one of the rounds that have a table;
//   uncut (region B is empty, no segment patches another's entry by position);
//   slices >= 32: the histogram copy, wave id % RT_WF_SORT_COPIES, is then a function of the path's shard (the wave serves slice
//     wave id % slicesIn, slicesIn >= slices a power of two), so a cell holds the same rays whatever the scheduling;
//   the opaque-diffuse class (the general machine reads an answered entry back by its slot), visit_log off (that hook does too);
//   one sample batch per frame (the table is one batch's);
//   a valid stamp that equals the round's mode and the frame's sample window.
inline bool round_goes_direct(bool planned, uint32_t r, const RtRoundMode &m, uint32_t pathClass, uint32_t placeDirect, uint32_t visitLog, uint32_t batches,
                              const PlaceStamp &stamp, uint32_t windowTotal, uint32_t windowFirst)
{
    return placeDirect && planned && r >= 1u && r <= RT_WF_PLACE_ROUNDS && m.ordered && m.segLen >= 4096u && m.slices >= 32u &&
           pathClass == RT_PATH_CLASS_OPAQUE_DIFFUSE && !visitLog && batches == 1u && stamp.valid && stamp.slices == m.slices && stamp.segLen == m.segLen &&
           stamp.windowTotal == windowTotal && stamp.windowFirst == windowFirst;
}

// The table wf_scatter_kernel records from a round's histogram hist[copy][bin]: cell (bin, copy), stored at bin * RT_WF_SORT_COPIES + copy,
// gets {first sorted position, entries} -- the cells in that order, class 0 (the longest walks) first, each starting where the one before
// ends.  Returns the total.  The host's statement of the kernel's arithmetic (tests/place_plan_host.cpp, test_place_direct_gpu.py).
inline uint32_t place_table(const uint32_t *hist, uint32_t *cells)
{
    uint32_t at = 0;
    for (uint32_t b = 0; b < RT_WF_SORT_BINS; ++b)
        for (uint32_t c = 0; c < RT_WF_SORT_COPIES; ++c) {
            const uint32_t n = hist[c * RT_WF_SORT_BINS + b];
            cells[2 * (b * RT_WF_SORT_COPIES + c)] = at;
            cells[2 * (b * RT_WF_SORT_COPIES + c) + 1] = n;
            at += n;
        }
    return at;
}

// A watched batch that took `rounds` rounds, laid out as modes[0 .. modeCount), has ended and left `log` (RtWavefront::roundLog):
// the plan for the batches and frames to come: the rounds that had anything to trace (+ the logic round that consumed
// the last answers), and every round's sizes
inline void fold_round_log(const uint4 *log, const RtRoundMode *modes, size_t modeCount, uint32_t rounds, RoundPlan *planNext, uint32_t *roundsNeeded)
{
    uint32_t needed = 1; // logic(0) always runs
    for (uint32_t r = 1; r < std::min<uint32_t>(rounds, RT_WF_ROUND_LOG); ++r)
        if (log[r].x) needed = r + 1;
    if (rounds > RT_WF_ROUND_LOG) needed = rounds;
    *roundsNeeded = std::max(*roundsNeeded, needed);
    for (uint32_t r = 0; r < RT_WF_ROUND_LOG; ++r) {
        RoundPlan &N = planNext[r]; // the maximum over the watched batches
        N.rays = std::max(N.rays, log[r].x);
        N.shade = std::max(N.shade, log[r].w);
        const uint32_t seg = r < modeCount ? modes[r].segLen : 4096u;
        if (N.extraSegLen != seg && N.extraSegLen != 0u) N.extraSegLen = 0xffffffffu; // (batches cut differently: no figure)
        else { N.extraSegLen = seg; N.extra = std::max(N.extra, log[r].z); }
    }
}

// What a tile group's watched batches left (planNext, *roundsNeeded) becomes its plan; returns the rounds the group needed.
// furtherBatches: for the further batches of the frame being watched -- the same pixels with other sample ids, statistically the same
// rounds: a tenth more than the largest batch so far saw (trace_blocks adds its own tenth), and the batches to come keep folding.
// Otherwise, at the end of a watched frame, for the frames to come: as logged, and the group starts its next watched frame from nothing.
inline uint32_t adopt_plan(RoundPlan *plan, RoundPlan *planNext, uint32_t *roundsNeeded, bool furtherBatches)
{
    const uint32_t need = *roundsNeeded;
    for (uint32_t r = 0; r < RT_WF_ROUND_LOG; ++r) {
        plan[r] = planNext[r];
        if (furtherBatches) { plan[r].rays += plan[r].rays / 10; plan[r].extra += plan[r].extra / 10; plan[r].shade += plan[r].shade / 10; }
        else planNext[r] = RoundPlan();
    }
    if (!furtherBatches) *roundsNeeded = 0;
    return need;
}

// Rounds a planned batch issues when its groups needed `need` (the maximum over them, at least 1).  spare: one round more -- a later
// batch's deepest path may go one bounce further.  cap: Tuning::planRounds at the end of a watched frame (0 = none).
inline uint32_t plan_rounds(uint32_t need, bool spare, uint32_t cap)
{
    if (spare) need += 1;
    return cap ? std::min(need, cap) : need;
}

} // namespace rthost
