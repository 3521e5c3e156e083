// rt_frame.cpp -- the frame loop of libraytrace_hip.so: one frame through the staged pipeline (render_wavefront) and the check behind
// planned frames (frame_finish).  What a round launches and how large is rt_frame_plan.h's arithmetic; the kernels are in rt_wavefront.hip.
#include "rt_host.h"
#include "rt_launch.h"

#include <cmath>
#include <cstdlib>

using namespace rthost;

namespace {

using Group = rtHipScene::Group;

// The running state of a frame being issued.
struct FrameState {
    bool planned;            // per batch: a watched frame's further batches follow its first batch's plan (Tuning::batchPlan)
    uint32_t planRounds;     // rounds a planned batch issues
    uint64_t splitRounds = 0; // logic rounds issued as answer + shade launches, over the batches and groups
    bool anyPlannedBatch = false;
    uint32_t directRounds = 0, scatterLaunches = 0; // ordered rounds placed directly / scatter launches issued, over the batches and groups
};

// Stage timing on: `launch` between two events of its own on `on`, counted under stage `which` (rtHipStageTimes).
template <class Launch> hipError_t stage(rtHipScene *sc, int which, hipStream_t on, Launch &&launch)
{
    if (!sc->stageTiming) return launch();
    if (sc->stageEventsUsed == sc->stageEvents.size()) {
        rtHipScene::StageEvent e{};
        hipError_t er = e.a.make();
        if (er != hipSuccess) return er;
        er = e.b.make();
        if (er != hipSuccess) return er;
        sc->stageEvents.push_back(std::move(e));
    }
    rtHipScene::StageEvent &e = sc->stageEvents[sc->stageEventsUsed++];
    e.stage = which;
    hipError_t er = hipEventRecord(e.a, on);
    if (er != hipSuccess) return er;
    er = launch();
    if (er != hipSuccess) return er;
    return hipEventRecord(e.b, on);
}

// The error text of RT_WF_ERR_* bits a tile group's kernels raised (RT_WF_STATUS_ERROR); -1.
int device_error(uint32_t err)
{
    return fail("wavefront pipeline: device error 0x%x%s -- the frame is invalid", err,
                (err & RT_WF_ERR_SPIN) ? " (wf_trace_kernel's walk guard tripped: rays were abandoned)" : "");
}

// TEST ONLY (tuning key visit_log; include/raytrace_hip.h, rtHipTestRoundVisits).  Round r of group G, once its trace launch is issued on
// `on` and before logic(r) consumes its answers and logic(r + 1) overwrites its entries: wait for the stream, read the round's queues back
// and add what they hold to sc->visitLog[r].  The entries are the ones the planning kernels wrote (rt_device.h, RtWavefront::ent).
int log_round_visits(rtHipScene *sc, Group &G, uint32_t r, const RtRoundMode &mode, hipStream_t on)
{
    const RtWavefront &W = G.wf;
    HIP_OK(hipStreamSynchronize(on));
    std::vector<uint32_t> ctl(RT_WF_CTL_WORDS);
    std::vector<float> planes(3 * (RT_GRID_DIV + 1));
    HIP_OK(hipMemcpy(ctl.data(), W.ctl + (size_t)(r % 3) * RT_WF_CTL_WORDS, sizeof(uint32_t) * RT_WF_CTL_WORDS, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(planes.data(), G.dev.boxMin, sizeof(float) * planes.size(), hipMemcpyDeviceToHost));
    const uint32_t cap = W.capacity, sliceCap = cap / mode.slices;
    const uint32_t extra = mode.ordered ? std::min(ctl[RT_WF_CTL_EXTRA], W.extraCap) : 0u;
    std::vector<uint4> ent((size_t)4 * (2 * (size_t)cap + extra));
    std::vector<unsigned long long> key(2 * (size_t)cap);
    std::vector<uint2> pathOf(cap);
    HIP_OK(hipMemcpy(ent.data(), W.ent[r & 1u], sizeof(uint4) * ent.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(key.data(), W.hitKey[r & 1u], sizeof(unsigned long long) * key.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(pathOf.data(), W.pathOf[r & 1u], sizeof(uint2) * pathOf.size(), hipMemcpyDeviceToHost));
    auto cell_of = [&](const float p[3]) { // (GetBoxAddress, as rt_wf_shared.h's cell_of)
        uint32_t c[3] = { 0, 0, 0 };
        for (int w = 0; w < 3; ++w)
            for (int div = RT_GRID_DIV / 2; div >= 1; div /= 2)
                if (planes[(size_t)w * (RT_GRID_DIV + 1) + c[w] + div] < p[w]) c[w] += div;
        return c[0] | c[1] << 8 | c[2] << 16;
    };
    // the cells an entry's walk makes if it hits nothing (plan_ray: one axis by one cell per step)
    auto visits_of = [&](const uint4 *e) -> uint64_t {
        const uint32_t start = e[0].y & 0xffffffu;
        uint32_t last = e[0].z;
        if (last == 0xffffffffu) { // no end cell: the walk leaves the box, at the smallest of the three wall crossings
            float o[3], d[3], te = HUGE_VALF;
            memcpy(o, &e[2], 12); memcpy(d, &e[3], 12);
            for (int w = 0; w < 3; ++w)
                if (d[w] != 0.f) { const float t = (planes[(size_t)w * (RT_GRID_DIV + 1) + (0.f <= d[w] ? RT_GRID_DIV : 0)] - o[w]) / d[w]; if (t < te) te = t; }
            if (!(te < HUGE_VALF)) return 1;
            const float to[3] = { o[0] + te * d[0], o[1] + te * d[1], o[2] + te * d[2] };
            last = cell_of(to);
        }
        uint64_t v = 1;
        for (int w = 0; w < 3; ++w) v += (uint64_t)std::abs((int)((last >> 8 * w) & 255u) - (int)((start >> 8 * w) & 255u));
        return v;
    };
    uint64_t *out = sc->visitLog[r].data();
    out[RT_ROUND_VISIT_ORDERED] = mode.ordered;
    auto kind_of = [&](uint32_t q) { return q >= cap ? 2u : (pathOf[q].y != 0xffffffffu ? 0u : 1u); }; // q: a ray's queue index
    for (uint32_t look = 0; look < 2; ++look)
        for (uint32_t s = 0; s < mode.slices; ++s) {
            const uint32_t n = std::min(ctl[RT_WF_CTL_COUNTS + look * RT_WF_SHARDS + s], sliceCap), base = look * cap + s * sliceCap;
            for (uint32_t q = base; q < base + n; ++q) {
                uint64_t *f = out + RT_ROUND_VISIT_RAYS + 3 * kind_of(q);
                f[0] += 1;
                f[1] += key[q] != ~0ull;
                if (!mode.ordered) continue;
                f[2] += visits_of(&ent[(size_t)4 * q]);
                out[RT_ROUND_VISIT_ENTRIES] += 1;
                out[RT_ROUND_VISIT_ENDED] += ent[(size_t)4 * q].z != 0xffffffffu;
            }
        }
    for (uint32_t i = 0; i < extra; ++i) { // region B: the further segments of cut rays, x = the ray's queue index (all ones: an unused reservation)
        const uint4 *e = &ent[(size_t)4 * (2 * (size_t)cap + i)];
        if (e[0].x >= 2 * cap) continue;
        out[RT_ROUND_VISIT_RAYS + 3 * kind_of(e[0].x) + 2] += visits_of(e);
        out[RT_ROUND_VISIT_ENTRIES] += 1;
        out[RT_ROUND_VISIT_ENDED] += e[0].z != 0xffffffffu;
    }
    return 0;
}

// the layout of round r: from the plan, or (watched batch) from what the round is assumed to hold
RtRoundMode round_mode(const rtHipScene *sc, const FrameState &S, Group &G, uint32_t r)
{
    if (G.modes.size() <= r) {
        const uint32_t before = G.modes.empty() ? (uint32_t)RT_WF_SHARDS : G.modes.back().slices;
        uint64_t rays = G.guessRays;
        if (S.planned) rays = r < RT_WF_ROUND_LOG ? G.plan[r].rays : 0;
        else G.guessRays = std::max<uint64_t>(G.guessRays / 4, 1); // (watched: a round is assumed to hold a quarter of the one before)
        RtRoundMode m = mode_for(sc->tune, r, rays, before);
        // (decided once, here: logic(r - 1) places the entries and trace(r) reads them by the same flag)
        const uint32_t batches = (sc->dev.sampleCount + sc->samplesPerBatch - 1u) / sc->samplesPerBatch;
        if (round_goes_direct(S.planned, r, m, G.dev.pathClass, sc->tune.placeDirect, sc->tune.visitLog, batches, r <= RT_WF_PLACE_ROUNDS ? G.place[r] : PlaceStamp(),
                              G.dev.seedStride, G.dev.sampleFirst))
            m.ordered |= RT_ROUND_DIRECT;
        G.modes.resize(r + 1, m);
    }
    return G.modes[r];
}

bool runs_split(const rtHipScene *sc, const Group &G, uint32_t r) { return round_runs_split(r, sc->tune.logicSplit, G.wf.lookAhead, G.dev.pathClass); }

// Round G.rounds of the batch, on `on`: (scatter,) trace of the entries the logic round before appended, then the logic round.
int issue_round(rtHipScene *sc, FrameState &S, Group &G, hipStream_t on)
{
    const Tuning &T = sc->tune;
    const uint32_t r = G.rounds;
    const RoundPlan plan = r < RT_WF_ROUND_LOG ? G.plan[r] : RoundPlan();
    const RtRoundMode mode = r > 0 ? round_mode(sc, S, G, r) : RtRoundMode{ 0u, 4096u, 64u, (uint32_t)RT_WF_SHARDS };
    if (r > 0) { // the entries appended by logic(r-1): order them if the round is an ordered one, then walk the grid
        if (mode.ordered & RT_ROUND_DIRECT) ++S.directRounds; // (logic(r - 1) wrote the entries in sorted place: nothing to scatter)
        else if (mode.ordered) {
            HIP_OK(stage(sc, 4, on, [&] { return rtw_launch_scatter(&G.wf, r, G.queueBlocks, &mode, on); }));
            ++S.scatterLaunches;
            // the launch records the round's placement table under this layout; a frame of several batches leaves its last batch's, which no frame may use
            if (r <= RT_WF_PLACE_ROUNDS) G.place[r] = PlaceStamp{ mode.slices, mode.segLen, G.dev.seedStride, G.dev.sampleFirst, sc->dev.sampleCount <= sc->samplesPerBatch };
        }
        const uint32_t traceBlocks = trace_blocks(S.planned, r, mode, plan, G.traceBlocks, G.wf.capacity, G.wf.extraCap, T.planGridTiny != 0);
        HIP_OK(stage(sc, 2, on, [&] { return rtw_launch_trace(&G.dev, &G.wf, r, traceBlocks, &mode, on); }));
        if (T.visitLog && r < RT_WF_ROUND_LOG && log_round_visits(sc, G, r, mode, on) != 0) return -1;
    }
    const RtRoundMode next = round_mode(sc, S, G, r + 1);
    if ((next.ordered & RT_ROUND_DIRECT) && T.placeSkew && !sc->placeSkewed) { // TEST ONLY: the table the entries are about to be placed by, skewed once
        HIP_OK(rtw_launch_place_skew(&G.wf, r + 1, on));
        sc->placeSkewed = true;
    }
    // A split round (round_runs_split).  A planned frame sizes the shade launch from the list the plan
    // logged and skips it where that was empty; the answer kernel is told, and raises RT_WF_ERR_GRID if it lists a path all the same.
    if (runs_split(sc, G, r)) {
        const uint32_t shadeBlocks = shade_blocks(S.planned, r, mode, plan, G.logicBlocks, T.planShadeSkip != 0);
        ++S.splitRounds;
        HIP_OK(stage(sc, 1, on, [&] { return rtw_launch_answer(&G.dev, &G.wf, r, G.logicBlocks, mode.slices, &G.shade, shadeBlocks ? 1u : 0u, on); }));
        if (shadeBlocks) HIP_OK(stage(sc, 1, on, [&] { return rtw_launch_shade(&G.dev, &G.wf, r, shadeBlocks, mode.slices, &next, &G.shade, on); }));
    } else
        HIP_OK(stage(sc, 1, on, [&] { return rtw_launch_logic(&G.dev, &G.wf, r, G.logicBlocks, mode.slices, &next, on); }));
    ++G.rounds;
    return 0;
}

// Watched: rounds are issued in chunks without looking at the queue.  A one-bounce scene needs exactly three logic rounds
// (shade the primary hits | consume shadow + bounce answers, shade the bounce hits | consume their shadow answers) with a
// trace before the last two, so a chunk is 3 rounds.
int issue_chunk(rtHipScene *sc, FrameState &S, Group &G, hipStream_t on)
{
    for (uint32_t k = 0; k < 3 && G.rounds < RT_WF_MAX_ROUNDS; ++k)
        if (issue_round(sc, S, G, on) != 0) return -1;
    HIP_OK(hipMemcpyAsync(G.hostCount, G.wf.ctl + (G.rounds % 3) * RT_WF_CTL_WORDS + RT_WF_CTL_COUNTS, sizeof(uint32_t) * RT_WF_SHARDS, hipMemcpyDeviceToHost, on)); // main slices
    return 0;
}

// The batch of samples base+1 .. of group G starts on `on`: its state is reset and its primary stage issued.
int start_batch(rtHipScene *sc, const FrameState &S, Group &G, hipStream_t on, uint32_t base)
{
    const uint32_t sampleCount = sc->dev.sampleCount;
    G.wf.sampleBase = base;
    G.wf.samplesInBatch = std::min<uint32_t>(sc->samplesPerBatch, sampleCount - base);
    G.rounds = 0;
    G.modes.clear();
    G.guessRays = (uint64_t)(G.slot1 - G.slot0) * RT_TILE_PIXELS * G.wf.samplesInBatch; // round 1 of a watched batch: as if every pixel were a path
    if (!G.ctlClean) {
        HIP_OK(hipMemsetAsync(G.wf.ctl, 0, sizeof(uint32_t) * (size_t)3 * RT_WF_CTL_WORDS, on));
        HIP_OK(hipMemsetAsync(G.shade.count, 0, sizeof(uint32_t) * (size_t)3 * RT_WF_SHARDS, on));
    }
    G.ctlClean = false;
    if (!S.planned) memset(G.hostLog, 0, sizeof(uint4) * RT_WF_ROUND_LOG); // (nothing of this group is in flight: the batch before was waited for)
    // NORMAL / ALBEDO on: the batch's samples are summed per pixel in the primary stage's bracket (the batch with sampleBase 0 starts
    // the sums from zero, so planned and redone frames need no memset)
    auto launch_surface = [&] { return rtw_launch_surface_passes(&G.dev, &G.wf, sc->surfBuf + (size_t)G.slot0 * RT_SURF_WORDS * RT_TILE_PIXELS, on); };
    if (sc->passBuf) {
        // passes on: with several samples per pixel the group's hit counters (one 64 KiB plane per slot) start at zero in every
        // frame -- in-stream, so planned and redone frames alike; a one-sample frame's kernel stores them, and sample 1 rewrites
        // every depth and triangle word
        uint32_t *pass = sc->passBuf + (size_t)G.slot0 * RT_PASS_WORDS * RT_TILE_PIXELS;
        HIP_OK(stage(sc, 0, on, [&] {
            if (base == 0 && sampleCount > 1) {
                const hipError_t er = hipMemset2DAsync(pass + RT_PASS_HITS * RT_TILE_PIXELS, (size_t)RT_PASS_WORDS * RT_TILE_PIXELS * 4, 0,
                                                       (size_t)RT_TILE_PIXELS * 4, G.slot1 - G.slot0, on);
                if (er != hipSuccess) return er;
            }
            const hipError_t er = rtw_launch_primary_passes(&G.dev, &G.wf, pass, on);
            return (er != hipSuccess || !sc->surfBuf) ? er : launch_surface();
        }));
    } else HIP_OK(stage(sc, 0, on, [&] {
        const hipError_t er = rtw_launch_primary(&G.dev, &G.wf, on);
        return (er != hipSuccess || !sc->surfBuf) ? er : launch_surface();
    }));
    return 0;
}

// A planned batch: the plan's rounds back to back, then the kernel that tells the host what was left waiting.
int issue_planned_batch(rtHipScene *sc, FrameState &S, Group &G, hipStream_t on)
{
    while (G.rounds < S.planRounds)
        if (issue_round(sc, S, G, on) != 0) return -1;
    // (the shade lists' lengths are zeroed with the control words where the batch can have run split rounds; G.rounds >= 1 here)
    HIP_OK(rtw_launch_status(&G.wf, G.rounds, runs_split(sc, G, G.rounds) ? G.shade.count : nullptr, on));
    G.ctlClean = true;
    return 0;
}

// A watched batch, its first chunk issued: chunk after chunk until no path is waiting, then its round log is folded into the group's next plan.
int watch_batch(rtHipScene *sc, FrameState &S, Group &G, hipStream_t on)
{
    for (;;) {
        HIP_OK(hipStreamSynchronize(on));
        if (const uint32_t err = G.hostStatus[RT_WF_STATUS_ERROR]) {
            G.hostStatus[RT_WF_STATUS_ERROR] = 0u;
            return device_error(err);
        }
        uint64_t waiting = 0;
        for (int i = 0; i < RT_WF_SHARDS; ++i) waiting += G.hostCount[i];
        if (waiting == 0) break;
        if (G.rounds >= RT_WF_MAX_ROUNDS) return fail("wavefront pipeline: more than %d rounds", RT_WF_MAX_ROUNDS);
        G.guessRays = 2 * waiting; // the next round holds at most two rays per waiting path
        if (issue_chunk(sc, S, G, on) != 0) return -1;
    }
    // (hostLog: mapped host memory; the stream was synchronised in the loop above)
    fold_round_log(G.hostLog, G.modes.data(), G.modes.size(), G.rounds, G.planNext, &G.roundsNeeded);
    return 0;
}

// Every group adopts what its watched batches needed; returns the rounds a planned batch issues (the maximum over the groups).
uint32_t adopt_plans(rtHipScene *sc, bool furtherBatches, bool spare, uint32_t cap)
{
    uint32_t need = 1;
    for (auto &G : sc->groups) need = std::max(need, adopt_plan(G.plan, G.planNext, &G.roundsNeeded, furtherBatches));
    return plan_rounds(need, spare, cap);
}

} // namespace

// One frame through the staged pipeline: per sample batch and tile group -- primary, then rounds of (scatter,) trace, logic until
// no path is waiting for the grid, then the ordered accumulate.  The round count is data dependent.
//
// WATCHED batch (the first batch of a scene's first frame, or Tuning::blocking): rounds are issued in chunks and the queue length
// is read back after every chunk (one small pinned copy + stream sync per chunk and group).  It leaves a PLAN behind: the number of
// rounds the batch needed and, per round, its rays, its longest queue slice and its further segments (RtWavefront::roundLog).
// PLANNED batches (every later frame, and the further batches of a watched frame): the plan's rounds are issued back to back with
// the layouts and grid sizes the plan implies and NO host synchronisation -- whatever the caller enqueues behind the frame (the tile
// gather) follows immediately.  The last kernel of a batch (wf_status_kernel) adds the number of paths still waiting to a mapped
// host word; frame_finish() looks at it after the caller's own synchronisation.  A non-zero count means the plan was too short for
// this frame (the frames of a scene are deterministic, so that only happens when something about the frame changed, or when a later
// sample batch needs more than the first one did): the frame is rendered again, every batch watched, and the caller is told, so
// that work enqueued behind the incomplete frame can be redone.
// How a round's entries are laid out (ordered or not, cut how finely, how many queue slices) is decided HERE, before the round exists,
// from the plan -- or, in a watched batch, from a guess: the layout changes when cells are visited, never what is found.
// Groups run concurrently on their own streams, forked from and joined to `st`; with stage timing on they run one after the
// other on `st`, so that a kernel's measured duration is its own.
int rthost::render_wavefront(rtHipScene *sc, hipStream_t st, bool forceDiscovery)
{
    const Tuning &T = sc->tune;
    if (T.visitLog) sc->visitLog.assign(RT_WF_ROUND_LOG, {});
    const bool serial = sc->stageTiming || sc->groups.size() == 1;
    auto streamOf = [&](size_t g) { return (serial || g == 0) ? st : sc->groups[g].stream; };
    if (!serial) {
        HIP_OK(hipEventRecord(sc->forkEvent, st));
        for (size_t g = 1; g < sc->groups.size(); ++g) HIP_OK(hipStreamWaitEvent(sc->groups[g].stream, sc->forkEvent, 0));
    }
    const bool watchedFrame = forceDiscovery || sc->blocking || sc->planRounds == 0;
    FrameState S{ !watchedFrame, sc->planRounds };
    // A watched frame is what everything that changes a frame's rays forces (planRounds = 0: camera, geometry, scene edit, sample window, pass
    // switches) and what redoes a flagged frame: the placement tables recorded before it are not this scene state's.  Its own scatter
    // launches record fresh ones.
    if (watchedFrame)
        for (auto &G : sc->groups)
            for (PlaceStamp &p : G.place) p = PlaceStamp();
    uint64_t rounds = 0;
    const uint32_t sampleCount = sc->dev.sampleCount;
    for (uint32_t base = 0; base < sampleCount; base += sc->samplesPerBatch) {
        for (size_t g = 0; g < sc->groups.size(); ++g) {
            Group &G = sc->groups[g];
            if (start_batch(sc, S, G, streamOf(g), base) != 0) return -1;
            if ((S.planned ? issue_planned_batch(sc, S, G, streamOf(g)) : issue_chunk(sc, S, G, streamOf(g))) != 0) return -1;
        }
        for (size_t g = 0; g < sc->groups.size(); ++g) {
            Group &G = sc->groups[g];
            const hipStream_t on = streamOf(g);
            if (S.planned) S.anyPlannedBatch = true;
            else if (watch_batch(sc, S, G, on) != 0) return -1;
            rounds = std::max<uint64_t>(rounds, G.rounds);
            if (!G.dev.directStore) // a one-sample frame that starts from zero: its pixels were written by the kernels that finished them
                HIP_OK(stage(sc, 3, on, [&] { return rtw_launch_accum(&G.dev, &G.wf, (base == 0 && !G.dev.continuesFrame) ? 1 : 0, on); }));
        }
        // a watched batch knows here that its rounds are over: tell whoever polls GetProgress (raytrace.c:566-587)
        if (!S.planned && sc->progress)
            sc->progress->store(sc->progressBase + sc->progressSpan * (float)std::min<uint64_t>(sampleCount, (uint64_t)base + sc->samplesPerBatch) / (float)sampleCount,
                                std::memory_order_relaxed);
        // A watched frame's further batches: the same pixels with other sample ids -- statistically the same rounds.  They are issued from
        // the plan the batches so far left (a fifth more than the largest of them saw, see trace_blocks) and verified like any planned
        // frame; should one of them need more, frame_finish renders the whole frame again, every batch watched.
        if (!S.planned && !forceDiscovery && !sc->blocking && T.batchPlan && base + sc->samplesPerBatch < sampleCount) {
            S.planRounds = adopt_plans(sc, true, true, 0); // (one spare round: a later batch's deepest path may go one bounce further)
            S.planned = true;
        }
    }
    if (watchedFrame) // adopt what this frame's watched batches needed (the maximum over batches and groups)
        // (the spare round of the further batches is kept for the frames to come)
        sc->planRounds = adopt_plans(sc, false, S.anyPlannedBatch && sampleCount > sc->samplesPerBatch, T.planRounds);
    if (S.anyPlannedBatch) sc->unverified = true;
    if (!serial)
        for (size_t g = 1; g < sc->groups.size(); ++g) {
            HIP_OK(hipEventRecord(sc->groups[g].done, sc->groups[g].stream));
            HIP_OK(hipStreamWaitEvent(st, sc->groups[g].done, 0));
        }
    sc->roundsLast = rounds;
    sc->splitRoundsLast = S.splitRounds;
    sc->directRoundsLast = S.directRounds;
    sc->scatterLaunchesLast = S.scatterLaunches;
    return 0;
}

// After the caller's synchronisation of `st`: were the planned frames since the last call complete?  If not, the LAST frame
// is rendered again with the queue watched (earlier incomplete frames were overwritten by it anyway).  *redone (optional)
// = 1 when that happened: whatever was enqueued behind the incomplete frame saw unfinished tiles.
int rthost::frame_finish(rtHipScene *sc, hipStream_t st, int *redone)
{
    if (redone) *redone = 0;
    if (!sc->unverified) return 0;
    HIP_OK(hipStreamSynchronize(st));
    for (auto &G : sc->groups)
        if (G.stream) HIP_OK(hipStreamSynchronize(G.stream));
    sc->unverified = false;
    uint64_t waiting = 0;
    for (auto &G : sc->groups) {
        if (const uint32_t err = G.hostStatus[RT_WF_STATUS_ERROR]) {
            G.hostStatus[RT_WF_STATUS_ERROR] = 0u;
            if (err & ~RT_WF_ERR_GRID) return device_error(err);
            waiting += 1; // a planned trace grid was too small: same remedy as a plan with too few rounds
        }
        waiting += G.hostStatus[RT_WF_STATUS_WAITING];
        G.hostStatus[RT_WF_STATUS_WAITING] = 0u;
    }
    if (waiting == 0) {
        return 0;
    }
    if (redone) *redone = 1;
    apply_window(sc, sc->lastWindow); // the window that frame had; the scene's next window has moved on already and stays where it is
    if (render_wavefront(sc, st, true) != 0) return -1;
    HIP_OK(hipStreamSynchronize(st));
    return 0;
}
