"""Sample windows on the MI355X (run with -m gpu): the default window leaves every frame alone; progressive rendering equals the oracle's
N-sample frame bit for bit on both pipelines, under pipeline modes, sample batches and tile deals; windows off the S grid; accumulating
frames are watched, never redone; the divisor; advance under planned and redone frames; the render passes of a window; the temporal
chain fed with a sequence; refusals on a scene; and single window frames against the window oracle (oracle_lib.oracle_render_window):
every frame of a progressive run and of a sequence, freely chosen windows (64-bit seeds among them), a progressive run that goes on
over camera, geometry and pipeline changes, and sequences under split logic rounds and the ray clip."""
import ctypes as C

import numpy as np
import pytest

import camera_cases as CC
import geometry_cases as GC
import motion_oracle as MO
import oracle_lib as O
import sample_window_cases as WC
import temporal_oracle as TO
from conftest import golden_names
from geometry_checks import update_to
from opencl_render_amd import raytrace as R, scene as SCN

pytestmark = pytest.mark.gpu

F32 = np.float32
U32_MAX = 2 ** 32 - 1
ZERO = dict(total=0, first=0, divisor=0, accumulate=0, advance=0)


def window(total, first, divisor, accumulate=0, advance=0):
    return dict(total=total, first=first, divisor=divisor, accumulate=accumulate, advance=advance)


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the sample window tests cannot run (and the product has no CPU fallback)")


def assert_planes(got, want, what):
    for ch, g, w in zip("RGB", got, want):
        g = np.asarray(g).reshape(np.asarray(w).shape)
        bad = int((g != w).sum())
        assert bad == 0, f"{what}: plane {ch} differs in {bad}/{g.size} values, max |d|={int(np.abs(g.astype(int) - w.astype(int)).max())}"


def frame(rs):
    """Renders one frame and reads it back into fresh planes."""
    rs.render()
    return rs.readback()


def framed(sc, env=None, monkeypatch=None, **win):
    """The frame a fresh scene renders under the window `win`."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_sample_window(**win)
        return frame(rs)
    finally:
        rs.close()


# ---- 3. the default window ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names())
def test_the_default_window_leaves_the_frame_alone(name):
    sc, want = WC.golden(name)
    S = sc.sample_count
    rs = R.ResidentScene(sc, 0)
    try:
        assert rs.sample_window() == {"next": window(S, 0, S), "last": ZERO}
        assert R.lib().rtHipSceneSetSampleWindow(rs.handle, None) == 0
        assert rs.sample_window() == {"next": window(S, 0, S), "last": ZERO}
        assert_planes(frame(rs), want, f"{name}: NULL window")
        assert rs.sample_window() == {"next": window(S, 0, S), "last": window(S, 0, S)}
        rs.set_sample_window(S, 0, S, accumulate=False, advance=False)
        assert_planes(frame(rs), want, f"{name}: the default window spelled out")  # (a planned frame)
        rs.set_sample_window(2 * S, S, 3)
        rs.set_sample_window()
        assert rs.sample_window()["next"] == window(S, 0, S)
        rs.set_pipeline(R.PIPELINE_MEGAKERNEL)
        assert_planes(frame(rs), want, f"{name}: back to the default, megakernel")
    finally:
        rs.close()


# ---- 4. progressive equals the reference -----------------------------------------------------------------------------------------------
def progressive(sc, total, pipeline=R.PIPELINE_WAVEFRONT, tiles=None, planes=None, finish=False):
    """The last planes of ResidentScene.progressive(total) on a fresh scene, and whether any finish() reported a redo."""
    rs = R.ResidentScene(sc, 0, tiles)
    redone = False
    try:
        rs.set_pipeline(pipeline)
        S = sc.sample_count
        if planes is not None or finish:  # (a tile deal adds into shared planes once, at the end)
            rs.set_sample_window(total, 0, total, accumulate=True, advance=True)
            for i in range(total // S):
                rs.render()
                if finish:
                    redone |= rs.finish()  # (waits for the frame itself; rtHipSync would verify it without telling)
            last = rs.sample_window()["last"]
            assert last == window(total, total - S, total, 1, 1)
            return rs.readback(planes), redone
        done, got = 0, None
        for done, got in rs.progressive(total):
            pass
        assert done == total
        assert rs.sample_window() == {"next": window(total, 0, total, 1, 1), "last": window(total, total - S, total, 1, 1)}
        return got, redone
    finally:
        rs.close()


@pytest.mark.parametrize("pipeline", [R.PIPELINE_WAVEFRONT, R.PIPELINE_MEGAKERNEL], ids=["wavefront", "megakernel"])
@pytest.mark.parametrize("name, samples, total", WC.PROGRESSIVE)
def test_progressive_equals_the_oracle(name, samples, total, pipeline):
    sc, _ = WC.golden(name)
    got, _ = progressive(sc, total, pipeline)
    assert_planes(got, WC.oracle_frame(name, total), f"{name}: {total // samples} frames of {samples}")


def test_the_saturating_case_saturates():
    """What makes degenerate_and_outside the case for the order of the adds: its 12-sample frame has saturated values, and summing the
    windows without saturation, or saturating once at the end, would give other planes."""
    want = WC.oracle_frame("degenerate_and_outside", 12)
    assert WC.shares(want)[1] > 0.01


SMALL_STATE = {"RT_WF_STATE_MB": "20"}  # ~1 sample per batch for one 128x128 tile: a window of the S >= 2 scenes needs several batches
MODES = [{"RT_WF_GROUPS": "3"}, {"RT_WF_BLOCKING": "1"}, {"RT_WF_LOOKAHEAD": "0"}, SMALL_STATE]


def scene_bytes(sc):
    rs = R.ResidentScene(sc, 0)
    try:
        return rs.bytes()
    finally:
        rs.close()


@pytest.mark.parametrize("env", MODES, ids=lambda e: ",".join(f"{k[3:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("name, samples, total", WC.PROGRESSIVE)
def test_progressive_equals_the_oracle_under_pipeline_modes(name, samples, total, env, monkeypatch):
    sc, _ = WC.golden(name)
    roomy = scene_bytes(sc) if env is SMALL_STATE and samples >= 2 else None
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if roomy is not None:
        # the path state is sized for the samples of one batch (min(what the budget holds, S) per pixel): a smaller scene means a batch
        # holds fewer than S samples, so every window is rendered in several batches.  (The S = 1 scenes run this mode in one batch.)
        assert scene_bytes(sc) < roomy, f"{name}: RT_WF_STATE_MB=20 no longer forces several batches"
    got, _ = progressive(sc, total)
    assert_planes(got, WC.oracle_frame(name, total), f"{name} under {env}")


def test_a_deal_over_two_instances_composes_the_progressive_frame():
    name, total = "odd_size_multi_tile", 4
    sc, _ = WC.golden(name)
    planes = [np.zeros(sc.pixels, np.uint16) for _ in range(3)]
    for rank in range(2):
        tiles = R.tiles_of_rank(sc.width, sc.height, rank, 2)
        assert len(tiles) > 0
        progressive(sc, total, tiles=tiles, planes=planes)
    assert_planes(planes, WC.oracle_frame(name, total), "two instances with disjoint tiles")


# ---- 5. windows that do not start on a multiple of S --------------------------------------------------------------------------------
def test_windows_off_the_sample_grid_sum_to_the_oracle():
    name, total = "lambert_distant", 4
    sc, _ = WC.golden(name)
    a = framed(WC.with_samples(sc, 1), total=total, first=0, divisor=total)
    b = framed(WC.with_samples(sc, 3), total=total, first=1, divisor=total)
    summed = [x.astype(np.uint32) + y.astype(np.uint32) for x, y in zip(a, b)]
    assert max(int(s.max()) for s in summed) < WC.SATURATED  # (no add saturated: a plain sum is the ordered sum)
    assert_planes(summed, WC.oracle_frame(name, total), "S = 1 at f = 0 plus S = 3 at f = 1")


# ---- 6. accumulating frames are never redone ------------------------------------------------------------------------------------------
def test_accumulating_frames_are_watched_not_redone(monkeypatch):
    monkeypatch.setenv("RT_WF_PLAN_ROUNDS", "1")  # planned frames issue one round: too few for mirror_hall
    sc, _ = WC.golden("mirror_hall")
    got, redone = progressive(sc, 4, finish=True)
    assert not redone
    assert_planes(got, WC.oracle_frame("mirror_hall", 4), "mirror_hall with plans of one round")


# ---- 7. the divisor ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WC.DIVISOR_SCENES))
def test_the_divisor_scales_each_sample_before_it_is_truncated(name):
    """A = trunc(out * 65535), B = trunc(out * (65535 / 4)): the quotient and the product scale exactly by a power of two and the colours
    of these scenes are non-negative, so B == A >> 2 wherever A did not saturate, and B >= 65535 >> 2 where it did."""
    sc, want = WC.golden(name)
    assert sc.sample_count == 1
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_sample_window(1, 0, 1)
        assert_planes(frame(rs), want, f"{name}: N = 1, f = 0")
        frames = []
        for f in range(4):
            rs.set_sample_window(4, f, 1)
            a = [p.copy() for p in frame(rs)]
            rs.set_sample_window(4, f, 4)
            b = frame(rs)
            assert rs.sample_window()["last"] == window(4, f, 4)
            nonzero, saturated = WC.shares(a)
            assert nonzero >= 0.05 and saturated <= 0.01, (name, f, nonzero, saturated)
            for ch, x, y in zip("RGB", a, b):
                below = x < WC.SATURATED
                assert np.array_equal(y[below], x[below] >> 2), f"{name} f={f}: plane {ch}"
                assert (y[~below] >= WC.SATURATED >> 2).all(), f"{name} f={f}: plane {ch}, saturated values"
            frames.append(a)
        for i in range(4):
            for j in range(i):
                assert WC.differing(frames[i], frames[j]) > 0, f"{name}: the frames of f = {j} and f = {i} are the same"
    finally:
        rs.close()


# ---- 8. advance under planned frames ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sequence_frames():
    """lambert_distant (S = 2), N = 8: the frame of each window f = 0, 2, 4, 6 from a fresh scene whose every frame is watched."""
    sc, _ = WC.golden("lambert_distant")
    mp = pytest.MonkeyPatch()
    try:
        return {f: framed(sc, {"RT_WF_BLOCKING": "1"}, mp, total=8, first=f, divisor=sc.sample_count) for f in range(0, 8, 2)}
    finally:
        mp.undo()


def test_advance_moves_the_window_under_planned_frames(sequence_frames):
    sc, _ = WC.golden("lambert_distant")
    S = sc.sample_count
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_sample_window(8, 0, S, advance=True)
        first = None
        for i in range(9):  # back to back: frames after the first are planned
            f = (i * S) % 8
            assert rs.sample_window()["next"] == window(8, f, S, 0, 1)
            got = frame(rs)
            assert rs.sample_window()["last"] == window(8, f, S, 0, 1)
            assert_planes(got, sequence_frames[f], f"frame {i}: window f = {f}")
            first = got if i == 0 else first
        assert_planes(got, first, "the ninth frame is the first again")
        assert len({tuple(p.tobytes() for p in v) for v in sequence_frames.values()}) == 4  # (four different frames)
    finally:
        rs.close()


def test_a_redone_frame_renders_its_own_window_and_does_not_advance_again(sequence_frames, monkeypatch):
    monkeypatch.setenv("RT_WF_PLAN_ROUNDS", "1")
    sc, _ = WC.golden("lambert_distant")
    S = sc.sample_count
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_sample_window(8, 0, S, advance=True)
        assert_planes(frame(rs), sequence_frames[0], "the watched frame that leaves the (shortened) plan")
        rs.render()
        moved = {"next": window(8, 4, S, 0, 1), "last": window(8, 2, S, 0, 1)}
        assert rs.sample_window() == moved
        assert rs.finish() is True  # the plan of one round was too short: the frame was rendered again
        assert rs.sample_window() == moved  # ... with the window it had; the next window has moved once
        assert_planes(rs.readback(), sequence_frames[2], "the redone frame is the watched frame of `last`")
    finally:
        rs.close()


# ---- 9. the render passes describe the window's own samples ------------------------------------------------------------------------------
def test_passes_describe_the_windows_samples():
    sc, _ = WC.golden("mixed_materials_textured")
    assert sc.sample_count == 2
    want = WC.window_passes(sc, 6, 2)
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_passes(alpha=True, depth=True, triangle=True, normal=True, albedo=True)
        rs.set_sample_window(6, 2, 2)
        planes = frame(rs)
        got = rs.readback_passes()
    finally:
        rs.close()
    for k in ("alpha", "triangle"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("depth", "normal", "albedo"):
        bad = int((~TO.same_bits(got[k], want[k])).sum())
        assert bad == 0, f"pass {k} differs bitwise in {bad} values"
    default = WC.window_passes(sc, 2, 0)
    assert (default["depth"].view(np.uint32) != want["depth"].view(np.uint32)).any()  # (other samples than the default window's)
    assert_planes(planes, framed(sc, total=6, first=2, divisor=2), "the frame with the passes on")


# ---- 10. the temporal chain gets something to average ------------------------------------------------------------------------------------
def colour_of(planes, sc):
    return np.stack([p.reshape(sc.height, sc.width) for p in planes], -1).astype(F32) / F32(65535.0)


def temporal_loop(sc, flow, frames, sequence):
    """`frames` times render, temporal(max_history=32) under a still camera, checked against the oracle fed with the read-backs.  Returns
    the first frame's colour, the last output and the variance plane of the same loop through temporal_variance."""
    rs = R.ResidentScene(sc, 0)
    try:
        if sequence:
            rs.set_sample_window(8, 0, 1, advance=True)
        hist = TO.empty_history(sc.height, sc.width)
        first = out = None
        for i in range(frames):
            rs.render()
            got = rs.temporal(max_history=32.0)
            colour = colour_of(rs.readback(), sc)
            want = TO.accumulate(colour, flow["motion"], flow["prev_t"], flow["triangle"], hist, max_history=32.0)
            for k in ("colour", "count"):
                bad = int((~TO.same_bits(got[k], want[k])).sum())
                assert bad == 0, f"frame {i}: {k} differs from the oracle in {bad} values"
            hist = TO.next_history(want, flow["t"], flow["triangle"])
            first = colour if i == 0 else first
            out = got
        rs.reset_temporal()
        if sequence:
            rs.set_sample_window(8, 0, 1, advance=True)
        for i in range(frames):
            rs.render()
            var = rs.temporal_variance(max_history=32.0)
        assert np.array_equal(var["colour"].view(np.uint32), out["colour"].view(np.uint32))  # (the same sequence, the same accumulation)
        return first, out, var["variance"]
    finally:
        rs.close()


def test_a_sequence_gives_the_temporal_chain_something_to_average():
    sc = WC.with_samples(WC.golden("lambert_distant")[0], 1)
    flow = MO.motion(sc, sc)  # a still camera
    first, out, variance = temporal_loop(sc, flow, 8, sequence=True)
    assert (out["count"] == 8.0).any()
    assert (out["colour"].view(np.uint32) != first.view(np.uint32)).any()
    assert (variance > 0).any()
    # the documented limit of the default window: every frame is the same frame and the temporal variance is 0 everywhere
    first, out, variance = temporal_loop(sc, flow, 8, sequence=False)
    assert (variance == 0).all()


# ---- 11. refusals on a scene ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_window_and_the_next_frame_unchanged():
    sc, want = WC.golden("lambert_distant")
    S = sc.sample_count
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_sample_window(8, 2, S)
        kept = [p.copy() for p in frame(rs)]
        before = rs.sample_window()
        for bad, text in (((0, 0, S, 0, 0), "total"), ((8, 0, 0, 0, 0), "divisor"), ((8, 7, 8, 0, 0), "reaches past"),
                          ((8, 0, 8, 2, 0), "accumulate"), ((8, 0, 8, 0, 3), "advance"), ((9, 0, 9, 0, 1), "multiple"), ((8, 1, 8, 0, 1), "multiple")):
            w = R.SampleWindow(*bad)
            assert R.lib().rtHipSceneSetSampleWindow(rs.handle, C.byref(w)) == -1
            assert text in R.last_error(), (bad, R.last_error())
            assert rs.sample_window() == before
        with pytest.raises(RuntimeError, match="reaches past"):
            rs.set_sample_window(8, 7)
        assert_planes(frame(rs), kept, "the frame after the refusals")
        # the work counters describe the default frame
        with pytest.raises(RuntimeError, match="sample window"):
            rs.render_counted()
        assert rs.sample_window()["next"] == before["next"]
        # a peer starts with the default window, whatever its model has
        peer = R.ResidentScene(sc, 0, like=rs)
        try:
            assert peer.sample_window() == {"next": window(S, 0, S), "last": ZERO}
            assert_planes(frame(peer), want, "a peer renders the default frame")
        finally:
            peer.close()
        rs.set_sample_window()
        rs.render_counted()
        assert_planes(rs.readback(), want, "the counted frame under the default window")
    finally:
        rs.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def test_command_line_progressive_and_sequence(tmp_path):
    from opencl_render_amd import __main__ as M, frontend as F, scene as S
    soup = ["--scene", "soup", "--width", "96", "--height", "64", "--triangles", "20000"]
    # --progressive 6 in frames of 2: the finished image is the --samples 6 image, the two previews are numbered and scaled by N / done
    assert M.main(soup + ["--samples", "2", "--progressive", "6", "--out", str(tmp_path / "img.ppm")]) == 0
    assert M.main(soup + ["--samples", "6", "--out", str(tmp_path / "ref.ppm")]) == 0
    assert open(tmp_path / "img.ppm", "rb").read() == open(tmp_path / "ref.ppm", "rb").read()
    assert (tmp_path / "img_000.ppm").exists() and (tmp_path / "img_001.ppm").exists() and not (tmp_path / "img_002.ppm").exists()
    sc = S.make_soup(96, 64, 20000, 0.02, samples=2)
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    rs = R.ResidentScene(sc, 0)
    try:
        for i, (done, planes) in enumerate(rs.progressive(6)):
            if done < 6:
                preview = [np.minimum(p.astype(np.uint64) * 6 // done, 65535).astype(np.uint16).reshape(64, 96) for p in planes]
                F.write_ppm(str(tmp_path / "want.ppm"), *preview)
                assert open(tmp_path / f"img_{i:03d}.ppm", "rb").read() == open(tmp_path / "want.ppm", "rb").read(), f"preview {i}"
    finally:
        rs.close()
    # --sequence 4 over an orbit of 3: frame i renders the window f = 2 i mod 4
    orbit = soup + ["--samples", "2", "--orbit", "3"]
    assert M.main(orbit + ["--sequence", "4", "--out", str(tmp_path / "seq.ppm")]) == 0
    assert M.main(orbit + ["--out", str(tmp_path / "same.ppm")]) == 0
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_sample_window(4, 0, 2, advance=True)
        for i, position in enumerate(R.orbit_positions(np.zeros(3, F32), np.float32([0, 0, 3]), 3)):
            rs.look_at(position, np.float32([0, 0, 3]), (0, 1, 0), np.radians(M.parser().get_default("fov")))
            assert rs.sample_window()["next"]["first"] == 2 * i % 4
            F.write_ppm(str(tmp_path / "want.ppm"), *[p.reshape(64, 96) for p in frame(rs)])
            assert open(tmp_path / f"seq_{i:03d}.ppm", "rb").read() == open(tmp_path / "want.ppm", "rb").read(), f"sequence frame {i}"
            assert open(tmp_path / f"seq_{i:03d}.ppm", "rb").read() != open(tmp_path / f"same_{i:03d}.ppm", "rb").read()
    finally:
        rs.close()


# ---- single window frames against the window oracle ------------------------------------------------------------------------------------------
# A window frame has an expected value of its own (oracle_lib.oracle_render_window): no sum in which two windows' errors could cancel, no
# other device frame as the reference.  Modes: the wavefront pipeline with its first frame watched and the later ones planned, every
# frame watched, every frame planned (a frame of the default window goes first), and the megakernel.
ORACLE_MODES = ("wavefront", "watched", "planned", "megakernel")


def opened(sc, mode, monkeypatch, env=None):
    """A fresh scene under `mode` (and the RT_* variables in env); under "planned" a frame of the default window has been rendered, so the
    next frame that does not continue from the tile buffer is issued from the launch plan."""
    for k, v in dict(env or {}, **({"RT_WF_BLOCKING": "1"} if mode == "watched" else {})).items():
        monkeypatch.setenv(k, v)
    rs = R.ResidentScene(sc, 0)
    try:
        if mode == "megakernel":
            rs.set_pipeline(R.PIPELINE_MEGAKERNEL)
        if mode == "planned":
            rs.render()
            rs.sync()
            assert not rs.finish()
    except BaseException:
        rs.close()
        raise
    return rs


def checked_frame(rs, want, what):
    """Renders a frame that must not be redone, reads it back and compares it with `want`; returns the read-back."""
    rs.render()
    rs.sync()
    assert not rs.finish(), f"{what}: the frame was rendered again"
    got = [p.copy() for p in rs.readback()]
    assert_planes(got, want, what)
    return got


@pytest.mark.parametrize("mode", ["wavefront", "planned", "megakernel"])  # (a continuing frame is watched whatever the mode)
@pytest.mark.parametrize("name, samples, total", WC.PROGRESSIVE)
def test_every_frame_of_a_progressive_sequence_equals_the_chained_oracle(name, samples, total, mode, monkeypatch):
    sc, _ = WC.golden(name)
    chain = WC.window_chain(name, total)
    rs = opened(sc, mode, monkeypatch)
    try:
        rs.set_sample_window(total, 0, total, accumulate=True, advance=True)
        for i, want in enumerate(chain + chain[:1]):  # (the frame after the last starts from zero again: f == 0)
            f = i * samples % total
            assert rs.sample_window()["next"] == window(total, f, total, 1, 1)
            checked_frame(rs, want, f"{name}, {mode}: the tile buffer after frame {i} (f = {f})")
    finally:
        rs.close()


@pytest.mark.parametrize("mode", ORACLE_MODES)
@pytest.mark.parametrize("name, samples, total", WC.PROGRESSIVE)
def test_every_frame_of_a_sequence_equals_the_window_oracle(name, samples, total, mode, monkeypatch):
    sc, _ = WC.golden(name)
    rs = opened(sc, mode, monkeypatch)
    try:
        rs.set_sample_window(total, 0, samples, advance=True)
        for i in range(total // samples + 1):
            f = i * samples % total
            checked_frame(rs, WC.window_frame(name, total, f, samples), f"{name}, {mode}: frame {i}, window {{{total}, {f}, {samples}}}")
            assert rs.sample_window() == {"next": window(total, (f + samples) % total, samples, 0, 1), "last": window(total, f, samples, 0, 1)}
    finally:
        rs.close()


# {7, 3, 3} on an S = 2 scene: neither N nor f a multiple of S, D neither N nor S (1.5 times over-bright).  {2^32 - 1, 2^32 - 2, 1} on an
# S = 1 scene: pixel * N passes 2^32 from pixel 2 on, and f + 1 = 2^32 - 1 is the largest sample id there is, so the seed is right only
# where product and sum are formed in 64 bits.  D = 1 = S is full brightness; primary_only casts no secondary rays, which keeps the
# frame from saturating: the oracle's frame has 9.8 % of its plane values non-zero and 0.038 % saturated.
FREE_WINDOWS = [("lambert_distant", 2, (7, 3, 3)), ("mirror_hall", 2, (7, 3, 3)), ("primary_only", 1, (U32_MAX, U32_MAX - 1, 1))]


@pytest.mark.parametrize("mode", ORACLE_MODES)
@pytest.mark.parametrize("name, samples, win", FREE_WINDOWS, ids=lambda v: v if isinstance(v, str) else None)
def test_a_freely_chosen_window_equals_the_window_oracle(name, samples, win, mode, monkeypatch):
    sc, golden = WC.golden(name)
    assert sc.sample_count == samples
    want = WC.window_frame(name, *win)
    nonzero, saturated = WC.shares(want)
    assert nonzero > 0.05 and saturated < 0.01, (nonzero, saturated)
    assert WC.differing(want, golden) > 0  # (other samples than the default window's)
    rs = opened(sc, mode, monkeypatch)
    try:
        rs.set_sample_window(*win)
        checked_frame(rs, want, f"{name}, {mode}: window {win}")
        assert rs.sample_window() == {"next": window(*win), "last": window(*win)}
        checked_frame(rs, want, f"{name}, {mode}: window {win} again")  # (no advance, no accumulate: the same frame, now planned)
    finally:
        rs.close()


# ---- a progressive run goes on after the scene changed ---------------------------------------------------------------------------------------
MOVED = [("lambert_distant", "pan", "twist"), ("mirror_hall", "orbit90", "scale")]
_moved = {}


def moved_states(name, pose, shape):
    """The golden scene, the scene seen from `pose`, and `shape` of it seen from `pose`: Scenes with the oracle's grid and lists."""
    if name not in _moved:
        base, _ = WC.golden(name)
        bent = GC.with_arrays(base, *GC.arrays(base, shape), lists=False)
        bent.box_min, bent.grid_start, bent.grid_list = O.oracle_scene_grid(bent)
        _moved[name] = (base, CC.posed(base, pose), CC.posed(bent, pose))
    return _moved[name]


@pytest.mark.parametrize("start", [R.PIPELINE_WAVEFRONT, R.PIPELINE_MEGAKERNEL], ids=["wavefront_first", "megakernel_first"])
@pytest.mark.parametrize("name, pose, shape", MOVED)
def test_a_progressive_run_continues_over_camera_geometry_and_pipeline_changes(name, pose, shape, start):
    """The header defines a frame that continues as its addends on top of what the tile buffer holds, whatever filled it: a camera move, a
    geometry update and a change of pipeline leave the tile buffer and the window alone, so each frame is the window oracle of the state
    it is rendered in, onto the read-back of the frame before."""
    base, turned, bent = moved_states(name, pose, shape)
    S, N = base.sample_count, 8
    assert N % S == 0 and N // S >= 4
    other = R.PIPELINE_MEGAKERNEL if start == R.PIPELINE_WAVEFRONT else R.PIPELINE_WAVEFRONT

    def nothing(rs):
        pass

    def move_camera(rs):
        rs.set_camera(turned.eye, turned.eye_to_top_left, turned.left_to_right, turned.top_to_bottom, turned.pixel_size_inv)

    def move_vertices(rs):
        update_to(rs, bent)

    steps = [("the first frame", base, nothing), (f"after the camera move to {pose}", turned, move_camera),
             (f"after the update to {shape}", bent, move_vertices), ("after the change of pipeline", bent, lambda rs: rs.set_pipeline(other))]
    rs = R.ResidentScene(base, 0)
    try:
        rs.set_pipeline(start)
        rs.set_sample_window(N, 0, N, accumulate=True, advance=True)
        held = None
        for i, (what, state, change) in enumerate(steps):
            change(rs)
            f = i * S
            assert rs.sample_window()["next"] == window(N, f, N, 1, 1), what
            want = O.oracle_render_window(state, N, f, N, onto=held, threads=WC.THREADS)
            fresh = O.oracle_render_window(state, N, f, N, threads=WC.THREADS)
            if held is not None:  # the inputs: the frame adds something, and it shows that it started from the buffer
                assert WC.differing(want, held) > 0 and WC.differing(want, fresh) > 0, what
                stale = O.oracle_render_window(steps[i - 1][1], N, f, N, onto=held, threads=WC.THREADS)
                assert i == 3 or WC.differing(want, stale) > 0, f"{what}: the change does not show in the oracle's frame"
            held = checked_frame(rs, want, f"{name}, {what} (f = {f})")
            assert rs.sample_window()["last"] == window(N, f, N, 1, 1), what
    finally:
        rs.close()


# ---- split logic rounds and the ray clip -----------------------------------------------------------------------------------------------------
_soup = {}


def clip_soup():
    """The frustum soup of tests/test_ray_clip_gpu.py (128 x 128, 10 000 triangles, opaque and diffuse: the class that takes split rounds)
    at S = 2, with the window oracle's frames of the sequence {6, f, 2}."""
    if not _soup:
        sc = SCN.make_soup(128, 128, 10_000, 0.02, seed=91, samples=2)
        R.build_lists(sc)
        _soup["scene"] = sc
        _soup["frames"] = {f: O.oracle_render_window(sc, 6, f, 2, threads=WC.THREADS) for f in (0, 2, 4)}
    return _soup["scene"], _soup["frames"]


@pytest.mark.parametrize("clip", ["0", "1"])
@pytest.mark.parametrize("split", ["0", "1"])
def test_sequence_frames_equal_the_window_oracle_under_split_rounds_and_the_ray_clip(split, clip, monkeypatch):
    sc, frames = clip_soup()
    assert R.path_class(sc) == R.PATH_CLASS_OPAQUE_DIFFUSE
    assert len({tuple(p.tobytes() for p in v) for v in frames.values()}) == 3  # (three different frames)
    rs = opened(sc, "wavefront", monkeypatch, {"RT_WF_LOGIC_SPLIT": split, "RT_WF_RAY_CLIP": clip})
    try:
        assert len(rs.clip_planes()) >= 1
        rs.set_sample_window(6, 0, 2, advance=True)
        for i in range(4):  # (the first frame watched, the others planned)
            f = 2 * i % 6
            checked_frame(rs, frames[f], f"logic_split {split}, ray_clip {clip}: frame {i}, window {{6, {f}, 2}}")
            assert (rs.shade_log(4)[0] > 0) == (split == "1"), f"frame {i}: split rounds issued {rs.shade_log(4)[0]}"
        assert rs.clip_applied() == (len(rs.clip_planes()) if clip == "1" else 0)
    finally:
        rs.close()
