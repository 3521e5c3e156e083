"""Temporal accumulation on the MI355X (run with -m gpu): rtHipTemporal / rtHipTemporalDevice give, bit for bit (a NaN on both sides
counts as equal), what the numpy restatement (temporal_oracle.py) gives on the synthetic fields of temporal_cases.py -- numpy and torch,
the current and a foreign stream, with and without the counts --; ResidentScene.temporal equals the oracle chained over the read-backs,
MO.motion and the previous step's outputs for camera and geometry chains, owns the mark, resets, honours max_history = 1, filters the
accumulation but keeps the unfiltered history with denoise=, changes nothing else and refuses what it cannot do; --temporal writes what the
API returns.  Every test needs the entry points of this feature, so all of them fail without it."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library loads its HIP runtime: the order bench.py uses)

import denoise_oracle as D
import motion_cases as MC
import motion_oracle as MO
import temporal_cases as TC
import temporal_oracle as TO
from test_temporal import still
from opencl_render_amd import frontend as F, raytrace as R, scene as S

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the temporal accumulation tests cannot run (and the product has no CPU fallback)")
    MC.use_grid_builder(lambda sc: R.build_scene_grid_device(sc, 0))
    yield
    MC.use_grid_builder(R.build_scene_grid)


def assert_same(got, want, label, keys=("colour", "count")):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (label, k, g.shape, g.dtype)
        bad = np.flatnonzero(~TO.same_bits(g, w).reshape(-1))
        assert bad.size == 0, (f"{label}: {k} differs in {bad.size} of {w.size} values; first {bad[:4]}: got {g.reshape(-1)[bad[:4]]}, "
                               f"want {w.reshape(-1)[bad[:4]]}")


def on_gpu(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def gpu_args(fields):
    colour, motion, prev_t, tri, hist = fields
    return [on_gpu(v) for v in (colour, motion, prev_t, tri)] + [{k: on_gpu(v) for k, v in hist.items()}]


def to_numpy(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- synthetic arrays -----------------------------------------------------------------------------------------------------------------
PARAMS = ({}, dict(max_history=4.0, depth_tolerance=0.0), dict(max_history=1.0), dict(max_history=65536.0, depth_tolerance=0.3))


@pytest.mark.parametrize("W, H", TC.SIZES)
def test_host_and_device_entry_points_match_the_oracle_bit_for_bit(W, H):
    fields = TC.fields(W, H)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    for params in PARAMS:
        want = TO.accumulate(*fields, **params)
        assert_same(R.temporal(*fields, **params), want, f"{W}x{H} {params}: numpy")
        got = R.temporal(*gpu_args(fields), **params)
        torch.cuda.synchronize()
        assert_same(to_numpy(got), want, f"{W}x{H} {params}: torch, current stream")
        with torch.cuda.stream(side):  # a foreign stream
            got = R.temporal(*gpu_args(fields), **params)
        torch.cuda.synchronize()
        assert_same(to_numpy(got), want, f"{W}x{H} {params}: torch, a stream of the caller")
    want = TO.accumulate(*fields)
    # the counts left out: the colour alone is written
    only = R.temporal(*fields, out=dict(colour=np.full((H, W, 3), -7.0, F32)))
    assert sorted(only) == ["colour"]
    assert_same(only, want, "numpy, colour only", ("colour",))
    out = dict(colour=torch.full((H, W, 3), -7.0, device=dev))
    assert R.temporal(*gpu_args(fields), out=out)["colour"] is out["colour"]
    torch.cuda.synchronize()
    assert_same(to_numpy(out), want, "torch, colour only", ("colour",))
    both = dict(colour=torch.full((H, W, 3), -7.0, device=dev), count=torch.full((H, W), -7.0, device=dev))
    R.temporal(*gpu_args(fields), out=both, stream=side.cuda_stream)
    torch.cuda.synchronize()
    assert_same(to_numpy(both), want, "torch, given outputs on a given stream")


def test_known_answers_through_the_entry_points():
    """The known answers of tests/test_temporal.py asserted on what rtHipTemporal and rtHipTemporalDevice return, not on the oracle."""
    colour, motion, t, tri = still()
    H, W = t.shape
    for cap in (3.0, 1.0):  # a still image converges on its count, the colour unchanged
        for device in (False, True):
            hist = TO.empty_history(H, W)
            for n in range(1, 6):
                if device:
                    out = to_numpy(R.temporal(*gpu_args((colour, motion, t, tri, hist)), max_history=cap))
                else:
                    out = R.temporal(colour, motion, t, tri, hist, max_history=cap)
                assert (out["count"] == F32(min(n, cap))).all() and out["colour"].tobytes() == colour.tobytes(), (cap, device, n)
                hist = TO.next_history(out, t, tri)
    # a shift by two whole pixels: the weights are 1, 0, 0, 0; the columns whose source lies outside the image start again
    rng = np.random.default_rng(5)
    hist = dict(colour=rng.random((H, W, 3), dtype=F32), count=np.full((H, W), 1.0, F32), t=t.copy(), triangle=tri.copy())
    frame = rng.random((H, W, 3), dtype=F32)
    shift = np.zeros((H, W, 2), F32)
    shift[..., 0] = 2.0
    out = R.temporal(frame, shift, t, tri, hist)
    hc = hist["colour"][:, 2:]
    assert out["colour"][:, :W - 2].tobytes() == (hc + (frame[:, :W - 2] - hc) * F32(0.5)).tobytes() and (out["count"][:, :W - 2] == 2.0).all()
    assert out["colour"][:, W - 2:].tobytes() == frame[:, W - 2:].tobytes() and (out["count"][:, W - 2:] == 1.0).all()
    # a missed pixel over missed history accumulates (only the == arm accepts: inf - inf is a NaN), over geometry it starts again
    inf, none = np.full_like(t, np.inf), np.full_like(tri, 0xFFFFFFFF)
    sky = dict(colour=np.full((H, W, 3), 0.5, F32), count=np.full_like(t, 2.0), t=inf, triangle=none)
    assert (R.temporal(colour, motion, inf, none, sky)["count"] == 3.0).all()
    assert (R.temporal(colour, motion, inf, none, dict(sky, t=t, triangle=tri))["count"] == 1.0).all()
    # every kind of invalid history starts again
    good = dict(colour=np.full((H, W, 3), 0.5, F32), count=np.full((H, W), 4.0, F32), t=t.copy(), triangle=tri.copy())
    assert (R.temporal(colour, motion, t, tri, good)["count"] == 5.0).all()
    for name, change in {"triangle": dict(history=dict(good, triangle=tri + np.uint32(1))), "prev_t <= 0": dict(prev_t=np.zeros_like(t)),
                         "NaN motion": dict(motion=np.full_like(motion, np.nan)), "no history": dict(history=dict(good, count=np.zeros_like(t))),
                         "depth": dict(history=dict(good, t=t * F32(1.06)))}.items():
        args = dict(colour=colour, motion=motion, prev_t=t, triangle=tri, history=good)
        args.update(change)
        out = R.temporal(**args)
        assert (out["count"] == 1.0).all() and out["colour"].tobytes() == colour.tobytes(), name


def test_the_device_entry_refuses_bad_pointers_overlaps_and_foreign_streams_and_launches_nothing():
    W, H = 37, 29
    colour, motion, prev_t, tri, hist = TC.fields(W, H)
    want = TO.accumulate(colour, motion, prev_t, tri, hist)
    L = R.lib()
    p = R.temporal_params()
    arrays = [colour, motion, prev_t, tri, hist["colour"], hist["count"], hist["t"], hist["triangle"]]
    dev = [on_gpu(a) for a in arrays]
    out_c, out_n = torch.full((H, W, 3), -7.0, device="cuda:0"), torch.full((H, W), -7.0, device="cuda:0")
    ptrs = [t.data_ptr() for t in dev] + [out_c.data_ptr(), out_n.data_ptr()]
    names = ["colour", "motion", "prevT", "triangle", "histColour", "histCount", "histT", "histTriangle", "outColour", "outCount"]

    def call(stream=None, **change):
        args = list(ptrs)
        for k, v in change.items():
            args[names.index(k)] = v
        return L.rtHipTemporalDevice(0, W, H, *[C.c_void_p(a) if a else None for a in args], C.byref(p), stream)

    host = np.full((H, W, 3), -7.0, F32)
    for k in names:  # a host pointer in any place
        assert call(**{k: host.ctypes.data}) == -1 and "not device memory" in R.last_error() and k in R.last_error(), k
    assert (host == -7.0).all()
    for k in names[:8]:  # an output on top of an input, or inside it
        assert call(outColour=ptrs[names.index(k)]) == -1 and f"outColour overlaps {k}" in R.last_error(), k
        assert call(outCount=ptrs[names.index(k)] + 4) == -1 and f"outCount overlaps {k}" in R.last_error(), k
    assert call(outCount=ptrs[8] + 8) == -1 and "overlaps" in R.last_error()  # the two outputs on each other
    small = L.rtHipDeviceAlloc(0, W * H * 4 - 4)  # an exact allocation, so that a range past its end is seen
    assert small, R.last_error()
    try:
        assert call(prevT=small) == -1 and "reach past the end" in R.last_error()
    finally:
        L.rtHipDeviceFree(0, C.c_void_p(small))
    assert call(outColour=ptrs[8] + 2) == -1  # (overlaps nothing it may not, but is not 4-byte aligned and reaches past the end)
    if torch.cuda.device_count() > 1:
        other = torch.cuda.Stream(device=1)
        assert call(stream=C.c_void_p(other.cuda_stream)) == -1 and "belongs to device 1" in R.last_error()
    torch.cuda.synchronize()
    assert (out_c.cpu().numpy() == -7.0).all() and (out_n.cpu().numpy() == -7.0).all(), "a refused call wrote its output"
    assert call() == 0
    torch.cuda.synchronize()
    assert_same(dict(colour=out_c.cpu().numpy(), count=out_n.cpu().numpy()), want, "after the refusals")


# ---- the scene path -------------------------------------------------------------------------------------------------------------------
def move(rs, sc):
    rs.set_camera(sc.eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)


def frame_colour(rs):
    """What rtHipSceneTemporal gathers, from the host read-back: u16 / 65535."""
    sc = rs.scene
    return np.stack([p.reshape(sc.height, sc.width) for p in rs.readback()], -1).astype(F32) / F32(65535.0)


def same_camera(rs, sc, label):
    cam = rs.motion_reference_camera()
    for k in ("eye", "eye_to_top_left", "left_to_right", "top_to_bottom"):
        assert cam[k][:3].tobytes() == np.asarray(getattr(sc, k), F32)[:3].tobytes(), (label, k)


_flows = {}


def flows_of(key, states):
    """MO.motion of a chain's (current, reference) pairs, computed once per module."""
    if key not in _flows:
        _flows[key] = TC.chain_flows(states)
    return _flows[key]


def step(rs, flow, hist, label, **params):
    """One frame of the caller's loop after the change: render, temporal(), and the oracle on the read-back.  Returns the oracle's
    output (the next history's colour and count)."""
    rs.render()
    got = rs.temporal(**params)
    want = TO.accumulate(frame_colour(rs), flow["motion"], flow["prev_t"], flow["triangle"], hist, **params)
    assert_same(got, want, label)
    for ch, g, w in zip("RGB", got["planes"], D.quantise(want["colour"])):
        assert g.dtype == np.uint16 and np.array_equal(g, w), f"{label}: plane {ch}"
    return want


@pytest.mark.parametrize("name", list(TC.CAMERA_SCENES))
def test_a_camera_chain_equals_the_oracle_chained_over_the_read_backs(name):
    sc = MC.base_scene(name, TC.CAMERA_SCENES[name])
    chain = TC.camera_chain(sc)
    flows = flows_of(("camera", name), [(cur, ref) for _, cur, ref in chain])
    rs = R.ResidentScene(sc, 0)
    try:
        with pytest.raises(RuntimeError):
            rs.motion_reference_camera()  # no mark yet: the first call marks by itself
        hist = TO.empty_history(sc.height, sc.width)
        accepted = 0
        for i, ((pose, cur, ref), flow) in enumerate(zip(chain, flows)):
            if i:
                move(rs, cur)
            want = step(rs, flow, hist, f"{name}/{pose}")
            same_camera(rs, cur, f"{name}/{pose}: the call marks the state its frame was rendered from")
            if i == 0:
                assert (want["count"] == 1.0).all() and want["colour"].tobytes() == frame_colour(rs).tobytes()
            else:
                accepted += int((want["count"] > 1.0).sum())
            hist = TO.next_history(want, flow["t"], flow["triangle"])
        assert accepted > 0
    finally:
        rs.close()


def test_a_geometry_chain_equals_the_oracle_chained_over_the_read_backs():
    name = TC.GEOMETRY_SCENE
    sc = MC.base_scene(name, MC.GEOMETRY_SCENES[name])
    chain = TC.geometry_chain(sc)
    flows = flows_of(("geometry", name), [(cur, ref) for _, _, cur, ref in chain])
    rs = R.ResidentScene(sc, 0)
    try:
        hist = TO.empty_history(sc.height, sc.width)
        for (change, arrays, cur, ref), flow in zip(chain, flows):
            if arrays is not None:
                rs.set_vertices(cur.vertex, cur.tri_index, None)
            want = step(rs, flow, hist, f"{name}/{change}", max_history=8.0, depth_tolerance=0.1)
            hist = TO.next_history(want, flow["t"], flow["triangle"])
        assert (hist["count"] > 2.0).any()
    finally:
        rs.close()


@pytest.fixture(scope="module")
def hall():
    """(base scene, its camera chain, the chain's flows) of the small mirror hall."""
    sc = MC.base_scene("mirror_hall", (24, 16))
    chain = TC.camera_chain(sc)
    return sc, chain, flows_of(("camera", "mirror_hall"), [(cur, ref) for _, cur, ref in chain])


def test_reset_and_max_history_one_return_the_frame_itself(hall):
    sc, chain, flows = hall
    rs = R.ResidentScene(sc, 0)
    try:
        hist = TO.empty_history(sc.height, sc.width)
        for i in range(2):
            if i:
                move(rs, chain[i][1])
            want = step(rs, flows[i], hist, f"step {i}")
            hist = TO.next_history(want, flows[i]["t"], flows[i]["triangle"])
        assert (want["count"] > 1.0).any()
        rs.reset_temporal()
        move(rs, chain[2][1])
        rs.render()
        got = rs.temporal()
        assert got["colour"].tobytes() == frame_colour(rs).tobytes() and (got["count"] == 1.0).all()
        hist = TO.next_history(got, flows[2]["t"], flows[2]["triangle"])  # the reset call's output is a history like any other
        move(rs, chain[3][1])
        want = step(rs, flows[3], hist, "after the reset")
        hist = TO.next_history(want, flows[3]["t"], flows[3]["triangle"])
        move(rs, chain[4][1])
        rs.render()
        got = rs.temporal(max_history=1.0)
        assert got["colour"].tobytes() == frame_colour(rs).tobytes() and (got["count"] == 1.0).all()
        times = rs.temporal_times_ms()
        assert sorted(times) == ["accumulate", "filter", "gather", "motion"] and all(v > 0 for v in times.values()), times
    finally:
        rs.close()


def test_denoise_filters_the_accumulation_and_the_history_stays_unfiltered(hall):
    sc, chain, flows = hall
    rs = R.ResidentScene(sc, 0)
    params = dict(iterations=3, colour_inv_sigma2=0.5)
    try:
        rs.set_passes(normal=True, albedo=True)
        hist = TO.empty_history(sc.height, sc.width)
        differs = False
        for i in range(3):
            if i:
                move(rs, chain[i][1])
            rs.render()
            got = rs.temporal(denoise=params)
            surf = rs.readback_passes()
            acc = TO.accumulate(frame_colour(rs), flows[i]["motion"], flows[i]["prev_t"], flows[i]["triangle"], hist)
            want = D.denoise(acc["colour"], surf["normal"], surf["albedo"], **dict(R.DENOISE_DEFAULTS, **params))
            assert_same(got, dict(colour=want, count=acc["count"]), f"denoised step {i}")
            for ch, g, w in zip("RGB", got["planes"], D.quantise(want)):
                assert np.array_equal(g, w), f"denoised step {i}: plane {ch}"
            differs |= not np.array_equal(want, acc["colour"])
            hist = TO.next_history(acc, flows[i]["t"], flows[i]["triangle"])  # unfiltered: a filtered history fails the next step
        assert differs and (acc["count"] > 1.0).any()
    finally:
        rs.close()


def test_outputs_left_out_on_the_scene_path(hall):
    """rtHipSceneTemporal with some or all of its outputs NULL: what is returned equals the oracle, the arrays left out keep their
    sentinels, and the history advances all the same (every later step is compared with the oracle chained through all of them)."""
    sc, chain, flows = hall
    L = R.lib()
    H, W = sc.height, sc.width
    filt = dict(iterations=2, colour_inv_sigma2=0.5)

    def call(rs, outs, denoise=None):
        """outs: the names given; the others are NULL.  Returns every array, those left out still holding their sentinels."""
        a = dict(colour=np.full((H, W, 3), -7.0, F32), r=np.full((H, W), 12345, np.uint16), g=np.full((H, W), 12345, np.uint16),
                 b=np.full((H, W), 12345, np.uint16), count=np.full((H, W), -7.0, F32))
        d = R.denoise_params(**denoise) if denoise is not None else None
        ptrs = [a[k].ctypes.data_as(C.c_void_p) if k in outs else None for k in ("colour", "r", "g", "b", "count")]
        assert L.rtHipSceneTemporal(rs.handle, C.byref(R.temporal_params()), C.byref(d) if d is not None else None, *ptrs) == 0, R.last_error()
        for k in a:
            if k not in outs:
                assert (a[k] == (-7.0 if a[k].dtype == F32 else 12345)).all(), f"{k} was left out but written"
        return a

    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_passes(normal=True, albedo=True)
        hist = TO.empty_history(H, W)
        plan = ((("colour", "count"), None), (("r", "g", "b"), None), (("r", "g", "b"), filt), ((), filt), (("g",), None))
        for i, (outs, denoise) in enumerate(plan):
            if i:
                move(rs, chain[i][1])
            rs.render()
            got = call(rs, outs, denoise)
            acc = TO.accumulate(frame_colour(rs), flows[i]["motion"], flows[i]["prev_t"], flows[i]["triangle"], hist)
            shown = acc["colour"]
            if denoise is not None:
                surf = rs.readback_passes()
                shown = D.denoise(acc["colour"], surf["normal"], surf["albedo"], **dict(R.DENOISE_DEFAULTS, **denoise))
            if "colour" in outs:
                assert_same(got, dict(colour=shown, count=acc["count"]), f"step {i} {outs}")
            for ch, w in zip("rgb", D.quantise(shown)):
                if ch in outs:
                    assert np.array_equal(got[ch], w), f"step {i} {outs}: plane {ch}"
            times = rs.temporal_times_ms()
            assert times["motion"] > 0 and times["accumulate"] > 0 and times["filter"] >= 0, times
            hist = TO.next_history(acc, flows[i]["t"], flows[i]["triangle"])
        assert (acc["count"] > 1.0).any()
        move(rs, chain[0][1])  # one more frame with every output: the history came through the calls above untouched
        rs.render()
        flow = MO.motion(chain[0][1], chain[4][1])
        got = rs.temporal()
        want = TO.accumulate(frame_colour(rs), flow["motion"], flow["prev_t"], flow["triangle"], hist)
        assert_same(got, want, "after the partial calls")
        assert (want["count"] > 2.0).any()
    finally:
        rs.close()


def storage_bytes(W, H):
    """The header's formula ("TEMPORAL ACCUMULATION", rtHipSceneTemporal, storage)."""
    n = W * H
    part = lambda b: (b + 255) & ~255  # noqa: E731
    return 2 * (part(12 * n) + 3 * part(4 * n)) + part(8 * n) + part(4 * n) + part(12 * n) + 3 * part(2 * n)


def test_nothing_else_changes(hall):
    sc, chain, flows = hall
    cur = chain[1][1]
    rs = R.ResidentScene(sc, 0)
    idle = R.ResidentScene(sc, 0)  # a scene that never calls holds no temporal storage
    try:
        idle_bytes = idle.bytes()
        rs.set_passes(alpha=True, depth=True, triangle=True)
        move(rs, cur)  # (a camera move makes storage of its own the first time and swaps the list sets: both poses are visited before
        move(rs, sc)   # anything is recorded, so that what grows below is the temporal storage alone)
        rs.render()
        planes, passes = rs.readback(), rs.readback_passes()
        rs.mark_motion()
        rs.motion()  # (the motion pass's own storage likewise)
        pointers, bytes0 = rs.pointers(), rs.bytes()
        rs.temporal()
        assert rs.bytes() - bytes0 == storage_bytes(sc.width, sc.height)
        rs.reset_temporal()
        rs.temporal(max_history=2.0)
        assert rs.bytes() - bytes0 == storage_bytes(sc.width, sc.height) and rs.pointers() == pointers
        move(rs, cur)
        moved = rs.pointers()
        rs.render()
        rs.temporal()
        assert rs.bytes() - bytes0 == storage_bytes(sc.width, sc.height) and rs.pointers() == moved
        move(rs, sc)
        rs.render()
        assert all(np.array_equal(a, b) for a, b in zip(planes, rs.readback()))
        again = rs.readback_passes()
        for k in passes:
            assert np.array_equal(np.asarray(passes[k]).view(np.uint8), np.asarray(again[k]).view(np.uint8)), k
        rs.mark_motion()  # a mark of the caller's own after the calls: motion() measures against it
        move(rs, cur)
        got = rs.motion()
        for k, w in flows[1].items():
            assert MO.same_bits(got[k], w).all(), k
        idle.render()
        idle.readback()
        assert idle.bytes() == idle_bytes
    finally:
        rs.close()
        idle.close()


def test_scene_refusals_launch_nothing():
    sc = MC.base_scene("axis_near_axis_mixed", MC.CAMERA_SCENES["axis_near_axis_mixed"])  # several tiles
    L = R.lib()
    H, W = sc.height, sc.width
    colour, count = np.full((H, W, 3), -7.0, F32), np.full((H, W), -7.0, F32)
    planes = [np.full((H, W), 12345, np.uint16) for _ in range(3)]

    def call(rs, params=None, denoise=None):
        return L.rtHipSceneTemporal(rs.handle, C.byref(params or R.temporal_params()), C.byref(denoise) if denoise else None,
                                    *[a.ctypes.data_as(C.c_void_p) for a in [colour] + planes + [count]])

    tiles = np.arange(R.tile_count(W, H), dtype=np.uint32)
    for part in (tiles[1:], np.concatenate([tiles, tiles[:1]])):
        rs = R.ResidentScene(sc, 0, part)
        try:
            rs.render()
            bytes0 = rs.bytes()
            assert call(rs) == -1 and "every tile of the image" in R.last_error()
            with pytest.raises(RuntimeError, match="every tile of the image"):
                rs.temporal()
            assert rs.bytes() == bytes0
        finally:
            rs.close()
    rs = R.ResidentScene(sc, 0)
    try:
        rs.render()
        bytes0 = rs.bytes()
        for passes in ({}, dict(normal=True), dict(albedo=True, depth=True)):
            rs.set_passes(**passes)
            rs.render()
            bytes0 = rs.bytes()
            assert call(rs, denoise=R.denoise_params()) == -1 and "normal and the albedo pass" in R.last_error()
            assert rs.bytes() == bytes0, passes
        assert call(rs, params=R.temporal_params(max_history=0.0)) == -1 and "maxHistory" in R.last_error()
        assert rs.bytes() == bytes0
        assert call(rs, params=R.temporal_params(depth_tolerance=-1.0)) == -1 and "depthTolerance" in R.last_error()
        assert rs.bytes() == bytes0
        rs.set_passes(normal=True, albedo=True)
        rs.render()
        bytes0 = rs.bytes()
        assert call(rs, denoise=R.denoise_params(iterations=13)) == -1 and "iterations 13" in R.last_error()
        assert rs.bytes() == bytes0
        with pytest.raises(RuntimeError):
            rs.motion_reference_camera()  # a refused call did not mark either
    finally:
        rs.close()
    assert (colour == -7.0).all() and (count == -7.0).all() and all((p == 12345).all() for p in planes)


def test_command_line_writes_what_the_api_returns(tmp_path):
    from opencl_render_amd import __main__ as M
    args = ["--scene", "soup", "--width", "64", "--height", "48", "--samples", "1", "--triangles", "20000", "--out", str(tmp_path / "img.bmp")]
    assert M.main(args + ["--orbit", "3", "--temporal", str(tmp_path / "acc.pfm")]) == 0
    assert M.main(args + ["--orbit", "3", "--temporal", str(tmp_path / "acc.ppm"), "--motion", str(tmp_path / "mv")]) == 0
    assert M.main(args + ["--orbit", "3", "--temporal", str(tmp_path / "accd.pfm"), "--denoise", str(tmp_path / "den.ppm")]) == 0
    sc = S.make_soup(64, 48, 20000, 0.02, samples=1)
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    rs = R.ResidentScene(sc, 0)
    try:  # with --denoise the filter runs on the accumulation
        rs.set_passes(normal=True, albedo=True)
        for i, position in enumerate(R.orbit_positions(np.zeros(3, F32), np.float32([0, 0, 3]), 3)):
            rs.look_at(position, np.float32([0, 0, 3]), (0, 1, 0), np.radians(M.parser().get_default("fov")))
            rs.render()
            want = rs.temporal(denoise={})
            assert open(tmp_path / f"accd_{i:03d}.pfm", "rb").read() == b"PF\n64 48\n-1.0\n" + want["colour"][::-1].astype("<f4").tobytes()
    finally:
        rs.close()
    rs = R.ResidentScene(sc, 0)
    try:
        longer = 0
        for i, position in enumerate(R.orbit_positions(np.zeros(3, F32), np.float32([0, 0, 3]), 3)):
            rs.look_at(position, np.float32([0, 0, 3]), (0, 1, 0), np.radians(M.parser().get_default("fov")))
            if i == 0:
                rs.mark_motion()
            flow = rs.motion()
            rs.render()
            want = rs.temporal()
            assert open(tmp_path / f"acc_{i:03d}.pfm", "rb").read() == b"PF\n64 48\n-1.0\n" + want["colour"][::-1].astype("<f4").tobytes()
            F.write_ppm(str(tmp_path / "want.ppm"), *want["planes"])
            assert open(tmp_path / f"acc_{i:03d}.ppm", "rb").read() == open(tmp_path / "want.ppm", "rb").read()
            with np.load(tmp_path / f"mv_{i:03d}.npz") as z:  # --motion beside --temporal still measures against the frame before
                assert all(MO.same_bits(z[k], flow[k]).all() for k in flow)
            longer += int((want["count"] > 1.0).any())
        assert longer == 2  # frame 0 has no history, the others accept some
    finally:
        rs.close()
    with pytest.raises(SystemExit):
        M.parse_args(["--temporal", str(tmp_path / "acc.pfm")])
    with pytest.raises(SystemExit):
        M.parse_args(["--orbit", "2", "--temporal", str(tmp_path / "acc.png")])
