"""The temporal clamp on the MI355X (run with -m gpu): rtHipTemporalClamp / rtHipTemporalClampDevice and their moments twins give, bit
for bit (a NaN on both sides counts as equal), what the numpy restatement (temporal_clamp_oracle.py) gives on the perturbed fields of
temporal_clamp_cases.py, at the image sizes where a partly filled block, a one-pixel second block or a halo between blocks can go wrong;
the device entries refuse what they must and write nothing; a resident scene under set_temporal_clamp equals the oracle chained over the
read-backs through a relight, with and without moments; after the relight no accumulated colour lies outside the new frame's 3x3 box
(and without the clamp some do); a scene whose clamp is off returns what it always returned; and --relight N --temporal PATH
--temporal-clamp writes what the API returns.  Every test needs the entry points of this feature, so all of them fail without it."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library loads its HIP runtime: the order bench.py uses)

import denoise_oracle as D
import motion_cases as MC
import motion_oracle as MO
import temporal_clamp_cases as CC
import temporal_clamp_oracle as CO
import temporal_oracle as TO
import variance_oracle as VO
from opencl_render_amd import raytrace as R

pytestmark = pytest.mark.gpu
F32 = np.float32
PLAIN, WITH_MOMENTS = ("colour", "count"), ("colour", "count", "moments", "variance")


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the temporal clamp's tests cannot run (and the product has no CPU fallback)")
    MC.use_grid_builder(lambda sc: R.build_scene_grid_device(sc, 0))
    yield
    MC.use_grid_builder(R.build_scene_grid)


def assert_same(got, want, label, keys=PLAIN):
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
def check_entry_points(fields, moments, label, clamps):
    call, keys = (R.temporal_moments, WITH_MOMENTS) if moments else (R.temporal, PLAIN)
    dev = gpu_args(fields)
    for clamp in clamps:
        want = CO.accumulate(*fields, **clamp)
        assert_same(call(*fields, clamp=clamp), want, f"{label} {clamp}: numpy", keys)
        got = call(*dev, clamp=clamp)
        torch.cuda.synchronize()
        assert_same(to_numpy(got), want, f"{label} {clamp}: torch", keys)


@pytest.mark.parametrize("W, H", CC.SHAPES)
def test_host_and_device_entry_points_match_the_oracle_bit_for_bit(W, H):
    clamps = [dict(mode=mode, gamma=gamma) for mode in CC.MODES for gamma in CC.GAMMAS]
    for moments in (False, True):
        fields = CC.fields(W, H, moments=moments)
        check_entry_points(fields, moments, f"{W}x{H} moments {moments}", clamps)
        call, keys = (R.temporal_moments, WITH_MOMENTS) if moments else (R.temporal, PLAIN)
        params = dict(max_history=4.0, depth_tolerance=0.0)
        want = CO.accumulate(*fields, **params)
        side = torch.cuda.Stream(torch.device("cuda", 0))
        with torch.cuda.stream(side):  # a stream of the caller, the default clamp, other temporal parameters
            got = call(*gpu_args(fields), clamp={}, **params)
        torch.cuda.synchronize()
        assert_same(to_numpy(got), want, f"{W}x{H} moments {moments}: torch, a stream of the caller", keys)
    fields = CC.fields(W, H)
    out = dict(colour=torch.full((H, W, 3), -7.0, device="cuda:0"))  # the counts left out
    assert R.temporal(*gpu_args(fields), out=out, clamp={})["colour"] is out["colour"]
    torch.cuda.synchronize()
    assert_same(to_numpy(out), CO.accumulate(*fields), "torch, colour only", ("colour",))


def test_special_values_through_the_entry_points():
    W, H = CC.SPECIAL_SHAPE
    clamps = [dict(mode=mode, gamma=gamma) for mode in CC.MODES for gamma in (0.0, 1.0)]
    for moments in (False, True):
        check_entry_points(CC.special_fields(W, H, moments=moments), moments, f"special moments {moments}", clamps)


def test_known_answer_through_the_entry_points():
    """A constant frame over a different, fully valid history: the frame itself in every mode; the old colour drags on without."""
    from test_temporal_clamp import constant_case
    f = constant_case()
    plain = R.temporal(*f)
    assert (plain["count"] == 5.0).all() and not (plain["colour"] == f[0]).any()
    for mode in CC.MODES:
        for gamma in CC.GAMMAS:
            out = R.temporal(*f, clamp=dict(mode=mode, gamma=gamma))
            assert out["colour"].tobytes() == f[0].tobytes() and out["count"].tobytes() == plain["count"].tobytes(), (mode, gamma)
            out = to_numpy(R.temporal(*gpu_args(f), clamp=dict(mode=mode, gamma=gamma)))
            assert out["colour"].tobytes() == f[0].tobytes() and out["count"].tobytes() == plain["count"].tobytes(), (mode, gamma)


def test_the_device_entries_refuse_bad_pointers_overlaps_streams_and_parameters_and_launch_nothing():
    W, H = 33, 9
    colour, motion, prev_t, tri, hist = CC.fields(W, H, moments=True)
    L = R.lib()
    p, good = R.temporal_params(), R.temporal_clamp_params()
    arrays = [colour, motion, prev_t, tri, hist["colour"], hist["count"], hist["t"], hist["triangle"], hist["moments"]]
    dev = [on_gpu(a) for a in arrays]
    outs = dict(outColour=torch.full((H, W, 3), -7.0, device="cuda:0"), outCount=torch.full((H, W), -7.0, device="cuda:0"),
                outMoments=torch.full((H, W, 2), -7.0, device="cuda:0"), outVariance=torch.full((H, W), -7.0, device="cuda:0"))
    inputs = ["colour", "motion", "prevT", "triangle", "histColour", "histCount", "histT", "histTriangle", "histMoments"]
    where = dict(zip(inputs, (t.data_ptr() for t in dev)), **{k: v.data_ptr() for k, v in outs.items()})
    entries = ((L.rtHipTemporalClampDevice, inputs[:8] + ["outColour", "outCount"]),
               (L.rtHipTemporalMomentsClampDevice, inputs + ["outColour", "outCount", "outMoments", "outVariance"]))
    host = np.full((H, W, 3), -7.0, F32)
    for entry, names in entries:
        def call(stream=None, clamp=good, **change):
            args = [change.get(k, where[k]) for k in names]
            return entry(0, W, H, *[C.c_void_p(a) if a else None for a in args], C.byref(p), C.byref(clamp) if clamp is not None else None, stream)

        for k in names:  # a host pointer in any place
            assert call(**{k: host.ctypes.data}) == -1 and "not device memory" in R.last_error() and k in R.last_error(), k
        for k in names:
            if k.startswith("out"):
                continue
            assert call(outColour=where[k]) == -1 and f"outColour overlaps {k}" in R.last_error(), k  # an output on top of an input
            assert call(outCount=where[k] + 4) == -1 and f"outCount overlaps {k}" in R.last_error(), k  # or inside it
        assert call(outCount=where["outColour"] + 8) == -1 and "overlaps" in R.last_error()  # two outputs on each other
        assert call(clamp=None) == -1 and "null parameters" in R.last_error()
        for bad in (dict(mode=0), dict(mode=4), dict(gamma=np.nan), dict(gamma=-1.0), dict(gamma=np.inf)):
            assert call(clamp=R.temporal_clamp_params(**bad)) == -1 and "temporal clamp" in R.last_error(), bad
        if torch.cuda.device_count() > 1:
            other = torch.cuda.Stream(device=1)
            assert call(stream=C.c_void_p(other.cuda_stream)) == -1 and "belongs to device 1" in R.last_error()
    torch.cuda.synchronize()
    assert (host == -7.0).all() and all((v.cpu().numpy() == -7.0).all() for v in outs.values()), "a refused call wrote its output"
    fields = (colour, motion, prev_t, tri, hist)
    want = CO.accumulate(*fields)
    for entry, names in entries:
        for v in outs.values():
            v.fill_(-7.0)
        assert entry(0, W, H, *[C.c_void_p(where[k]) for k in names], C.byref(p), C.byref(good), None) == 0, R.last_error()
        torch.cuda.synchronize()
        got = dict(colour=outs["outColour"].cpu().numpy(), count=outs["outCount"].cpu().numpy(), moments=outs["outMoments"].cpu().numpy(),
                   variance=outs["outVariance"].cpu().numpy())
        assert_same(got, want, "after the refusals", WITH_MOMENTS if len(names) == 13 else PLAIN)


# ---- the scene path: a relight under a still camera -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def relit():
    """(scene, its flow against itself, the two light sets, a ResidentScene the chains below share: each starts with a reset)."""
    sc = MC.base_scene(CC.RELIGHT_SCENE, CC.RELIGHT_SIZE)
    assert (sc.width, sc.height) == CC.RELIGHT_SIZE
    flow = MO.motion(sc, sc)
    hit = flow["triangle"] != 0xFFFFFFFF
    assert hit.mean() > 0.1 and np.abs(flow["motion"][hit]).max() < 1e-3  # (a still camera: the flow is rounding noise)
    rs = R.ResidentScene(sc, 0)
    try:
        yield sc, flow, CC.relight_lights(), rs
    finally:
        rs.close()


def frame_colour(rs):
    """What rtHipSceneTemporal gathers, from the host read-back: u16 / 65535."""
    sc = rs.scene
    return np.stack([p.reshape(sc.height, sc.width) for p in rs.readback()], -1).astype(F32) / F32(65535.0)


def chain(rs, lights, clamp, variance=False):
    """reset, then for each light set: set_lights, render, temporal() (or temporal_variance()).  Returns [(what the call returned, the
    frame's colour)]."""
    rs.reset_temporal()
    if clamp is None:
        rs.set_temporal_clamp(None)
    else:
        rs.set_temporal_clamp(**clamp)
    steps = []
    for spec in lights:
        rs.set_lights(spec)
        rs.render()
        got = rs.temporal_variance() if variance else rs.temporal()
        steps.append((got, frame_colour(rs)))
    return steps


def oracle_chain(frames, flow, clamp, moments=False):
    """The oracle over the read-back frames: clamp None is the unclamped oracle (temporal_oracle.py or variance_oracle.py)."""
    H, W = flow["t"].shape
    hist = VO.empty_history(H, W) if moments else TO.empty_history(H, W)
    outs = []
    for frame in frames:
        if clamp is None:
            out = (VO if moments else TO).accumulate(frame, flow["motion"], flow["prev_t"], flow["triangle"], hist)
        else:
            out = CO.accumulate(frame, flow["motion"], flow["prev_t"], flow["triangle"], hist, **clamp)
        outs.append(out)
        hist = CO.next_history(out, flow["t"], flow["triangle"])
    return outs


def assert_step(got, want, label, keys=PLAIN):
    assert_same(got, want, label, keys)
    for ch, g, w in zip("RGB", got["planes"], D.quantise(want["colour"])):
        assert g.dtype == np.uint16 and np.array_equal(g, w), f"{label}: plane {ch}"


@pytest.mark.parametrize("clamp", [dict(mode=3, gamma=1.0), dict(mode=1, gamma=1.0), dict(mode=2, gamma=0.5)], ids=["both", "minmax", "variance"])
def test_a_relight_under_the_clamp_equals_the_oracle_chained_over_the_read_backs(relit, clamp):
    sc, flow, lights, rs = relit
    steps = chain(rs, lights, clamp)
    assert rs.temporal_clamp() == clamp
    frames = [f for _, f in steps]
    assert not np.array_equal(frames[0], frames[1]), "the dimmed lights render the same frame"
    wants = oracle_chain(frames, flow, clamp)
    for i, ((got, _), want) in enumerate(zip(steps, wants)):
        assert_step(got, want, f"{clamp} step {i}")
    assert (wants[1]["count"] == 2.0).mean() > 0.2 and (wants[1]["moved"] != 0).any(), "the relight step pulled no history in"
    assert rs.temporal_times_ms()["accumulate"] > 0
    # temporal_variance() under the same clamp: the same colour and count; the moments are not clamped, so the variance is the
    # unclamped moments chain's
    steps = chain(rs, lights, clamp, variance=True)
    assert all(np.array_equal(a, b) for a, b in zip(frames, [f for _, f in steps]))
    wants_m, plain_m = oracle_chain(frames, flow, clamp, moments=True), oracle_chain(frames, flow, None, moments=True)
    for i, ((got, _), want, plain) in enumerate(zip(steps, wants_m, plain_m)):
        assert_step(got, want, f"{clamp} with moments, step {i}", ("colour", "count", "variance"))
        assert_same(want, wants[i], f"{clamp} step {i}: the oracle with moments against the one without")
        assert_same(want, plain, f"{clamp} step {i}: moments", ("count", "moments", "variance"))
        assert_same(got, plain, f"{clamp} step {i}: the variance of the unclamped moments", ("variance",))
    assert (plain_m[1]["variance"] > 0).any()


def test_after_a_relight_no_clamped_colour_lies_outside_the_new_frames_box(relit):
    """What the feature is for.  Without the clamp the old lighting is still in the accumulation after the edit: pixels lie outside the
    3x3 min/max box of the frame they belong to.  With the min/max box, alone or intersected, none does."""
    sc, flow, lights, rs = relit
    (_, _), (off, frame) = chain(rs, lights, None)
    hit = flow["triangle"] != 0xFFFFFFFF
    outside = CO.outside_minmax(off["colour"], frame)
    print(f"clamp off: {int(outside.sum())} of {int(hit.sum())} hit pixels lie outside their box after the relight")
    assert outside.sum() >= 1 and (off["count"][hit] == 2.0).mean() > 0.9
    for clamp in (dict(mode=1), dict(mode=3)):
        (_, _), (on, again) = chain(rs, lights, clamp)
        assert np.array_equal(again, frame)
        outside = CO.outside_minmax(on["colour"], frame)
        print(f"clamp {clamp}: {int(outside.sum())} pixels outside")
        assert outside.sum() == 0, clamp
        assert on["count"].tobytes() == off["count"].tobytes()  # the clamp leaves the history length alone


def test_a_scene_whose_clamp_is_off_returns_what_it_always_returned(relit):
    sc, flow, lights, rs = relit
    rs.set_temporal_clamp("minmax", 0.25)
    assert rs.temporal_clamp() == dict(mode=1, gamma=0.25)
    rs.set_temporal_clamp()
    assert rs.temporal_clamp() == dict(mode=3, gamma=1.0)
    with pytest.raises(RuntimeError, match="mode 4"):
        rs.set_temporal_clamp(4)
    with pytest.raises(RuntimeError, match="gamma"):
        rs.set_temporal_clamp(1, -1.0)
    assert rs.temporal_clamp() == dict(mode=3, gamma=1.0)  # a refused setting changes nothing
    bytes0 = rs.bytes()
    used = chain(rs, lights, None)  # set_temporal_clamp(None) after use
    assert rs.temporal_clamp() is None and rs.bytes() == bytes0
    frames = [f for _, f in used]
    wants = oracle_chain(frames, flow, None)
    for i, ((got, _), want) in enumerate(zip(used, wants)):
        assert_step(got, want, f"clamp turned off, step {i}")
    fresh = R.ResidentScene(sc, 0)  # a scene that never set it
    try:
        assert fresh.temporal_clamp() is None
        for i, spec in enumerate(lights):
            fresh.set_lights(spec)
            fresh.render()
            got = fresh.temporal()
            assert np.array_equal(frame_colour(fresh), frames[i])
            assert_step(got, wants[i], f"clamp never set, step {i}")
    finally:
        fresh.close()
    clamped = oracle_chain(frames, flow, dict(mode=3, gamma=1.0))
    assert not np.array_equal(clamped[1]["colour"], wants[1]["colour"])  # (the chains differ where it matters)


def test_command_line_relights_under_the_clamp(tmp_path):
    """--relight 3 --temporal PATH --temporal-clamp through the command line's own loop writes what the API returns, differs from the
    run without the clamp from the first relit frame on, and the options refuse what they cannot do."""
    from opencl_render_amd import __main__ as cli, scene as S
    base = ["--scene", "soup", "--triangles", "400", "--width", "48", "--height", "36", "--samples", "2", "--relight", "3"]
    assert cli.main(base + ["--out", str(tmp_path / "a.ppm"), "--temporal", str(tmp_path / "off.pfm")]) == 0
    assert cli.main(base + ["--out", str(tmp_path / "b.ppm"), "--temporal", str(tmp_path / "on.pfm"), "--temporal-clamp"]) == 0
    assert cli.main(base + ["--out", str(tmp_path / "c.ppm"), "--temporal", str(tmp_path / "mm.pfm"), "--temporal-clamp", "0.5",
                            "--temporal-clamp-mode", "minmax"]) == 0
    sc = S.make_soup(48, 36, 400, 0.02, samples=2)
    R.build_lists(sc)
    lights = R.scene_lights(sc)
    for name, clamp in (("off", None), ("on", dict(mode=3, gamma=1.0)), ("mm", dict(mode=1, gamma=0.5))):
        rs = R.ResidentScene(sc, 0)
        try:
            if clamp:
                rs.set_temporal_clamp(**clamp)
            for i in range(3):
                if i:
                    rs.set_lights(R.relight(lights, i, 3))
                rs.render()
                want = rs.temporal()
                assert (tmp_path / f"{name}_{i:03d}.pfm").read_bytes() == b"PF\n48 36\n-1.0\n" + want["colour"][::-1].astype("<f4").tobytes(), (name, i)
        finally:
            rs.close()
    assert (tmp_path / "on_000.pfm").read_bytes() == (tmp_path / "off_000.pfm").read_bytes()
    assert (tmp_path / "on_001.pfm").read_bytes() != (tmp_path / "off_001.pfm").read_bytes()
    for bad in (["--temporal-clamp"], ["--orbit", "2", "--temporal-clamp-mode", "minmax", "--temporal", str(tmp_path / "x.pfm")],
                ["--orbit", "2", "--temporal", str(tmp_path / "x.pfm"), "--temporal-clamp", "-1"],
                ["--orbit", "2", "--temporal", str(tmp_path / "x.pfm"), "--temporal-clamp", "nan"],
                ["--temporal", str(tmp_path / "x.pfm"), "--temporal-clamp"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
