"""Ray queries on the MI355X (run with -m gpu): rtHipSceneIntersect / rtHipSceneIntersectDevice answer exactly what the restatement of
the reference's grid walk (rt_oracle_grid_trace) answers -- triangle, and t, abL, acL compared as bits -- on every ray set of
query_cases.py for every golden scene, the AXIS scenes and a 1M-triangle soup; the host and device entry points, numpy and torch, agree;
batches of 0, 1, 257 rays and across staging chunks; queries between frames change nothing; every kind of instance answers alike; a
host pointer never reaches the kernel."""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the library loads its HIP runtime: the order bench.py uses)

import query_cases as Q
import scenarios
from conftest import golden_names, load_golden_scene
from opencl_render_amd import raytrace as R, scene as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the ray query tests cannot run (and the product has no CPU fallback)")


def query(rs_scene, rs):
    return rs_scene.intersect(rs["o"], rs["d"], rs["tmin"], rs["tmax"], rs["excluded"])


def assert_same(got, want, what):
    bad = Q.mismatches(dict(triangle=got["triangle"], t=got["t"], ab=got["ab"], ac=got["ac"]), want)
    assert bad.size == 0, (f"{what}: {bad.size} of {len(want['t'])} rays differ; first {bad[:4]}: got tri {got['triangle'][bad[:4]]} "
                           f"t {got['t'][bad[:4]]}, want tri {want['triangle'][bad[:4]]} t {want['t'][bad[:4]]}")


def check_scene(sc, n, what, seed=3):
    rs_scene = R.ResidentScene(sc)
    try:
        for kind, rs in Q.all_sets(sc, n=n, seed=seed).items():
            assert_same(query(rs_scene, rs), Q.oracle_answers(sc, rs), f"{what}/{kind}")
    finally:
        rs_scene.close()


@pytest.mark.parametrize("name", golden_names())
def test_golden_scenes_bit_exact(name):
    sc, _ = load_golden_scene(name)
    check_scene(sc, 3000, name)


@pytest.mark.parametrize("make", scenarios.AXIS, ids=lambda f: f.__name__)
def test_axis_scenes_bit_exact(make):
    check_scene(make(), 3000, make.__name__)


def test_million_triangle_soup_bit_exact():
    sc = S.make_soup(256, 144, 1_000_000, 0.004, seed=12345, name="soup_1m")
    R.build_lists(sc)
    rs_scene = R.ResidentScene(sc)
    try:
        sets = Q.all_sets(sc, n=40_000, seed=11)
        sets["camera"] = Q.camera_rays(sc)  # every pixel centre
        for kind, rs in sets.items():
            got = query(rs_scene, rs)
            assert_same(got, Q.oracle_answers(sc, rs), f"soup_1m/{kind}")
            if kind in ("camera", "segments"):
                assert got["hit"].mean() > 0.05, f"soup_1m/{kind}: hit rate {got['hit'].mean():.3f}"
    finally:
        rs_scene.close()


@pytest.fixture(scope="module")
def axis_scene():
    return scenarios.axis_by_name("axis_near_axis_mixed")()


@pytest.fixture(scope="module")
def axis_sets(axis_scene):
    return Q.concat(*Q.all_sets(axis_scene, n=700, seed=5).values())  # 3500 rays: not a multiple of 256


def test_host_device_numpy_torch_and_small_counts_agree(axis_scene, axis_sets):
    sc, rs = axis_scene, axis_sets
    want = Q.oracle_answers(sc, rs)
    rsc = R.ResidentScene(sc)
    try:
        host = query(rsc, rs)
        assert_same(host, want, "host entry")
        dev = torch.device("cuda", 0)
        tt = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(dev) for k, v in rs.items()}
        got = rsc.intersect(tt["o"], tt["d"], tt["tmin"], tt["tmax"], tt["excluded"])
        torch.cuda.synchronize()
        assert all(v.device == dev for v in got.values())
        g = dict(triangle=got["triangle"].view(torch.int32).cpu().numpy().view(np.uint32), t=got["t"].cpu().numpy(),
                 ab=got["ab"].cpu().numpy(), ac=got["ac"].cpu().numpy())
        assert_same(g, want, "device entry (torch)")
        for k in ("hit", "material", "mesh"):
            assert np.array_equal(got[k].cpu().numpy(), host[k]), k
        assert np.array_equal(Q.bits(got["position"].cpu().numpy()), Q.bits(host["position"]))
        # a count of 0, of 1 and one that is not a multiple of 256
        for n in (0, 1, 257):
            part = Q.take(rs, np.arange(n))
            got_n = query(rsc, part)
            assert_same(got_n, Q.take(want, np.arange(n)), f"count {n}")
            tn = rsc.intersect(tt["o"][:n], tt["d"][:n], tt["tmin"][:n], tt["tmax"][:n], tt["excluded"][:n])
            assert tn["t"].shape == (n,)
            assert np.array_equal(Q.bits(tn["t"].cpu().numpy()), Q.bits(got_n["t"]))
        # no exclusion and scalar limits broadcast like the per-ray arrays
        a = rsc.intersect(rs["o"], rs["d"])
        b = rsc.intersect(rs["o"], rs["d"], np.zeros(len(rs["o"]), np.float32), np.full(len(rs["o"]), np.inf, np.float32),
                          np.full(len(rs["o"]), 0xFFFFFFFF, np.uint32))
        assert np.array_equal(a["triangle"], b["triangle"]) and np.array_equal(Q.bits(a["t"]), Q.bits(b["t"]))
        with pytest.raises(ValueError):
            rsc.intersect(tt["o"].cpu(), tt["d"])
        with pytest.raises(ValueError):
            rsc.intersect(rs["o"], rs["d"][:-1])
    finally:
        rsc.close()


def test_torch_query_on_a_stream_that_is_not_the_current_one(axis_scene, axis_sets):
    """intersect(..., stream=s) with s neither torch's current stream nor the null stream: the packing before it and the read-outs after it
    run on the current stream and must be ordered against s; the buffers must outlive the query.  Several calls in a row, with other work
    enqueued on the current stream in between, all answer like the oracle."""
    sc, rs = axis_scene, axis_sets
    want = Q.oracle_answers(sc, rs)
    dev = torch.device("cuda", 0)
    rsc = R.ResidentScene(sc)
    try:
        side = torch.cuda.Stream(dev)
        tt = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(dev) for k, v in rs.items()}
        for current in (torch.cuda.Stream(dev), torch.cuda.default_stream(dev)):
            with torch.cuda.stream(current):
                current.wait_stream(torch.cuda.default_stream(dev))
                outs = []
                for rep in range(3):
                    busy = torch.randn(4096, 4096, device=dev)  # work on the current stream ahead of the packing
                    busy = busy @ busy
                    outs.append(rsc.intersect(tt["o"], tt["d"], tt["tmin"], tt["tmax"], tt["excluded"], stream=side.cuda_stream))
                    del busy
                got = [dict(triangle=o["triangle"].view(torch.int32).cpu().numpy().view(np.uint32), t=o["t"].cpu().numpy(),
                            ab=o["ab"].cpu().numpy(), ac=o["ac"].cpu().numpy()) for o in outs]
            for rep, g in enumerate(got):
                assert_same(g, want, f"stream {side.cuda_stream:#x} under current stream {current.cuda_stream:#x}, call {rep}")
    finally:
        torch.cuda.synchronize()
        rsc.close()


def test_host_batch_across_staging_chunks(axis_scene, axis_sets, monkeypatch):
    monkeypatch.setenv("RT_HIP_QUERY_RAYS", "999")  # chunks of 999 rays (odd: the staging layout keeps the 16-byte records aligned): four launches
    rsc = R.ResidentScene(axis_scene)
    try:
        before = rsc.bytes()
        got = query(rsc, axis_sets)
        assert rsc.bytes() == before + 999 * 52  # the staging chunk, counted once it exists
        assert_same(got, Q.oracle_answers(axis_scene, axis_sets), "chunked")
    finally:
        rsc.close()


def test_queries_between_frames_change_nothing():
    sc, gold = load_golden_scene("mirror_hall")
    rs = Q.concat(*Q.all_sets(sc, n=1000, seed=9).values())
    rsc = R.ResidentScene(sc)
    try:
        rsc.render()
        first = query(rsc, rs)
        rsc.render()
        planes = rsc.readback()
        second = query(rsc, rs)
        for got, want in zip(planes, gold):
            assert np.array_equal(got.reshape(want.shape), want)
        for k in ("triangle", "t", "ab", "ac"):
            assert np.array_equal(Q.bits(first[k]) if k != "triangle" else first[k], Q.bits(second[k]) if k != "triangle" else second[k])
        assert_same(first, Q.oracle_answers(sc, rs), "between frames")
    finally:
        rsc.close()


def test_every_instance_kind_answers_alike(axis_scene, axis_sets, gpu_count):
    sc, rs = axis_scene, axis_sets
    want = Q.oracle_answers(sc, rs)
    base = R.ResidentScene(sc)
    made = [base]
    try:
        made.append(R.ResidentScene(sc, tiles=[1], like=base))  # a peer with a partial tile set
        passes = R.ResidentScene(sc)
        made.append(passes)
        passes.set_passes(alpha=True, depth=True, triangle=True)
        passes.render()
        mega = R.ResidentScene(sc)
        made.append(mega)
        mega.set_pipeline(R.PIPELINE_MEGAKERNEL)
        if gpu_count > 1:
            made.append(R.ResidentScene(sc, device=1, like=base))
        for i, m in enumerate(made):
            assert_same(query(m, rs), want, f"instance {i} (device {m.device})")
        passes.readback_passes()
    finally:
        for m in made:
            m.close()


def test_device_entry_refuses_host_memory(axis_scene, hip_lib):
    rsc = R.ResidentScene(axis_scene)
    try:
        rays = np.zeros((256, 8), np.float32)
        hits = np.zeros((256, 4), np.float32)
        rc = hip_lib.rtHipSceneIntersectDevice(C.c_void_p(rsc.handle), R._ptr(rays), None, 256, R._ptr(hits), None)
        assert rc == -1 and "device memory" in R.last_error()
        dev_rays = hip_lib.rtHipDeviceAlloc(0, 256 * 32)
        try:
            rc = hip_lib.rtHipSceneIntersectDevice(C.c_void_p(rsc.handle), C.c_void_p(dev_rays), None, 256, R._ptr(hits), None)
            assert rc == -1 and "hits" in R.last_error()
            rc = hip_lib.rtHipSceneIntersectDevice(C.c_void_p(rsc.handle), C.c_void_p(dev_rays), None, 257, C.c_void_p(dev_rays), None)
            assert rc == -1  # 257 rays reach past the 256-ray allocation
            assert hip_lib.rtHipSceneIntersectDevice(C.c_void_p(rsc.handle), None, None, 0, None, None) == 0
        finally:
            hip_lib.rtHipDeviceFree(0, C.c_void_p(dev_rays))
    finally:
        rsc.close()


def test_material_mesh_and_position_on_a_mesh_scene(axis_scene):
    sc = axis_scene
    assert sc.tri_mesh is not None
    rs = Q.segments(sc, 2000, seed=21)
    rsc = R.ResidentScene(sc)
    try:
        got = query(rsc, rs)
    finally:
        rsc.close()
    hit = got["triangle"] != Q.NONE
    assert hit.any() and (~hit).any(), f"{hit.sum()} hits of {hit.size}: the miss checks below need both"
    idx = got["triangle"][hit].astype(np.int64)
    assert np.array_equal(got["material"][hit], np.asarray(sc.tri_material, np.int32)[idx])
    assert np.array_equal(got["mesh"][hit], np.asarray(sc.tri_mesh, np.int32)[idx])
    assert (got["material"][~hit] == -1).all() and (got["mesh"][~hit] == -1).all()
    pos = rs["o"] + got["t"][:, None] * rs["d"]
    assert np.array_equal(Q.bits(got["position"]), Q.bits(pos.astype(np.float32)))
    assert (got["ab"][~hit] == 0).all() and (got["ac"][~hit] == 0).all()
    assert np.array_equal(Q.bits(got["t"][~hit]), Q.bits(rs["tmax"][~hit]))
