"""CPU tests of the shading known answers (tests/golden/kat_shading.npz, minted by make_golden.py shading from the reference's own
Get2dTableValue3, GetTriangleNormal and GetSpherePoint): the restatement must give every answer bit for bit, the queries must still
be what the generators draw, and they must still cover the edges.  Where oracle/_ref exists the reference itself must still give
the stored answers.  The same answers are checked on the device by tests/test_shading_kat_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import scenarios
import shading_kat as K


@pytest.fixture(scope="module")
def kat():
    return K.fixture()


@pytest.fixture(scope="module")
def mg():
    return K.make_golden()


def _fp(a):
    return np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))


def test_queries_are_what_the_generators_draw(kat, mg):
    q = mg.shading_queries()
    for k in ("texel_q", "normal_q_1", "normal_q_50", "sphere_seeds", "sphere_radius"):
        assert q[k].tobytes() == kat[k].tobytes(), f"{k}: the generator no longer draws the stored queries (re-mint kat_shading.npz)"


def test_texel_queries_cover_the_edges(kat):
    q = kat["texel_q"]
    m = q.view(np.int32)[:, 0]
    assert np.array_equal(np.bincount(m, minlength=len(scenarios.TEXEL_TABLES)) >= K.MIN_TEXEL_PER_TABLE, np.ones(len(scenarios.TEXEL_TABLES), bool))
    L = O.oracle()
    for axis in (0, 1):
        s = q[:, 2 + axis] + (q[:, 4 + axis] - q[:, 2 + axis]) * q[:, 8] + (q[:, 6 + axis] - q[:, 2 + axis]) * q[:, 9]
        p = np.array([L.rt_oracle_positive_modf(float(x)) for x in s], np.float32)
        assert (p == 1.0).sum() >= K.MIN_TEXEL_ONE, f"axis {axis}: {(p == 1.0).sum()} queries land on the last column / row"
        assert np.isfinite(s).all()  # NaN / inf uvs are left out (make_golden.shading_queries)
    uv = q[:, 2:8]
    for v in (0.0, 1.0, 2.0 ** 23, 2.0 ** 24, -(2.0 ** -30)):
        assert (uv == np.float32(v)).any(), v
    assert (np.signbit(uv) & (uv == 0)).any()  # -0.0
    assert (np.abs(q[:, 8:10]) == np.float32(1e6)).any() and (q[:, 8:10] < 0).any()
    sc = scenarios.shade_texel_scene()
    assert int(sc.mat_start[5 * (len(scenarios.TEXEL_TABLES) - 1) + 4]) > 2 ** 24  # the last table starts above 2^24 texels


@pytest.mark.parametrize("zoom", K.ZOOMS)
def test_normal_queries_cover_the_edges(kat, mg, zoom):
    sc = scenarios.shade_normal_scene(zoom)
    k = mg.normal_kinds(sc, kat[f"normal_q_{zoom}"])
    assert k["tb_miss"].sum() >= K.MIN_PROBE_MISS and k["lr_miss"].sum() >= K.MIN_PROBE_MISS
    assert (k["tb_miss"] & ~k["lr_miss"]).any() and (~k["tb_miss"] & k["lr_miss"]).any()
    assert (k["tb_miss"] & k["lr_miss"] & k["image_bump"]).sum() >= 50
    assert k["vertex"].sum() >= K.MIN_VERTEX and k["edge"].sum() >= K.MIN_EDGE
    assert k["degenerate"].sum() >= K.MIN_DEGENERATE
    counts = np.bincount(k["material"] + 1, minlength=len(scenarios.NORMAL_BUMPS) + 1)
    assert (counts >= K.MIN_PER_MATERIAL).all(), counts
    nrm = sc.tri_normal.reshape(-1, 3, 4)[:, :, :3]
    ln = np.sqrt((nrm.astype(np.float64) ** 2).sum(2))
    tri = kat[f"normal_q_{zoom}"].view(np.uint32)[:, 0]
    assert (np.abs(ln[tri] - 1) > 0.1).any(axis=1).sum() >= 100  # non-unit vertex normals
    assert (np.all(nrm[tri, 0] == nrm[tri, 1], axis=1) & np.all(nrm[tri, 0] == nrm[tri, 2], axis=1)).sum() >= 100  # flat


def test_cameras_differ(kat):
    a, b = scenarios.shade_normal_scene(1), scenarios.shade_normal_scene(50)
    assert b.pixel_size_inv / a.pixel_size_inv == 50
    for s in (a, b):  # not powers of two: x / pixelSizeInv and x * (1 / pixelSizeInv) round differently
        assert np.frexp(np.float32(s.pixel_size_inv))[0] != 0.5


def test_oracle_texel_matches_reference(kat):
    sc = scenarios.shade_texel_scene()
    L = O.oracle()
    q, want = kat["texel_q"], kat["texel_ans"]
    got = np.zeros_like(want)
    for j, row in enumerate(q):
        m, ch = (int(x) for x in row.view(np.int32)[:2])
        table = sc.textures[int(sc.mat_start[5 * m + ch]):]
        w, h = (int(x) for x in sc.mat_size[5 * m + ch])
        out = np.zeros(3, np.float32)
        L.rt_oracle_texel(table.ctypes.data_as(C.c_void_p), w, h, _fp(row[2:8]), float(row[8]), float(row[9]), out.ctypes.data_as(C.POINTER(C.c_float)))
        got[j] = out
    bad = K.same(got, want)
    assert bad.size == 0, f"{bad.size} texel answers differ, first query {q[bad[0]]}"
    if O.have_ref():
        live = np.zeros_like(want)
        for j, row in enumerate(q):
            m, ch = (int(x) for x in row.view(np.int32)[:2])
            w, h = (int(x) for x in sc.mat_size[5 * m + ch])
            live[j] = O.ref_texel(sc.textures[int(sc.mat_start[5 * m + ch]):], w, h, row[2:8], row[8], row[9])
        assert live.tobytes() == want.tobytes(), "the reference no longer gives the stored texel answers"


@pytest.mark.parametrize("zoom", K.ZOOMS)
def test_oracle_shading_normal_matches_reference(kat, zoom):
    from opencl_render_amd import raytrace as R
    sc = scenarios.shade_normal_scene(zoom)
    R.build_lists(sc)
    planes = [np.zeros(sc.pixels, np.uint16) for _ in range(3)]
    osc = O.oracle_scene(sc, planes)
    L = O.oracle()
    L.rt_oracle_shading_normal.argtypes = [C.POINTER(O.OracleScene)] + [C.POINTER(C.c_float)] * 3 + [C.c_uint32, C.c_float, C.c_float, C.POINTER(C.c_float)]
    q, want = kat[f"normal_q_{zoom}"], kat[f"normal_ans_{zoom}"]
    got = np.zeros_like(want)
    for j, row in enumerate(q):
        out = np.zeros(3, np.float32)
        L.rt_oracle_shading_normal(C.byref(osc), _fp(row[1:4]), _fp(row[4:7]), _fp(row[7:10]), int(row.view(np.uint32)[0]), float(row[10]),
                                   float(row[11]), out.ctypes.data_as(C.POINTER(C.c_float)))
        got[j] = out
    bad = K.same(got, want)
    assert bad.size == 0, f"{bad.size} normals differ, first query {q[bad[0]]}: {got[bad[0]]} vs {want[bad[0]]}"
    if O.have_ref_zeroed():  # (a library built from an older ref_glue.c has no ref_triangle_normal: the stored answers stand in)
        live = np.stack([O.ref_triangle_normal_zeroed(sc, row[1:4], row[4:7], row[7:10], row.view(np.uint32)[0], row[10], row[11]) for row in q])
        assert live.tobytes() == want.tobytes(), "the reference no longer gives the stored normals"


def test_oracle_sphere_point_at_spread_radii(kat):
    L = O.oracle()
    for j in range(len(kat["sphere_seeds"])):
        st = C.c_uint64(int(kat["sphere_seeds"][j]))
        out = np.zeros(3, np.float32)
        L.rt_oracle_sphere_point(C.byref(st), float(kat["sphere_radius"][j]), out.ctypes.data_as(C.POINTER(C.c_float)))
        assert out.tobytes() == kat["sphere_out"][j].tobytes(), j
        assert st.value == int(kat["sphere_state"][j])
    r = set(kat["sphere_radius"].tolist())
    assert 0.0 in r and 1.0 in r and len(r) >= 8
