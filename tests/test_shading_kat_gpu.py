"""The shading building blocks ON THE DEVICE (run with -m gpu), against the answers minted from the reference's own functions
(tests/golden/kat_shading.npz): the texel look-up on every route of texel_rec / texel, the shading normal in all three
instantiations the kernels use (with and without the round-0 row's firstVertex), both run through rtHipTestShadeKat on resident
scenes -- so the records the upload built (triangle records, shading rows, material descriptors, atlas, bump tables) are what is
tested -- and the wavefront kernels' split sphere draw and the u16 accumulation through rtHipDeviceKat."""
import ctypes as C
import os

import numpy as np
import pytest

import scenarios
import shading_kat as K
from conftest import GOLDEN
from opencl_render_amd import raytrace as R

pytestmark = pytest.mark.gpu

TEXEL, NORMAL = 0, 1
SPHERE, SPHERE_SPLIT, ACCUM = 1, 9, 10


@pytest.fixture(scope="module")
def kat(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the device KATs cannot run (there is no CPU stand-in)")
    return K.fixture()


def run(op, inp, out_stride):
    inp = np.ascontiguousarray(inp)
    n = inp.shape[0]
    out = np.zeros((n, out_stride), np.uint8)
    rc = R.lib().rtHipDeviceKat(0, op, n, inp.ctypes.data_as(C.c_void_p), inp.nbytes // n, out.ctypes.data_as(C.c_void_p), out_stride, None)
    assert rc == 0, f"rtHipDeviceKat(op={op}) returned {rc}"
    return out


def resident(sc):
    R.build_lists(sc)
    return R.ResidentScene(sc, 0)


def test_texel_every_route(kat):
    sc = scenarios.shade_texel_scene()
    rs = resident(sc)
    try:
        q, want = kat["texel_q"], kat["texel_ans"]
        out = rs.shade_kat(TEXEL, q).view(np.float32)
        words = out.view(np.uint32)
        desc = words[:, 12]
        m = q.view(np.int32)[:, 0]
        one = np.array([scenarios.TEXEL_TABLES[i] == (1, 1) for i in m])
        assert np.array_equal(desc >> 31, one.astype(np.uint32)), "a one-texel table must be held in its descriptor, an image not"
        assert (desc != 0).all()
        for name, cols in (("texel_rec", slice(0, 3)), ("texel<false>", slice(4, 7)), ("texel<true>", slice(8, 11))):
            bad = K.same(out[:, cols], want)
            assert bad.size == 0, f"{name}: {bad.size} of {len(q)} look-ups differ, first {q[bad[0]]}: {out[bad[0], cols]} vs {want[bad[0]]}"
            raw = words[:, cols.stop]
            assert (raw < 256).all() and np.array_equal((raw.astype(np.float32) / np.float32(255)).astype(np.float32), want[:, 0]), name
        assert (words[:, 13] == 1).all(), "the counted look-up must count one texel fetch"
    finally:
        rs.close()


@pytest.mark.parametrize("zoom", K.ZOOMS)
def test_shading_normal_every_instantiation(kat, zoom):
    sc = scenarios.shade_normal_scene(zoom)
    rs = resident(sc)
    try:
        q, want = kat[f"normal_q_{zoom}"], kat[f"normal_ans_{zoom}"]
        out = rs.shade_kat(NORMAL, q).view(np.float32).reshape(len(q), 6, 4)
        ran = out.view(np.uint32)[:, :, 3]
        tri = q.view(np.uint32)[:, 0]
        m = sc.tri_material[tri]
        image = np.array([k >= 0 and isinstance(scenarios.NORMAL_BUMPS[k], tuple) and len(scenarios.NORMAL_BUMPS[k]) == 2 for k in m])
        assert (ran[:, :4] == 1).all()
        assert np.array_equal(ran[:, 4] == 1, ~image) and np.array_equal(ran[:, 5] == 1, ~image)
        names = ["<false> (MatRec)", "<false> (MatRec, firstVertex)", "<true> (megakernel)", "<true> (megakernel, firstVertex)",
                 "<false, true> (class)", "<false, true> (class, firstVertex)"]
        for f, name in enumerate(names):
            rows = np.flatnonzero(ran[:, f] == 1)
            assert rows.size >= (len(q) // 2 if f >= 4 else len(q)), name
            bad = K.same(out[rows, f, :3], want[rows])
            assert bad.size == 0, (f"shading_normal{name}: {bad.size} of {rows.size} normals differ, first query {q[rows[bad[0]]]}: "
                                   f"{out[rows[bad[0]], f, :3]} vs {want[rows[bad[0]]]}")
    finally:
        rs.close()


def _sphere_inputs(seeds, radius):
    inp = np.zeros((len(seeds), 16), np.uint8)
    inp[:, :8] = np.asarray(seeds, np.uint64).reshape(-1, 1).view(np.uint8)
    inp[:, 8:12] = np.asarray(radius, np.float32).reshape(-1, 1).view(np.uint8)
    return inp


def test_split_sphere_draw(kat):
    old = np.load(os.path.join(GOLDEN, "kat.npz"))
    for seeds, radius, pts, states in ((old["sphere_seeds"], old["sphere_radius"], old["sphere_out"], old["sphere_state"]),
                                       (kat["sphere_seeds"], kat["sphere_radius"], kat["sphere_out"], kat["sphere_state"])):
        for op in (SPHERE_SPLIT, SPHERE):
            out = run(op, _sphere_inputs(seeds, radius), 24)
            got = out[:, :12].copy().view(np.float32)
            bad = np.flatnonzero(got.view(np.uint32) != pts.view(np.uint32))
            assert bad.size == 0, f"op {op}: {bad.size // 3} draws differ, first seed {seeds[bad[0] // 3]} radius {radius[bad[0] // 3]!r}"
            assert np.array_equal(out[:, 16:24].copy().view(np.uint64).reshape(-1), states)


def _trunc_x86(v):
    v = np.asarray(v, np.float32)
    ok = (v > np.float32(-2147483904.0)) & (v < np.float32(2147483648.0))
    out = np.full(v.shape, -(2 ** 31), np.int64)
    out[ok] = np.trunc(v[ok]).astype(np.int64)
    return out


def test_accumulation_saturates_like_cvttss2si():
    """sat_add_u16 / trunc_x86 (raytrace_opencl.c:726-741 as the x86 binary computes it: cvttss2si gives INT_MIN for NaN and out of
    range) against a numpy restatement.  The plane is 0 where plane + the truncated value would overflow an int (undefined in C)."""
    rng = np.random.default_rng(55)
    special = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, -1e-30, 1.0, 0.99999994, 1.0000001, 65535.0, 65534.996, 65535.5, 65536.0,
                        2147483520.0, 2147483648.0, 2147483904.0, -2147483648.0, -2147483904.0, -2147483648.0 - 256, -2147483520.0, 3e38, -3e38],
                       np.float32)
    scales = np.array([np.float32(65535) / np.float32(s) for s in (1, 2, 3, 7, 100, 1000)] + [1.0], np.float32)
    colour = np.concatenate([special, rng.uniform(-0.5, 1.5, 4000).astype(np.float32), rng.uniform(0, 1, 500).astype(np.float32) * np.float32(1e6),
                             np.float32(1) / np.arange(1, 400, dtype=np.float32)])
    c, s = np.meshgrid(colour, scales, indexing="ij")
    c, s = c.reshape(-1).astype(np.float32), s.reshape(-1).astype(np.float32)
    # special colours are also taken as the product itself (scale 1): values around +-2^31 and 65535 reach the conversion as they are
    plane = rng.integers(0, 65536, c.size).astype(np.int64)
    plane[::7] = rng.choice([0, 1, 65534, 65535], c[::7].size)
    with np.errstate(all="ignore"):
        prod = (c * s).astype(np.float32)
    t = _trunc_x86(prod)
    plane[np.abs(t) > 2 ** 31 - 2 ** 17] = 0
    inp = np.zeros((c.size, 3), np.float32)
    inp.view(np.int32)[:, 0] = plane
    inp[:, 1], inp[:, 2] = c, s
    out = run(ACCUM, inp, 8).view(np.int32)
    assert np.array_equal(out[:, 1], t), "trunc_x86 is not cvttss2si"
    want = np.clip(plane + t, 0, 65535)
    bad = np.flatnonzero(out[:, 0] != want)
    assert bad.size == 0, f"{bad.size} sums differ, first plane {plane[bad[0]]} colour {c[bad[0]]!r} scale {s[bad[0]]!r}: {out[bad[0], 0]} vs {want[bad[0]]}"
    assert (t == -(2 ** 31)).sum() >= 3 * len(scales) and ((prod > 65535) & (t < 2 ** 31 - 1)).any() and (want == 65535).any() and (want == 0).any()
