"""Seeded ray sets for the ray queries (rtHipSceneIntersect, ResidentScene.intersect) on a Scene, and their expected answers from the C
restatement of the reference's grid walk (rt_oracle_grid_trace) and from the reference's own RayIntersectsTriangles.

A ray set is a dict of numpy arrays: o, d [N, 3] f32, tmin, tmax [N] f32, excluded [N] u32 (0xffffffff = none).  An answer is a dict
triangle [N] u32, t, ab, ac [N] f32 (ab = ac = 0 on a miss, t = tmax)."""
import ctypes as C

import numpy as np

import oracle_lib as O

NONE = 0xFFFFFFFF
F32 = np.float32


def _set(o, d, tmin, tmax, excluded):
    n = len(o)
    return dict(o=np.ascontiguousarray(o, F32).reshape(n, 3), d=np.ascontiguousarray(d, F32).reshape(n, 3),
                tmin=np.ascontiguousarray(np.broadcast_to(np.asarray(tmin, F32), (n,))),
                tmax=np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, F32), (n,))),
                excluded=np.ascontiguousarray(np.broadcast_to(np.asarray(excluded, np.uint32), (n,))))


def concat(*sets):
    return {k: np.concatenate([s[k] for s in sets]) for k in sets[0]}


def take(rs, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in rs.items()}


def _box(sc):
    b = np.asarray(sc.box_min, F32)
    return b[0, :3].astype(np.float64), b[256, :3].astype(np.float64)


def _tri_points(sc, tris, rng):
    """A point inside each triangle (float32), from random barycentrics."""
    v = np.asarray(sc.vertex, F32)[:, :3]
    ix = np.asarray(sc.tri_index, np.int64)[tris, :3]
    u = rng.random((len(tris), 2))
    flip = u.sum(1) > 1
    u[flip] = 1 - u[flip]
    a, b, c = (v[ix[:, k]].astype(np.float64) for k in range(3))
    return (a + u[:, :1] * (b - a) + u[:, 1:] * (c - a)).astype(F32)


def camera_rays(sc, n=None, seed=0):
    """The eye through pixel centres: d = topLeft + lr * (x + 0.5) + tb * (y + 0.5) in float32; every pixel, or n of them at random."""
    W, H = sc.width, sc.height
    p = np.arange(W * H) if n is None or n >= W * H else np.random.default_rng(seed).choice(W * H, n, replace=False)
    x, y = (p % W).astype(F32) + F32(0.5), (p // W).astype(F32) + F32(0.5)
    tl, lr, tb = (np.asarray(v, F32)[:3] for v in (sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom))
    d = tl[None, :] + lr[None, :] * x[:, None]
    d = d + tb[None, :] * y[:, None]
    o = np.broadcast_to(np.asarray(sc.eye, F32)[:3], d.shape)
    return _set(o, d, 0.0, np.inf, NONE)


def random_rays(sc, n, seed=0):
    """Origins uniform in the grid's box grown by half its size on every side (inside and outside it), directions uniform on the sphere
    with lengths from 2^-8 to 2^8; a quarter with a finite tmax, a quarter with tmin > 0."""
    rng = np.random.default_rng(seed)
    lo, hi = _box(sc)
    ext = hi - lo
    o = lo - 0.5 * ext + rng.random((n, 3)) * 2 * ext
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.exp2(rng.uniform(-8, 8, (n, 1)))
    tmax = np.where(rng.random(n) < 0.25, rng.uniform(0, 2, n) * np.linalg.norm(ext) / np.linalg.norm(d, axis=1), np.inf)
    tmin = np.where(rng.random(n) < 0.25, rng.uniform(0, 0.5, n) * np.linalg.norm(ext) / np.linalg.norm(d, axis=1), 0.0)
    return _set(o, d, tmin, tmax, NONE)


def segments(sc, n, seed=0):
    """Finite segments between points on two triangles, tmax = 1, the source triangle excluded (what a shadow ray is)."""
    rng = np.random.default_rng(seed)
    T = sc.triangle_count
    src, dst = rng.integers(0, T, n), rng.integers(0, T, n)
    a, b = _tri_points(sc, src, rng), _tri_points(sc, dst, rng)
    tmin = np.where(rng.random(n) < 0.5, 0.0, 1e-4)
    return _set(a, (b - a).astype(F32), tmin, 1.0, src.astype(np.uint32))


def axis_edges(sc, n, seed=0):
    """Directions with +0 / -0 and subnormal components and untame magnitudes (2^-60 .. 2^60), origins exactly on split planes, rays
    that run along a plane (origin on it, that axis' component +-0)."""
    rng = np.random.default_rng(seed)
    planes = np.asarray(sc.box_min, F32)[:, :3]
    lo, hi = _box(sc)
    o = (lo + rng.random((n, 3)) * (hi - lo)).astype(F32)
    d = rng.normal(size=(n, 3)).astype(F32)
    specials = np.array([0.0, -0.0, 1e-40, -1e-40, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -41, 2.0 ** 41, 1e-30, -1e30], F32)
    for k in range(3):
        pick = rng.random(n) < 0.4
        d[pick, k] = rng.choice(specials, pick.sum())
        on = rng.random(n) < 0.5
        o[on, k] = planes[rng.integers(0, 257, on.sum()), k]
    along = rng.random(n) < 0.25  # run along the plane the origin lies on
    ax = rng.integers(0, 3, n)
    d[along, ax[along]] = np.where(rng.random(along.sum()) < 0.5, F32(0.0), F32(-0.0))
    scale = np.exp2(rng.uniform(-60, 60, (n, 1))).astype(F32)
    d = np.where(rng.random((n, 1)) < 0.3, d * scale, d)
    tmax = np.where(rng.random(n) < 0.3, F32(rng.uniform(0, 4)), np.inf)
    return _set(o, d, 0.0, tmax, NONE)


def hostile(sc, n, seed=0):
    """NaN or +-inf in any field, tmin > tmax, tmin < 0, o + tmin*d overflowing, d = 0, excluded ids >= T (quiet NaNs only: the
    oracle's arguments go through ctypes doubles)."""
    rng = np.random.default_rng(seed)
    base = random_rays(sc, n, seed + 1)
    o, d, tmin, tmax, ex = (base[k].copy() for k in ("o", "d", "tmin", "tmax", "excluded"))
    bad = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 3e38, -3e38, 1e-45], F32)
    kind = rng.integers(0, 8, n)
    for i in range(n):
        k = kind[i]
        if k == 0:
            o[i, rng.integers(0, 3)] = rng.choice(bad)
        elif k == 1:
            d[i, rng.integers(0, 3)] = rng.choice(bad)
        elif k == 2:
            tmin[i], tmax[i] = rng.choice(bad), rng.choice(bad)
        elif k == 3:
            tmin[i], tmax[i] = F32(5.0), F32(1.0)  # tmin > tmax
        elif k == 4:
            tmin[i] = F32(-rng.uniform(0, 10))
        elif k == 5:
            tmin[i], d[i] = F32(3e38), d[i] * F32(1e10)  # o + tmin*d overflows
        elif k == 6:
            d[i] = 0.0
        else:
            ex[i] = rng.choice([sc.triangle_count, sc.triangle_count + 1, 0x7FFFFFFF, 0xFFFFFFFE])
    return _set(o, d, tmin, tmax, ex)


def all_sets(sc, n=2000, seed=0):
    """Every kind of ray set, n rays each (camera rays: up to n pixel centres)."""
    return dict(camera=camera_rays(sc, n, seed), random=random_rays(sc, n, seed), segments=segments(sc, n, seed),
                axis=axis_edges(sc, n, seed), hostile=hostile(sc, n, seed))


def oracle_answers(sc, rs):
    """rt_oracle_grid_trace on every ray (abL = acL = 0 where it leaves them unwritten)."""
    L = O.oracle()
    dummy = [np.zeros(1, np.uint16) for _ in range(3)]
    osc = O.oracle_scene(sc, dummy)
    n = len(rs["o"])
    out = dict(triangle=np.empty(n, np.uint32), t=np.empty(n, F32), ab=np.empty(n, F32), ac=np.empty(n, F32))
    fp = C.POINTER(C.c_float)
    o, d = rs["o"], rs["d"]
    ob, db = o.ctypes.data, d.ctypes.data
    t, ab, ac = C.c_float(), C.c_float(), C.c_float()
    fn, ref = L.rt_oracle_grid_trace, C.byref(osc)
    tmin, tmax, ex = rs["tmin"].tolist(), rs["tmax"].tolist(), rs["excluded"].tolist()
    for i in range(n):
        ab.value = 0.0
        ac.value = 0.0
        out["triangle"][i] = fn(ref, C.cast(ob + 12 * i, fp), C.cast(db + 12 * i, fp), tmin[i], tmax[i], ex[i], C.byref(t), C.byref(ab), C.byref(ac))
        out["t"][i], out["ab"][i], out["ac"][i] = t.value, ab.value, ac.value
    return out


# The reference passes float3 (cl_float4: a 16-byte aligned union) by value, and its 9th and 10th vector arguments go on the stack in 16-byte
# aligned slots, which ctypes cannot lay out.  So a few lines of C that take pointers make the call; they are compiled next to the test's
# temporary files and link the reference's library.
_SHIM = r"""
typedef union { float s[4]; float v __attribute__((vector_size(16))); } f3;
unsigned RayIntersectsTriangles(f3, f3, float, float, unsigned, void *, void *, void *, void *, void *, void *, void *, void *, f3, f3, float,
                                int, void *, void *, void *, float *, float *, float *);
void ref_grid_walk(unsigned n, const float *o, const float *d, const float *tmin, const float *tmax, const unsigned *ex, void *triIndex,
                   void *vertex, const float *tb, const float *lr, float pixelSizeInv, void *boxMin, void *gridStart, void *gridList,
                   unsigned *tri, float *t, float *ab, float *ac)
{
    f3 T = { { tb[0], tb[1], tb[2], 0.f } }, L = { { lr[0], lr[1], lr[2], 0.f } };
    for (unsigned i = 0; i < n; ++i) {
        f3 O = { { o[3 * i], o[3 * i + 1], o[3 * i + 2], 0.f } }, D = { { d[3 * i], d[3 * i + 1], d[3 * i + 2], 0.f } };
        ab[i] = 0.f; ac[i] = 0.f;
        tri[i] = RayIntersectsTriangles(O, D, tmin[i], tmax[i], ex[i], triIndex, 0, 0, 0, vertex, 0, 0, 0, T, L, pixelSizeInv, 256, boxMin,
                                        gridStart, gridList, &t[i], &ab[i], &ac[i]);
    }
}
"""
_shim = None


def _ref_shim(workdir):
    global _shim
    if _shim is None:
        import os
        import subprocess
        src, so = os.path.join(workdir, "ref_walk_shim.c"), os.path.join(workdir, "ref_walk_shim.so")
        open(src, "w").write(_SHIM)
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src, O.REF_SO, "-Wl,-rpath," + os.path.dirname(O.REF_SO)],
                       check=True)
        O.ref()  # (loaded first, globally visible to the shim's reference)
        _shim = C.CDLL(so)
        _shim.ref_grid_walk.argtypes = [C.c_uint32] + [C.c_void_p] * 9 + [C.c_float] + [C.c_void_p] * 7
        _shim.ref_grid_walk.restype = None
    return _shim


def reference_answers(sc, rs, workdir):
    """The reference's own RayIntersectsTriangles (raytrace_opencl.c:324-401, oracle/_ref/libref_kernel.so) on every ray; the shim is
    built in `workdir`."""
    n = len(rs["o"])
    out = dict(triangle=np.empty(n, np.uint32), t=np.empty(n, F32), ab=np.empty(n, F32), ac=np.empty(n, F32))
    p = O._ptr
    tb, lr = (np.ascontiguousarray(np.asarray(v, F32)[:3]) for v in (sc.top_to_bottom, sc.left_to_right))
    _ref_shim(workdir).ref_grid_walk(n, p(rs["o"]), p(rs["d"]), p(rs["tmin"]), p(rs["tmax"]), p(rs["excluded"]), p(sc.tri_index), p(sc.vertex),
                                     p(tb), p(lr), float(sc.pixel_size_inv), p(sc.box_min), p(sc.grid_start), p(sc.grid_list),
                                     p(out["triangle"]), p(out["t"]), p(out["ab"]), p(out["ac"]))
    return out


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def mismatches(got, want, hits_only=False):
    """Indices where two answers differ: triangle, and the bits of t, ab, ac (on hits only, or everywhere)."""
    bad = got["triangle"] != want["triangle"]
    hit = want["triangle"] != NONE
    for k in ("t", "ab", "ac"):
        diff = bits(got[k]) != bits(want[k])
        bad |= (diff & hit) if hits_only else diff
    return np.flatnonzero(bad)
