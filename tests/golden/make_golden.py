#!/usr/bin/env python3
"""Mints the golden fixtures under tests/golden/ from the REFERENCE's own kernel.

Run in the build container only (it needs oracle/_ref/libref_kernel.so, i.e. /root/reference):

    make -C oracle && python tests/golden/make_golden.py

Provenance of every number written here: oracle/_ref/libref_kernel.so is /root/reference/source/opencl/
raytrace_opencl.c compiled in place by oracle/Makefile (plus the 3 OpenCL built-ins and the pixel/sample loop in
oracle/ref_glue.c); the reference ships no golden vectors of its own.  Fixtures are data only:
scene inputs in the ABI layouts and the expected u16 planes / function results.

  scene_<name>.npz   inputs (grid start stored sparsely as non-empty cell ids + counts) and planes R,G,B
  kat.npz            function-level known answers (randF, GetSpherePoint, positive_modf, RayIntersectsTriangle,
                     GetPointToLineSqLen, GetBoxAddress, BindInCube)
  ref_fresh_scenes.npz  planes R,G,B ("<seed>_r", "_g", "_b") of scenarios.fresh_soup(seed) for scenarios.FRESH_SEEDS
                     (inputs not stored: the test regenerates them from the seed)
  ref_class_scenes.npz  planes R,G,B ("<name>_r", "_g", "_b") of every opaque-diffuse scenario in scenarios.CLASS (inputs not
                     stored: the tests regenerate them from the code and R.build_lists); written byte for byte the same on every run
  ref_axis_scenes.npz   planes R,G,B ("<name>_r", "_g", "_b") of every grid-walk edge scenario in scenarios.AXIS (inputs not stored,
                     as for ref_class_scenes.npz); written byte for byte the same on every run
  kat_shading.npz    known answers of Get2dTableValue3 on scenarios.shade_texel_scene's tables, of GetTriangleNormal on
                     scenarios.shade_normal_scene(1) and (50), and of GetSpherePoint at radius 0, 1 and the host's light spreads
                     (shading_queries builds the queries); written byte for byte the same on every run
"""
import ctypes as C
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib as O  # noqa: E402
import scenarios  # noqa: E402
from opencl_render_amd import raytrace as R  # noqa: E402

SCENE_FIELDS = ["eye", "eye_to_top_left", "left_to_right", "top_to_bottom", "vertex", "tri_index", "tri_material", "tri_uv",
                "tri_normal", "mat_size", "mat_start", "textures", "light_type", "light_pos", "light_dir", "light_col",
                "light_radius", "light_half_att", "cam_start", "cam_end", "cam_list", "box_min", "grid_list"]


def save_scene(sc, planes, path):
    counts = np.diff(sc.grid_start.astype(np.int64))
    cells = np.nonzero(counts)[0].astype(np.uint32)
    data = {k: getattr(sc, k) for k in SCENE_FIELDS}
    data.update(grid_cells=cells, grid_counts=counts[cells].astype(np.uint32),
                dims=np.array([sc.width, sc.height, sc.sample_count], np.uint32),
                pixel_size_inv=np.float32(sc.pixel_size_inv), out_r=planes[0], out_g=planes[1], out_b=planes[2])
    np.savez_compressed(path, **data)


def f3(v):
    out = O.Float3()
    for i in range(3):
        out.s[i] = float(v[i])
    return out


def make_kat(path):
    ref = O.ref()
    rng = np.random.Generator(np.random.PCG64(2024))
    kat = {}
    # randF streams (raytrace_opencl.c:12-23)
    seeds = np.array([0, 1, 2, 12345, 2**32 - 1, 2**32, 2**63, 2**64 - 1, 987654321987654321], np.uint64)
    draws = np.zeros((len(seeds), 16), np.float32)
    states = np.zeros((len(seeds), 16), np.uint64)
    for i, s in enumerate(seeds):
        st = C.c_uint64(int(s))
        for j in range(16):
            lo, hi = ((0.0, 1.0), (-1.0, 1.0))[j & 1]
            draws[i, j] = ref.randF(C.byref(st), lo, hi)
            states[i, j] = st.value
    kat.update(rand_seeds=seeds, rand_draws=draws, rand_states=states)
    # GetSpherePoint (:30-45)
    sp_seeds = rng.integers(0, 2**63, 64).astype(np.uint64)
    sp_radius = rng.uniform(0.0, 3.0, 64).astype(np.float32)
    sp_out = np.zeros((64, 3), np.float32)
    sp_state = np.zeros(64, np.uint64)
    for i in range(64):
        st = C.c_uint64(int(sp_seeds[i]))
        p = ref.GetSpherePoint(C.byref(st), float(sp_radius[i]))
        sp_out[i] = p.s[0], p.s[1], p.s[2]
        sp_state[i] = st.value
    kat.update(sphere_seeds=sp_seeds, sphere_radius=sp_radius, sphere_out=sp_out, sphere_state=sp_state)
    # positive_modf (:25-28), including tiny negatives that round to 1.0f
    pm_in = np.concatenate([rng.uniform(-5, 5, 200), [-0.0, 0.0, 1.0, -1.0, -2.0 ** -30, 2.0 ** -30, -1e-8, 123456.75, -123456.75, 0.99999994]]).astype(np.float32)
    pm_out = np.array([ref.positive_modf(float(v)) for v in pm_in], np.float32)
    kat.update(pmodf_in=pm_in, pmodf_out=pm_out)
    # RayIntersectsTriangle (:124-172): random rays against random triangles, plus degenerate triangles
    n = 400
    ro = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    rd = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    ta = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    tb = ta + rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    tc = ta + rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    tb[::17] = ta[::17]           # zero-area
    rd[::23, 2] = 0               # axis-parallel rays
    tmin = np.where(np.arange(n) % 3 == 0, np.float32(0.2), np.float32(0)).astype(np.float32)
    tmax = np.where(np.arange(n) % 5 == 0, np.float32(1.5), np.float32(np.inf)).astype(np.float32)
    res = np.zeros((n, 4), np.float32)  # hit, t, abL, acL (abL/acL = 0 when not written)
    for i in range(n):
        t, l1, l2 = C.c_float(0), C.c_float(0), C.c_float(0)
        hit = ref.RayIntersectsTriangle(f3(ro[i]), f3(rd[i]), float(tmin[i]), float(tmax[i]), f3(ta[i]), f3(tb[i]), f3(tc[i]),
                                        C.byref(t), C.byref(l1), C.byref(l2))
        res[i] = hit, t.value, l1.value, l2.value
    kat.update(tri_o=ro, tri_d=rd, tri_a=ta, tri_b=tb, tri_c=tc, tri_tmin=tmin, tri_tmax=tmax, tri_res=res)
    # GetPointToLineSqLen (:83-101)
    pl = np.array([ref.GetPointToLineSqLen(f3(ta[i]), f3(tb[i]), f3(ro[i])) for i in range(n)], np.float32)
    kat.update(pline_out=pl)
    # GetBoxAddress (:174-193) and BindInCube (:265-322) on a real grid
    sc = scenarios.lambert_distant()
    R.build_scene_grid(sc)
    pts = np.concatenate([rng.uniform(-3, 3, (300, 3)) * [1, 1, 0] + [0, 0, 3], sc.box_min[[0, 1, 128, 255, 256], :3],
                          sc.vertex[:50, :3]]).astype(np.float32)
    addr = np.zeros((len(pts), 3), np.int32)
    for i, p in enumerate(pts):
        a = ref.GetBoxAddress(256, sc.box_min.ctypes.data_as(C.c_void_p), f3(p))
        addr[i] = a.s[0], a.s[1], a.s[2]
    kat.update(box_min=sc.box_min, box_pts=pts, box_addr=addr)
    bo = (rng.uniform(-4, 4, (300, 3)) + [0, 0, 3]).astype(np.float32)
    bd = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    bd[::13, 0] = 0
    bres = np.zeros((300, 4), np.float32)
    for i in range(300):
        p = f3(bo[i])
        ok = ref.BindInCube(C.byref(p), f3(bd[i]), f3(sc.box_min[0]), f3(sc.box_min[256]))
        bres[i] = ok, p.s[0], p.s[1], p.s[2]
    kat.update(bind_o=bo, bind_d=bd, bind_res=bres)
    # pow(0.5f, maxLen/halfAtt) cast to float (:631).  Not a reference symbol: the call goes to the C library, so the known
    # answers are THIS container's glibc pow -- the library the reference's C path calls here (parity-unpinned by
    # the reference itself).  x = the float quotient the kernel forms first.
    libm = C.CDLL("libm.so.6")
    libm.pow.restype = C.c_double
    libm.pow.argtypes = [C.c_double, C.c_double]
    px = np.concatenate([rng.uniform(0, 40, 600), rng.uniform(0, 1e-3, 100), [0.0, 1.0, 2.0, 126.0, 127.0, 149.0, 150.0, 200.0, np.inf]]).astype(np.float32)
    pw = np.array([libm.pow(0.5, float(v)) for v in px], np.float64).astype(np.float32)
    kat.update(pow_x=px, pow_out=pw)
    np.savez_compressed(path, **kat)


def make_fresh(path):
    planes = {}
    for seed in scenarios.FRESH_SEEDS:
        sc = scenarios.fresh_soup(seed)
        R.build_lists(sc)
        for c, p in zip("rgb", O.ref_render(sc)):
            planes[f"{seed}_{c}"] = p
    np.savez_compressed(path, **planes)


def save_npz_stable(path, arrays):
    """np.savez_compressed without the wall-clock time stamps: entries in key order, each dated 1980-01-01, so that the same
    planes give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            z.writestr(info, buf.getvalue())


def make_class(path):
    planes = {}
    for f in scenarios.CLASS:
        sc = f()
        R.build_lists(sc)
        if R.path_class(sc) != R.PATH_CLASS_OPAQUE_DIFFUSE:
            sys.exit(f"{f.__name__} is not in the opaque-diffuse class")
        for c, p in zip("rgb", O.ref_render(sc)):
            planes[f"{f.__name__}_{c}"] = p
    save_npz_stable(path, planes)


def make_axis(path):
    planes = {}
    for f in scenarios.AXIS:
        sc = f()  # (builds its lists and asserts its edge)
        for c, p in zip("rgb", O.ref_render(sc)):
            planes[f"{f.__name__}_{c}"] = p
    save_npz_stable(path, planes)


def shading_queries(answers=False):
    """The queries of kat_shading.npz, drawn from fixed seeds, and (given the reference) their answers.  Texel queries are rows
    (material, channel, uv[6], l1, l2); normal queries rows (triangle, where[3], ray o[3], ray d[3], l1, l2) per camera zoom.
    NaN and infinite uvs are left out: the reference's (int)floor(NaN) indexes outside its table (raytrace_opencl.c:114-117)."""
    rng = np.random.Generator(np.random.PCG64(777))
    out = {}
    # ---- texel look-ups, TEXEL_TABLES[i] is channel i % 5 of material i
    specials = np.array([0.0, 1.0, -0.0, -1.0, -0.5, -3.25, 2.0 ** 23, 2.0 ** 23 + 1, 2.0 ** 24, 3.0e7, -(2.0 ** 23), -(2.0 ** -30),
                         2.0 ** -30, 0.99999994, -2.0 ** -25, 7.5], np.float32)
    bary_pool = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0.5], [0.25, 0], [0, 0.75], [1e6, 0], [0, -1e6], [-1e6, 1e6], [1e6, 1e6], [-3.5, 2.0]],
                         np.float32)
    rows = []
    for i, (w, h) in enumerate(scenarios.TEXEL_TABLES):
        k = 400
        uv = rng.uniform(-5, 5, (k, 6)).astype(np.float32)
        pick = rng.random((k, 6)) < 0.5
        uv[pick] = rng.choice(specials, int(pick.sum()))
        bary = rng.uniform(0, 1, (k, 2)).astype(np.float32)
        inside = bary.sum(1) > 1
        bary[inside] = 1 - bary[inside]
        far = rng.random(k) < 0.4
        bary[far] = bary_pool[rng.integers(0, len(bary_pool), int(far.sum()))]
        edge = rng.random(k) < 0.15
        bary[edge, 1] = (1 - bary[edge, 0]).astype(np.float32)
        bary[:24] = bary_pool[np.arange(24) % len(bary_pool)]
        # uvs whose positive_modf rounds to 1.0f at the first corner: the last column / row
        uv[:12, 0] = np.float32(-(2.0 ** -30))
        uv[6:18, 1] = np.float32(-(2.0 ** -26))
        bary[:18] = 0
        r = np.zeros((k, 10), np.float32)
        r.view(np.int32)[:, 0] = i
        r.view(np.int32)[:, 1] = i % 5
        r[:, 2:8] = uv
        r[:, 8:10] = bary
        rows.append(r)
    tq = np.concatenate(rows)
    with np.errstate(all="ignore"):
        u = tq[:, 2] + (tq[:, 4] - tq[:, 2]) * tq[:, 8] + (tq[:, 6] - tq[:, 2]) * tq[:, 9]
        v = tq[:, 3] + (tq[:, 5] - tq[:, 3]) * tq[:, 8] + (tq[:, 7] - tq[:, 3]) * tq[:, 9]
    tq = tq[np.isfinite(u) & np.isfinite(v)]
    out["texel_q"] = tq
    # ---- shading normals, two cameras
    O_ = O.oracle()
    for zoom in (1, 50):
        sc = scenarios.shade_normal_scene(zoom)
        R.build_lists(sc)
        planes = [np.zeros(sc.pixels, np.uint16) for _ in range(3)]
        osc = O.oracle_scene(sc, planes)
        v = sc.vertex.reshape(-1, 3, 4)[:, :, :3]
        t = sc.triangle_count
        tb, lr = sc.top_to_bottom[:3], sc.left_to_right[:3]
        eye = sc.eye[:3].astype(np.float32)
        q = []

        def fp(a):
            return np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))

        def hit(o, d, tri):
            tt, l1, l2 = C.c_float(0), C.c_float(0), C.c_float(0)
            O_.rt_oracle_ray_triangle(fp(o), fp(d), 0.0, float("inf"), fp(v[tri, 0]), fp(v[tri, 1]), fp(v[tri, 2]), C.byref(tt), C.byref(l1), C.byref(l2))
            return np.float32(tt.value), np.float32(l1.value), np.float32(l2.value)

        def add(tri, where, o, d, l1, l2):
            row = np.zeros(12, np.float32)
            row.view(np.uint32)[0] = tri
            row[1:4], row[4:7], row[7:10], row[10], row[11] = where, o, d, l1, l2
            q.append(row)

        # camera rays through pixel centres and random sub-pixel points: the nearest hit (the oracle's grid walk)
        for _ in range(1400):
            x, y = np.float32(rng.uniform(0, sc.width)), np.float32(rng.uniform(0, sc.height))
            d = (sc.eye_to_top_left[:3] + x * lr + y * tb).astype(np.float32)
            tt, l1, l2 = C.c_float(0), C.c_float(0), C.c_float(0)
            tri = O_.rt_oracle_grid_trace(C.byref(osc), fp(eye), fp(d), 0.0, float("inf"), 0xFFFFFFFF, C.byref(tt), C.byref(l1), C.byref(l2))
            if tri == 0xFFFFFFFF:
                continue
            where = (eye + np.float32(tt.value) * d).astype(np.float32)
            add(tri, where, eye, d, l1.value, l2.value)
        # hits exactly on the vertices and on the edges, seen from the eye
        for tri in rng.choice(t, 120, replace=False):
            a, b, c = v[tri]
            for where, l1, l2 in ((a, 0, 0), (b, 1, 0), (c, 0, 1)):
                add(tri, where, eye, (where - eye).astype(np.float32), l1, l2)
            s_ = np.float32(rng.uniform(0, 1))
            for where, l1, l2 in (((a + s_ * (b - a)).astype(np.float32), s_, 0), ((a + s_ * (c - a)).astype(np.float32), 0, s_),
                                  ((b + s_ * (c - b)).astype(np.float32), 1 - s_, s_)):
                add(tri, where, eye, (where - eye).astype(np.float32), l1, l2)
        # grazing rays: one probe or both fall behind the plane or run parallel to it
        for _ in range(900):
            tri = int(rng.integers(0, t))
            a, b, c = v[tri]
            n = np.cross(c - a, b - a).astype(np.float32)
            ln = float(np.sqrt((n.astype(np.float64) ** 2).sum()))
            if ln == 0:
                continue
            n = n / np.float32(ln)
            l1, l2 = np.float32(rng.uniform(0, 0.5)), np.float32(rng.uniform(0, 0.5))
            where = (a + l1 * (b - a) + l2 * (c - a)).astype(np.float32)
            u = rng.normal(size=3).astype(np.float32)
            u = (u - np.float32(u @ n) * n).astype(np.float32)
            eps = np.float32(10.0 ** rng.uniform(-6, -1)) * np.linalg.norm(tb).astype(np.float32) * np.float32(rng.choice([-1, 1]))
            d = (u + eps * n).astype(np.float32)
            o = (where - d * np.float32(rng.uniform(0.5, 2))).astype(np.float32)
            add(tri, where, o, d, l1, l2)
        # rays parallel to the planar triangles (z = 3): tb and lr have no z, so both probes are parallel too
        planar = np.flatnonzero(np.all(v[:, :, 2] == np.float32(3.0), axis=1))
        for tri in planar:
            a, b, c = v[tri]
            for oz in (np.float32(3.0), np.float32(2.0), np.float32(0.0)):
                where = ((a + b + c) / np.float32(3)).astype(np.float32)
                o = np.array([0.1, -0.2, oz], np.float32)
                d = np.array([where[0] - o[0], where[1] - o[1], 0.0], np.float32)
                add(int(tri), where, o, d, np.float32(1 / 3), np.float32(1 / 3))
        nq = np.stack(q).astype(np.float32)
        out[f"normal_q_{zoom}"] = nq
    # ---- sphere draws at radius 0, 1 and the host's light spreads (rt_api.cpp: (float)(sin((r/2)*PI_F/180) * sqrt(|dir|^2)))
    libm = C.CDLL("libm.so.6")
    libm.sin.restype = libm.sqrt.restype = C.c_double
    libm.sin.argtypes = libm.sqrt.argtypes = [C.c_double]
    radii = [0.0, 1.0]
    for dvec in scenarios.SPREAD_DIRS:
        dd = np.float32(np.float32(dvec[0]) * np.float32(dvec[0]) + np.float32(dvec[1]) * np.float32(dvec[1])) + np.float32(dvec[2]) * np.float32(dvec[2])
        for r in scenarios.SPREAD_RADII:
            arg = np.float32(np.float32(np.float32(r) / np.float32(2)) * np.float32(3.14159265)) / np.float32(180)
            radii.append(float(np.float32(libm.sin(float(arg)) * libm.sqrt(float(np.float32(dd))))))
    radii = np.array(radii, np.float32)
    seeds = np.concatenate([rng.integers(0, 2 ** 63, 48).astype(np.uint64), np.array([0, 1, 2 ** 64 - 1], np.uint64)])
    out["sphere_seeds"] = np.repeat(seeds, len(radii))
    out["sphere_radius"] = np.tile(radii, len(seeds))
    if not answers:
        return out
    # ---- answers from the reference's own functions
    sc = scenarios.shade_texel_scene()
    ans = np.zeros((len(tq), 3), np.float32)
    for j, row in enumerate(tq):
        m, ch = int(row.view(np.int32)[0]), int(row.view(np.int32)[1])
        w, h = (int(x) for x in sc.mat_size[5 * m + ch])
        ans[j] = O.ref_texel(sc.textures[int(sc.mat_start[5 * m + ch]):], w, h, row[2:8], row[8], row[9])
    out["texel_ans"] = ans
    for zoom in (1, 50):
        sc = scenarios.shade_normal_scene(zoom)
        nq = out[f"normal_q_{zoom}"]
        kinds = normal_kinds(sc, nq)
        got = {}
        for fill in (0.0, 0.75):
            got[fill] = np.stack([O.ref_triangle_normal_zeroed(sc, row[1:4], row[4:7], row[7:10], row.view(np.uint32)[0], row[10], row[11], fill)
                                  for row in nq])
        # a stack filled with 0.75 instead of 0 may only change answers whose first probe misses (the uninitialised read)
        moved = np.any(got[0.0].view(np.uint32) != got[0.75].view(np.uint32), axis=1) & ~np.all(np.isnan(got[0.0]) & np.isnan(got[0.75]), axis=1)
        if np.any(moved & ~kinds["tb_miss"]):
            sys.exit(f"zoom {zoom}: the stack fill changed answers whose first probe hits the plane")
        if not np.any(moved):
            sys.exit(f"zoom {zoom}: the stack fill changed nothing: the missed-probe queries do not reach the uninitialised read")
        out[f"normal_ans_{zoom}"] = got[0.0]
    sp = np.zeros((len(out["sphere_seeds"]), 3), np.float32)
    st = np.zeros(len(sp), np.uint64)
    for j in range(len(sp)):
        s_ = C.c_uint64(int(out["sphere_seeds"][j]))
        p = O.ref().GetSpherePoint(C.byref(s_), float(out["sphere_radius"][j]))
        sp[j] = p.s[0], p.s[1], p.s[2]
        st[j] = s_.value
    out["sphere_out"], out["sphere_state"] = sp, st
    return out


def normal_kinds(sc, nq):
    """Per normal query: which edge it covers (for the coverage counts of the tests).  tb_miss / lr_miss: the probe ray
    d + tb / d + lr meets the triangle's plane outside (0, inf) (the reference leaves abL/acL unwritten, :244,:249)."""
    L = O.oracle()
    v = sc.vertex.reshape(-1, 3, 4)[:, :, :3]
    tri = nq.view(np.uint32)[:, 0].astype(np.int64)
    where, o, d = nq[:, 1:4], nq[:, 4:7], nq[:, 7:10]
    fp = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    miss = {}
    for name, off in (("tb_miss", sc.top_to_bottom[:3]), ("lr_miss", sc.left_to_right[:3])):
        m = np.zeros(len(nq), bool)
        for j in range(len(nq)):
            p = (d[j] + off).astype(np.float32)
            t, l1, l2 = C.c_float(0), C.c_float(0), C.c_float(0)
            L.rt_oracle_ray_triangle(fp(o[j]), fp(p), 0.0, float("inf"), fp(v[tri[j], 0]), fp(v[tri[j], 1]), fp(v[tri[j], 2]),
                                     C.byref(t), C.byref(l1), C.byref(l2))
            m[j] = not (0.0 < t.value < float("inf"))
        miss[name] = m
    vt = v[tri]
    on_vertex = np.any(np.all(where[:, None, :] == vt, axis=2), axis=1)
    l1, l2 = nq[:, 10], nq[:, 11]
    on_edge = ~on_vertex & ((l1 == 0) | (l2 == 0) | (l1 + l2 == 1)) & (l1 >= 0) & (l2 >= 0) & (l1 + l2 <= 1)
    a, b, c = vt[:, 0], vt[:, 1], vt[:, 2]
    degenerate = np.all(np.cross(c - a, b - a) == 0, axis=1)
    m = sc.tri_material[tri]
    bump = np.array([scenarios.NORMAL_BUMPS[k] if k >= 0 else None for k in m], dtype=object)
    image = np.array([b_ is not None and k >= 5 for b_, k in zip(bump, m)])
    return dict(tb_miss=miss["tb_miss"], lr_miss=miss["lr_miss"], vertex=on_vertex, edge=on_edge, degenerate=degenerate,
                no_material=m < 0, image_bump=image, material=m)


def make_shading(path):
    if not O.have_ref_zeroed():
        sys.exit("oracle/_ref/libref_kernel.so predates ref_glue.c's ref_triangle_normal: rebuild it with `make -C oracle`")
    save_npz_stable(path, shading_queries(answers=True))


def main():
    if not O.have_ref():
        sys.exit("oracle/_ref/libref_kernel.so missing: run `make -C oracle` where /root/reference exists")
    only = set(sys.argv[1:])  # optional: names of the fixtures to (re)write, "kat" / "fresh" / "class" / "axis" / "shading" for kat.npz /
    # ref_fresh_scenes.npz / ref_class_scenes.npz / ref_axis_scenes.npz / kat_shading.npz; default = everything
    for f in scenarios.ALL:
        if only and f.__name__ not in only:
            continue
        sc = f()
        R.build_lists(sc)
        planes = O.ref_render(sc)
        path = os.path.join(HERE, f"scene_{sc.name}.npz")
        save_scene(sc, planes, path)
        print(f"{sc.name}: {os.path.getsize(path) / 1024:.0f} KiB, lit pixels {(planes[0] > 0).mean():.2f}")
    if not only or "kat" in only:
        make_kat(os.path.join(HERE, "kat.npz"))
        print("kat.npz written")
    if not only or "fresh" in only:
        make_fresh(os.path.join(HERE, "ref_fresh_scenes.npz"))
        print("ref_fresh_scenes.npz written")
    if not only or "class" in only:
        make_class(os.path.join(HERE, "ref_class_scenes.npz"))
        print("ref_class_scenes.npz written")
    if not only or "axis" in only:
        make_axis(os.path.join(HERE, "ref_axis_scenes.npz"))
        print("ref_axis_scenes.npz written")
    if not only or "shading" in only:
        make_shading(os.path.join(HERE, "kat_shading.npz"))
        print("kat_shading.npz written")


if __name__ == "__main__":
    main()
