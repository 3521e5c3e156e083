"""Sample windows (include/raytrace_hip.h, "SAMPLE WINDOWS"): what tests/test_sample_window.py and tests/test_sample_window_gpu.py share
-- the golden scenes with another sample count, the oracle's N-sample frames (computed once each and never written to), the cases of
the progressive test, and the render passes restated for a window's seeds."""
import ctypes as C
import dataclasses
import os

import numpy as np

import oracle_lib as O
from conftest import load_golden_scene
from opencl_render_amd import scene as S

SATURATED = 65535

# (golden scene, the S it was minted with, N): progressive rendering in N / S frames equals the oracle's N-sample frame.
# degenerate_and_outside has 5.8 % of its golden saturated and one negative light: the case that proves the order of the saturating adds.
PROGRESSIVE = [("lambert_distant", 2, 8), ("mixed_materials_textured", 2, 6), ("mirror_hall", 2, 4), ("degenerate_and_outside", 3, 12),
               ("all_light_types", 1, 3), ("odd_size_multi_tile", 1, 4)]
# the one-sample scenes of the divisor test, with the shares of their golden's plane values that are non-zero / saturated (the test's
# premises: checked against the fixtures without a GPU)
DIVISOR_SCENES = {"all_light_types": (0.079, 0.0), "primary_only": (0.107, 0.0001), "odd_size_multi_tile": (0.194, 0.0)}

U32_MAX = 2 ** 32 - 1
# every refusal of rtHipSampleWindowCheck: what tests/test_sample_window.py asserts one by one and the session sequences draw from
REFUSALS = [
    # (S, window, what the error text must say)
    (2, (0, 0, 2, 0, 0), "total must be >= 1"),
    (2, (8, 0, 0, 0, 0), "divisor must be >= 1"),
    (2, (8, 7, 8, 0, 0), "reaches past total"),
    (3, (U32_MAX, U32_MAX - 2, 1, 0, 0), "reaches past total"),      # f + S = 2^32 - 2 + 3 wraps in 32 bits: compared in 64
    (U32_MAX, (U32_MAX, 1, 1, 0, 0), "reaches past total"),
    (2, (8, 0, 8, 2, 0), "accumulate must be 0 or 1"),
    (2, (8, 0, 8, 0, 2), "advance must be 0 or 1"),
    (2, (8, 0, 8, U32_MAX, 0), "accumulate must be 0 or 1"),
    (3, (8, 0, 8, 0, 1), "multiple of sampleCount"),                  # N % S != 0
    (2, (8, 1, 8, 0, 1), "advance needs first"),                      # f % S != 0
]

THREADS = min(os.cpu_count() or 1, 16)

_golden = {}
_oracle = {}


def golden(name):
    """(Scene, golden planes) of tests/golden/scene_<name>.npz, loaded once."""
    if name not in _golden:
        _golden[name] = load_golden_scene(name)
    return _golden[name]


def with_samples(sc, samples):
    """The same scene (arrays shared) with another sample count."""
    return dataclasses.replace(sc, sample_count=int(samples))


def oracle_frame(name, total):
    """The oracle's frame of the golden scene `name` at sample_count = total: three read-only [H, W] u16 planes, computed once."""
    key = (name, int(total))
    if key not in _oracle:
        planes = O.oracle_render(with_samples(golden(name)[0], total), threads=min(os.cpu_count() or 1, 16))
        for p in planes:
            p.setflags(write=False)
        _oracle[key] = planes
    return _oracle[key]


def _frozen(planes):
    for p in planes:
        p.setflags(write=False)
    return planes


def window_frame(name, total, first, divisor, samples=None):
    """The window oracle's frame {total, first, divisor} of the golden scene `name` (at another sample count where `samples` is given)
    from zeros: three read-only [H, W] u16 planes, computed once."""
    key = (name, int(total), int(first), int(divisor), samples)
    if key not in _oracle:
        sc = golden(name)[0]
        sc = sc if samples is None else with_samples(sc, samples)
        _oracle[key] = _frozen(O.oracle_render_window(sc, total, first, divisor, threads=THREADS))
    return _oracle[key]


def window_chain(name, total):
    """The tile buffer after each frame of progressive rendering {total, 0, total, 1, 1} of the golden scene `name`, by the window
    oracle: total / S triples of read-only planes, each frame added onto the one before; computed once."""
    key = (name, int(total), "chain")
    if key not in _oracle:
        sc = golden(name)[0]
        out, planes = [], None
        for f in range(0, total, sc.sample_count):
            planes = _frozen(O.oracle_render_window(sc, total, f, total, onto=planes, threads=THREADS))
            out.append(planes)
        _oracle[key] = out
    return _oracle[key]


def shares(planes):
    """(share of the plane values that are non-zero, share that equals 65535) over the three planes."""
    a = np.concatenate([np.asarray(p).ravel() for p in planes])
    return float((a != 0).mean()), float((a == SATURATED).mean())


def differing(got, want):
    """Plane values that differ, over the three planes."""
    return sum(int((np.asarray(g).reshape(np.asarray(w).shape) != w).sum()) for g, w in zip(got, want))


def window_passes(sc, total, first):
    """alpha u16, depth f32, triangle u32 [H, W] and normal, albedo [H, W, 3] f32 of a frame that renders sample ids first+1 .. first+S of
    a sequence of `total`: the definitions tests/test_passes_gpu.py and tests/test_surface_passes_gpu.py restate, with sample s of pixel p
    seeded p*total + first + s.  "Sample 1" (depth, triangle) is sample id first + 1; alpha and the means divide by S."""
    L = O.oracle()
    fp = C.POINTER(C.c_float)
    L.rt_oracle_shading_normal.argtypes = [C.POINTER(O.OracleScene), fp, fp, fp, C.c_uint32, C.c_float, C.c_float, fp]
    osc = O.oracle_scene(sc, [np.zeros(1, np.uint16) for _ in range(3)])
    f3 = C.c_float * 3
    W, H, S_ = sc.width, sc.height, sc.sample_count
    eye = np.asarray(sc.eye, np.float32)[:3]
    eye_c = f3(*[float(v) for v in eye])
    tl, lr, tb = (np.asarray(v, np.float32)[:3] for v in (sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom))
    verts = [[f3(*[float(c) for c in sc.vertex[int(i)][:3]]) for i in sc.tri_index[t][:3]] for t in range(sc.triangle_count)]
    mat_size = np.asarray(sc.mat_size, np.uint32).reshape(-1, 2)
    tri_uv = np.ascontiguousarray(sc.tri_uv, np.float32).reshape(-1, 6)
    alpha = np.zeros(H * W, np.uint16)
    depth = np.full(H * W, np.inf, np.float32)
    tri = np.full(H * W, 0xFFFFFFFF, np.uint32)
    normal = np.zeros((H * W, 3), np.float32)
    albedo = np.zeros((H * W, 3), np.float32)
    t, l1, l2 = C.c_float(), C.c_float(), C.c_float()
    n_out, a_out = np.zeros(3, np.float32), np.zeros(3, np.float32)
    for p in range(H * W):
        x, y = p % W, p // W
        cands = [int(c) for c in sc.cam_list[int(sc.cam_start[p]):int(sc.cam_end[p])]]
        acc_n, acc_a, hits = np.zeros(3, np.float32), np.zeros(3, np.float32), 0
        for s in range(1, S_ + 1):
            state = C.c_uint64(p * total + first + s)
            kx = np.float32(x) + np.float32(L.rt_oracle_randf(C.byref(state), 0.0, 1.0))
            ky = np.float32(y) + np.float32(L.rt_oracle_randf(C.byref(state), 0.0, 1.0))
            d = tl.copy()
            d = d + lr * kx
            d = d + tb * ky
            dc = f3(*[float(v) for v in d])
            best, best_t, best_l1, best_l2 = None, np.float32(np.inf), 0.0, 0.0
            for c in cands:
                a, b, cc = verts[c]
                if L.rt_oracle_ray_triangle(eye_c, dc, 0.0, float(best_t), a, b, cc, C.byref(t), C.byref(l1), C.byref(l2)):
                    best, best_t, best_l1, best_l2 = c, np.float32(t.value), l1.value, l2.value
            n_s, a_s = np.zeros(3, np.float32), np.zeros(3, np.float32)
            if best is not None:
                hits += 1
                if s == 1:
                    tri[p] = best
                    depth[p] = best_t * np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                where = eye + best_t * d
                L.rt_oracle_shading_normal(C.byref(osc), where.ctypes.data_as(fp), eye.ctypes.data_as(fp), d.ctypes.data_as(fp), best,
                                           best_l1, best_l2, n_out.ctypes.data_as(fp))
                n_s = n_out.copy()
                m = int(sc.tri_material[best])
                if m >= 0:
                    cw, ch = (int(v) for v in mat_size[S.CH_COUNT * m + S.CH_COLOR])
                    if cw > 0:
                        table = sc.textures[int(sc.mat_start[S.CH_COUNT * m + S.CH_COLOR]):]
                        L.rt_oracle_texel(table.ctypes.data_as(C.c_void_p), cw, ch, tri_uv[best].ctypes.data_as(fp), best_l1, best_l2,
                                          a_out.ctypes.data_as(fp))
                        a_s = a_out.copy()
            acc_n = acc_n + n_s
            acc_a = acc_a + a_s
        alpha[p] = hits * 65535 // S_
        normal[p] = acc_n / np.float32(S_)
        albedo[p] = acc_a / np.float32(S_)
    return dict(alpha=alpha.reshape(H, W), depth=depth.reshape(H, W), triangle=tri.reshape(H, W), normal=normal.reshape(H, W, 3),
                albedo=albedo.reshape(H, W, 3))
