"""Motion vectors (include/raytrace_hip.h, "MOTION VECTORS") restated in vectorised numpy: the centre ray of every pixel, the reference
point of its hit from the barycentrics, and the projection through the reference camera by Cramer's rule.  The walks come from `walk`,
by default rt_oracle_grid_trace through query_cases.oracle_answers (whose ab / ac outputs are the barycentrics); a test on the GPU may
pass ResidentScene.intersect instead.  Every intermediate is np.float32, in the order the header writes; `dtype=np.float64` evaluates the
same formulas on the same hits in double precision (what the bounds of tests/test_motion.py are measured against).

The current state is a Scene.  The reference state is anything with the attributes eye, eye_to_top_left, left_to_right, top_to_bottom,
vertex and tri_index: a Scene, or reference(...) below."""
import types

import numpy as np

import query_cases as Q
from ao_oracle import cross, dot

F32 = np.float32
NONE = 0xFFFFFFFF


def reference(camera, vertex, tri_index):
    """A reference state from camera fields -- a Scene, ResidentScene.camera()'s dict or (eye, eye_to_top_left, left_to_right,
    top_to_bottom) -- plus vertex and index arrays."""
    if isinstance(camera, dict):
        camera = tuple(camera[k] for k in ("eye", "eye_to_top_left", "left_to_right", "top_to_bottom"))
    elif not isinstance(camera, (tuple, list)):
        camera = (camera.eye, camera.eye_to_top_left, camera.left_to_right, camera.top_to_bottom)
    eye, tl, lr, tb = (np.asarray(v, F32).reshape(-1)[:3].copy() for v in camera[:4])
    return types.SimpleNamespace(eye=eye, eye_to_top_left=tl, left_to_right=lr, top_to_bottom=tb, vertex=np.asarray(vertex, F32),
                                 tri_index=np.asarray(tri_index, np.int32))


def centre_rays(sc):
    """The ray through every pixel's centre, row-major: the AO block's primary ray at Sp = 1."""
    W, H = sc.width, sc.height
    p = np.arange(W * H, dtype=np.int64)
    fx, fy = (p % W).astype(F32) + F32(0.5), (p // W).astype(F32) + F32(0.5)
    tl, lr, tb = (np.asarray(v, F32).reshape(-1)[:3] for v in (sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom))
    d = (tl[None, :] + lr[None, :] * fx[:, None]) + tb[None, :] * fy[:, None]
    o = np.broadcast_to(np.asarray(sc.eye, F32).reshape(-1)[:3], d.shape)
    rs = Q._set(o, d, 0.0, np.inf, NONE)
    rs["fx"], rs["fy"] = fx, fy
    return rs


def trace(sc, walk=None):
    """The centre rays and their hits: (ray set, triangle u32, t, abL, acL f32)."""
    if walk is None:
        def walk(rs):
            return Q.oracle_answers(sc, rs)
    rs = centre_rays(sc)
    hit = walk(rs)
    return rs, np.asarray(hit["triangle"], np.uint32), np.asarray(hit["t"], F32), np.asarray(hit["ab"], F32), np.asarray(hit["ac"], F32)


def project(sc, ref, traced, dtype=F32):
    """Steps 1 to 4 of the header on the hits of trace(): {"motion" [H, W, 2], "t", "prev_t" [H, W] of `dtype`, "triangle" [H, W] u32}."""
    rs, tri, t, ab_l, ac_l = traced
    X = dtype
    hit = tri != NONE
    E, TL, lr, tb = (np.asarray(v, F32).reshape(-1)[:3].astype(X) for v in (ref.eye, ref.eye_to_top_left, ref.left_to_right, ref.top_to_bottom))
    v = np.asarray(ref.vertex, F32)[:, :3]
    ix = np.asarray(ref.tri_index, np.int64)[np.where(hit, tri, 0).astype(np.int64), :3] if len(ref.tri_index) else np.zeros((len(tri), 3), np.int64)
    with np.errstate(all="ignore"):
        if len(v):
            a = v[ix[:, 0]]
            ab, ac = v[ix[:, 1]] - a, v[ix[:, 2]] - a  # fp32, as the triangle records hold them
        else:
            a = ab = ac = np.zeros((len(tri), 3), F32)
        a, ab, ac = a.astype(X), ab.astype(X), ac.astype(X)
        P = (a + ab_l.astype(X)[:, None] * ab) + ac_l.astype(X)[:, None] * ac
        w = np.where(hit[:, None], P - E[None, :], rs["d"].astype(X))
        n = cross(lr, tb)
        den = dot(w, n[None, :])
        px = dot(TL[None, :], cross(w, tb[None, :])) / den
        py = dot(TL[None, :], cross(lr[None, :], w)) / den
        motion = np.stack([px - rs["fx"].astype(X), py - rs["fy"].astype(X)], -1)
        prev_t = np.where(hit, den / dot(TL, n), X(np.inf))
    shape = (sc.height, sc.width)
    return dict(motion=motion.astype(X).reshape(shape + (2,)), t=np.where(hit, t, F32(np.inf)).astype(X).reshape(shape),
                prev_t=prev_t.astype(X).reshape(shape), triangle=np.where(hit, tri, NONE).astype(np.uint32).reshape(shape))


def motion(sc, ref, walk=None, dtype=F32, with_hits=False):
    """The four outputs for current state `sc` (a Scene) against reference state `ref`; with_hits: also trace()'s tuple."""
    traced = trace(sc, walk)
    out = project(sc, ref, traced, dtype)
    return (out, traced) if with_hits else out


def same_bits(got, want):
    """Element-wise: equal bit patterns, or a NaN on both sides."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype == np.uint32 or got.dtype == np.int32:
        return got.view(np.uint32) == want.view(np.uint32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
