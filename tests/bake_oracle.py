"""The ambient occlusion bake (include/raytrace_hip.h, "AMBIENT OCCLUSION BAKE") restated in vectorised numpy: texel centres, coverage
with the smallest-id rule, surface points and oriented normals, the AO rays (directions from ao_oracle.hemisphere with the bake's
counters), the count and the dilation.  The walks come from `walk`, by default rt_oracle_grid_trace through query_cases.oracle_answers;
a test on the GPU may pass ResidentScene.intersect instead.

Coverage is tested texel by texel against every selected triangle (blocks of triangles, smallest ids first).  For maps too large for
that, `rects=True` tests each triangle over its UV bounding box grown by two texels, which holds every texel the test can pass for a
triangle that is not a sliver; slivers (|den| <= 1e-3 of the largest edge component squared) and triangles with an infinite UV are
still tested over the whole map."""
import numpy as np

import ao_oracle as A
import query_cases as Q

F32 = np.float32
U64 = np.uint64
NONE = 0xFFFFFFFF


def centres(W, H):
    """cu [W], cv [H]: ((float)i + 0.5f) / (float)n."""
    return ((np.arange(W).astype(F32) + F32(0.5)) / F32(W)), ((np.arange(H).astype(F32) + F32(0.5)) / F32(H))


def cover(uv, cu, cv):
    """uv [B, 3, 2] f32 corners, cu / cv [N] f32 texel centres -> (covered [B, N], l1 [B, N], l2 [B, N])."""
    uv = np.asarray(uv, F32)
    ax, ay = uv[:, 0, 0:1], uv[:, 0, 1:2]
    e1x, e1y = uv[:, 1, 0:1] - ax, uv[:, 1, 1:2] - ay
    e2x, e2y = uv[:, 2, 0:1] - ax, uv[:, 2, 1:2] - ay
    with np.errstate(all="ignore"):
        qx, qy = np.asarray(cu, F32)[None, :] - ax, np.asarray(cv, F32)[None, :] - ay
        den = e1x * e2y - e1y * e2x
        l1 = (qx * e2y - qy * e2x) / den
        l2 = (e1x * qy - e1y * qx) / den
        return (l1 >= F32(0)) & (l2 >= F32(0)) & (l1 + l2 <= F32(1)), l1, l2


def selected(sc, triangles=None, material=None):
    """The selected triangle ids, ascending: triangles None (all), a range, or (first, count); material None or an id."""
    T = sc.triangle_count
    if triangles is None:
        ids = np.arange(T)
    elif isinstance(triangles, range):
        ids = np.arange(triangles.start, triangles.stop)
    else:
        ids = np.arange(int(triangles[0]), int(triangles[0]) + int(triangles[1]))
    if material is not None:
        ids = ids[np.asarray(sc.tri_material, np.int32)[ids] == np.int32(material)]
    return ids.astype(np.int64)


def _brute(uvs, ids, cu, cv, W, win):
    """Every texel against every triangle of `ids` (ascending), the first covering one wins where win is still NONE."""
    N = len(cu)
    block = max(1, (1 << 22) // max(N, 1))
    for s in range(0, len(ids), block):
        part = ids[s:s + block]
        m, _, _ = cover(uvs[part], cu, cv)
        hit = m.any(0)
        first = part[np.argmax(m, 0)]
        take = hit & (win == NONE)
        win[take] = first[take]
    return win


def coverage(sc, W, H, triangles=None, material=None, rects=False):
    """The triangle map [H*W] u32 (row-major, t = y*W + x): the smallest selected id covering each texel, NONE where none does."""
    uvs = np.asarray(sc.tri_uv, F32).reshape(-1, 3, 2)
    ids = selected(sc, triangles, material)
    cu1, cv1 = centres(W, H)
    cu, cv = np.tile(cu1, H), np.repeat(cv1, W)
    win = np.full(W * H, NONE, np.uint32)
    if not rects:
        return _brute(uvs, ids, cu, cv, W, win)
    u = uvs[ids].astype(np.float64)
    with np.errstate(all="ignore"):
        e1, e2 = u[:, 1] - u[:, 0], u[:, 2] - u[:, 0]
        D = np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])
        E = np.abs(np.concatenate([e1, e2], 1)).max(1)
        lo, hi = u.min(1), u.max(1)
        x0 = np.floor(lo[:, 0] * W - 0.5) - 2
        x1 = np.ceil(hi[:, 0] * W - 0.5) + 2
        y0 = np.floor(lo[:, 1] * H - 0.5) - 2
        y1 = np.ceil(hi[:, 1] * H - 0.5) + 2
    finite = np.isfinite(u).all((1, 2))
    whole = ~finite | ~(D > 1e-3 * E * E)
    whole &= ~np.isnan(u).any((1, 2))  # (NaN covers nothing)
    keep = ~whole & finite & (x1 >= 0) & (y1 >= 0) & (x0 <= W - 1) & (y0 <= H - 1)
    kid = ids[keep]
    x0, x1 = np.clip(x0[keep], 0, W - 1).astype(np.int64), np.clip(x1[keep], 0, W - 1).astype(np.int64)
    y0, y1 = np.clip(y0[keep], 0, H - 1).astype(np.int64), np.clip(y1[keep], 0, H - 1).astype(np.int64)
    best = np.full(W * H, np.iinfo(np.int64).max, np.int64)
    kx, ky = x1 - x0 + 1, y1 - y0 + 1
    for w in np.unique(kx):
        for h in np.unique(ky[kx == w]):
            g = np.flatnonzero((kx == w) & (ky == h))
            for s in range(0, len(g), max(1, (1 << 22) // int(w * h))):
                gg = g[s:s + max(1, (1 << 22) // int(w * h))]
                xs = (x0[gg, None, None] + np.arange(w)[None, None, :]) + 0 * np.arange(h)[None, :, None]
                ys = (y0[gg, None, None] + np.arange(h)[None, :, None]) + 0 * np.arange(w)[None, None, :]
                xs, ys = xs.reshape(len(gg), -1), ys.reshape(len(gg), -1)
                ux = uvs[kid[gg]]
                m, _, _ = _cover_pairs(ux, cu1[xs], cv1[ys])
                t = (ys * W + xs)[m]
                np.minimum.at(best, t, np.broadcast_to(kid[gg][:, None], m.shape)[m])
    win[best != np.iinfo(np.int64).max] = best[best != np.iinfo(np.int64).max].astype(np.uint32)
    wid = ids[whole]
    if len(wid):
        extra = _brute(uvs, wid, cu, cv, W, np.full(W * H, NONE, np.uint32))
        win = np.where((extra != NONE) & ((win == NONE) | (extra < win)), extra, win).astype(np.uint32)
    return win


def _cover_pairs(uv, cu, cv):
    """cover() with a texel set per triangle: uv [B, 3, 2], cu / cv [B, K]."""
    uv = np.asarray(uv, F32)
    ax, ay = uv[:, 0, 0:1], uv[:, 0, 1:2]
    e1x, e1y = uv[:, 1, 0:1] - ax, uv[:, 1, 1:2] - ay
    e2x, e2y = uv[:, 2, 0:1] - ax, uv[:, 2, 1:2] - ay
    with np.errstate(all="ignore"):
        qx, qy = cu - ax, cv - ay
        den = e1x * e2y - e1y * e2x
        l1 = (qx * e2y - qy * e2x) / den
        l2 = (e1x * qy - e1y * qx) / den
        return (l1 >= F32(0)) & (l2 >= F32(0)) & (l1 + l2 <= F32(1)), l1, l2


def surface(sc, W, H, win):
    """For the covered texels (t = flatnonzero(win != NONE)): (t, P [n, 3], unit normal [n, 3], ok [n]); ok False = zero normal."""
    t = np.flatnonzero(win != NONE)
    tri = win[t].astype(np.int64)
    cu1, cv1 = centres(W, H)
    uvs = np.asarray(sc.tri_uv, F32).reshape(-1, 3, 2)[tri]
    _, l1, l2 = _cover_pairs(uvs, cu1[t % W][:, None], cv1[t // W][:, None])
    l1, l2 = l1[:, 0], l2[:, 0]
    v = np.asarray(sc.vertex, F32)[:, :3]
    ix = np.asarray(sc.tri_index, np.int64)[tri, :3]
    a, b, c = v[ix[:, 0]], v[ix[:, 1]], v[ix[:, 2]]
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        P = (a + l1[:, None] * ab) + l2[:, None] * ac
        n = A.cross(ac, ab)
        cn = np.asarray(sc.tri_normal, F32)[:, :3].reshape(-1, 3, 3)[tri]
        s = (cn[:, 0] + cn[:, 1]) + cn[:, 2]
        n = np.where((A.dot(n, s) < F32(0))[:, None], -n, n)
        m = A.dot(n, n)
        ok = m > F32(0)
        n = n / np.sqrt(m)[:, None]
    return t, P, n, ok


def dilate(values, valid, W, H, G):
    """G Jacobi gutter-fill passes over [H*W] f32 values (valid: [H*W] bool); texels still invalid at the end are 0."""
    v = np.asarray(values, F32).reshape(H, W).copy()
    ok = np.asarray(valid, bool).reshape(H, W).copy()
    for _ in range(int(G)):
        pv = np.zeros((H + 2, W + 2), F32)
        pk = np.zeros((H + 2, W + 2), bool)
        pv[1:-1, 1:-1], pk[1:-1, 1:-1] = np.where(ok, v, F32(0)), ok
        total = np.zeros((H, W), F32)
        k = np.zeros((H, W), np.int64)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                nv, nk = pv[1 + dy:1 + dy + H, 1 + dx:1 + dx + W], pk[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
                total = total + np.where(nk, nv, F32(0))  # (+0 for an invalid neighbour: the sum is >= +0, so adding +0 changes nothing)
                k += nk
        fill = ~ok & (k > 0)
        with np.errstate(all="ignore"):
            v = np.where(fill, total / k.astype(F32), v).astype(F32)
        ok = ok | fill
    return np.where(ok, v, F32(0)).astype(F32).reshape(-1)


def bake(sc, width, height, rays=16, radius=np.inf, seed=0, dilate_passes=2, triangles=None, material=None, walk=None, rects=False,
         with_rays=False):
    """{"ao": [H, W] f32, "triangle": [H, W] u32} of the bake of Scene sc (its tri_uv).  walk(ray set) -> dict with "triangle" (u32):
    the grid walk, by default rt_oracle_grid_trace.  with_rays: also "rays" (the AO ray set) and "texel" (each ray's texel)."""
    if walk is None:
        def walk(rs):
            return Q.oracle_answers(sc, rs)
    W, H, R = int(width), int(height), int(rays)
    win = coverage(sc, W, H, triangles, material, rects)
    t, P, n, ok = surface(sc, W, H, win)
    U = np.zeros(W * H, np.int64)
    U[t[~ok]] = R
    live = t[ok]
    P, n = P[ok], n[ok]
    counters = ((live.astype(np.int64) * (R + 1))[:, None] + 1 + np.arange(R)[None, :]) * 32
    dirs = A.hemisphere(n, counters.astype(U64), seed).reshape(-1, 3)
    rs = Q._set(np.repeat(P, R, 0), dirs, 0.0, F32(radius), np.repeat(win[live], R))
    if len(live):
        occluded = np.asarray(walk(rs)["triangle"], np.uint32) != NONE
        U[live] = R - occluded.reshape(-1, R).sum(1)
    covered = win != NONE
    val = np.where(covered, U.astype(F32) / F32(R), F32(0)).astype(F32)
    ao = dilate(val, covered, W, H, dilate_passes).reshape(H, W)
    out = dict(ao=ao, triangle=win.reshape(H, W))
    if with_rays:
        out["rays"], out["texel"] = rs, np.repeat(live, R)
    return out
