"""Ambient occlusion (include/raytrace_hip.h, "AMBIENT OCCLUSION") restated in vectorised numpy: the splitmix64 hash, the primary rays,
hit points and oriented normals, the Duff et al. frame, Malley's method and the count.  The walks come from `walk`, by default
rt_oracle_grid_trace through query_cases.oracle_answers; a test on the GPU may pass ResidentScene.intersect instead.

uint64 arithmetic on numpy arrays wraps mod 2^64 without a warning; every hash below runs on arrays, never on numpy scalars (whose
overflow warns)."""
import numpy as np

import query_cases as Q

F32 = np.float32
U64 = np.uint64
NONE = 0xFFFFFFFF
_M1, _M2, _GAMMA = U64(0xBF58476D1CE4E5B9), U64(0x94D049BB133111EB), U64(0x9E3779B97F4A7C15)


def mix(z):
    """splitmix64's finaliser on a uint64 array."""
    z = np.atleast_1d(np.asarray(z, U64))
    z = (z ^ (z >> U64(30))) * _M1
    z = (z ^ (z >> U64(27))) * _M2
    return z ^ (z >> U64(31))


def hashes(seed, c):
    """h(c) = mix(S0 + (c + 1) * 0x9E3779B97F4A7C15), S0 = mix(seed), for a uint64 array of counters c."""
    s0 = mix(np.array([seed], U64))
    return mix(s0 + (np.atleast_1d(np.asarray(c, U64)) + U64(1)) * _GAMMA)


def uniform(seed, c):
    """U(c) = (float)(h(c) >> 40) * 2^-24 (exact)."""
    return (hashes(seed, c) >> U64(40)).astype(F32) * F32(2.0 ** -24)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def hemisphere(n, counters, seed):
    """Directions of AO rays around unit normals n [N, 3] f32: counters [N, K] uint64 are each ray's c at draw 0 (its slot's first
    counter); returns [N, K, 3] f32."""
    n = np.asarray(n, F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nx, ny, nz = n[:, 0:1], n[:, 1:2], n[:, 2:3]
        s = np.where(nz >= F32(0), F32(1), F32(-1))
        a = F32(-1) / (s + nz)
        b = (nx * ny) * a
        t1 = np.stack([F32(1) + ((s * nx) * nx) * a, s * b, -(s * nx)], -1)
        t2 = np.stack([b, s + (ny * ny) * a, -ny], -1)
        c = np.asarray(counters, U64)
        xd, yd, r2 = (np.zeros(c.shape, F32) for _ in range(3))
        todo = np.ones(c.shape, bool)
        for k in range(16):
            if not todo.any():
                break
            idx = np.nonzero(todo)
            cc = c[idx]
            x = F32(2) * uniform(seed, cc + U64(2 * k)) - F32(1)
            y = F32(2) * uniform(seed, cc + U64(2 * k + 1)) - F32(1)
            q = x * x + y * y
            take = q < F32(1)
            sel = tuple(i[take] for i in idx)
            xd[sel], yd[sel], r2[sel] = x[take], y[take], q[take]
            todo[sel] = False
        z = np.sqrt(F32(1) - r2)
        return (xd[..., None] * t1 + yd[..., None] * t2) + z[..., None] * n[:, None, :]


def primary_rays(sc, pixel_samples=1, rays=16, seed=0):
    """The primary ray of every pixel sample, in the order (p, j): a query_cases ray set plus p and j."""
    W, H, Sp, R = sc.width, sc.height, pixel_samples, rays
    p = np.repeat(np.arange(W * H, dtype=np.int64), Sp)
    j = np.tile(np.arange(Sp, dtype=np.int64), W * H)
    if Sp == 1:
        u = v = np.full(len(p), F32(0.5))
    else:
        c = ((p * Sp + j) * (R + 1) * 32).astype(U64)
        u, v = uniform(seed, c), uniform(seed, c + U64(1))
    fx, fy = (p % W).astype(F32) + u, (p // W).astype(F32) + v
    tl, lr, tb = (np.asarray(x, F32)[:3] for x in (sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom))
    d = (tl[None, :] + lr[None, :] * fx[:, None]) + tb[None, :] * fy[:, None]
    o = np.broadcast_to(np.asarray(sc.eye, F32)[:3], d.shape)
    rs = Q._set(o, d, 0.0, np.inf, NONE)
    rs["p"], rs["j"] = p, j
    return rs


def ambient_occlusion(sc, rays=16, radius=np.inf, pixel_samples=1, seed=0, walk=None, with_rays=False):
    """The [H, W] f32 AO image of Scene sc.  walk(ray set) -> dict with "triangle" (u32) and "t" (f32): the grid walk, by default
    rt_oracle_grid_trace.  with_rays: also returns {"primary": ray set, "ao": ray set, "sample": the pixel sample index of each AO ray}."""
    if walk is None:
        def walk(rs):
            return Q.oracle_answers(sc, rs)
    R, Sp = int(rays), int(pixel_samples)
    pr = primary_rays(sc, Sp, R, seed)
    hit = walk(pr)
    tri = np.asarray(hit["triangle"], np.uint32)
    t = np.asarray(hit["t"], F32)
    got = np.flatnonzero(tri != NONE)
    o, d = pr["o"][got], pr["d"][got]
    with np.errstate(invalid="ignore", over="ignore"):
        P = o + t[got, None] * d
        v = np.asarray(sc.vertex, F32)[:, :3]
        ix = np.asarray(sc.tri_index, np.int64)[tri[got], :3]
        a, b, c = v[ix[:, 0]], v[ix[:, 1]], v[ix[:, 2]]
        n = cross(c - a, b - a)
        n = np.where((dot(n, d) > F32(0))[:, None], -n, n)
        m = dot(n, n)
        ok = m > F32(0)
        n = n / np.sqrt(m)[:, None]
    live = got[ok]
    P, n = P[ok], n[ok]
    counters = (((pr["p"][live] * Sp + pr["j"][live]) * (R + 1))[:, None] + 1 + np.arange(R)[None, :]) * 32
    dirs = hemisphere(n, counters.astype(U64), seed).reshape(-1, 3)
    ao = Q._set(np.repeat(P, R, 0), dirs, 0.0, F32(radius), np.repeat(tri[live], R))
    occluded = np.asarray(walk(ao)["triangle"], np.uint32) != NONE
    open_rays = np.full(len(pr["p"]), R, np.int64)
    open_rays[live] = R - occluded.reshape(-1, R).sum(1)
    U = open_rays.reshape(sc.width * sc.height, Sp).sum(1)
    img = (U.astype(F32) / F32(Sp * R)).reshape(sc.height, sc.width)
    if with_rays:
        return img, dict(primary=pr, ao=ao, sample=np.repeat(live, R))
    return img
