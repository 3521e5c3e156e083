"""The depth of field of include/raytrace_hip.h ("DEPTH OF FIELD") restated in numpy: fp32 throughout, the header's order of operations,
vectorised over the image per tap; and the lens helper (rtHipDepthOfFieldLens) in float64.  The device (tests/test_dof_gpu.py) and the
kernel's per-pixel code compiled for the host (tests/test_dof.py) are compared with this bit for bit; a NaN on both sides counts as equal."""
import numpy as np

F32 = np.float32
F64 = np.float64
DEFAULTS = dict(focus=1.0, coc_scale=8.0, max_coc=16.0, rings=3, depth_softness=0.05)
TILE = 32
ZERO, HALF, ONE = F32(0.0), F32(0.5), F32(1.0)
C8 = F32(0.70710678)
V = np.array([(1, 0), (C8, C8), (0, 1), (-C8, C8), (-1, 0), (-C8, -C8), (0, -1), (C8, -C8), (1, 0)], F32)  # the unit octagon, closed


def same_bits(a, b):
    """Elementwise: the same fp32 bit pattern, or a NaN on both sides."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def clamp01(r):
    return np.where(~(r > ZERO), ZERO, np.where(r > ONE, ONE, r))


def sdc(a, b, e):
    return np.where(a == b, ONE, clamp01(ONE - (a - b) / e))


def taps(rings):
    """The (k, s) of every ring tap in the order of (d)."""
    return [(k, s) for k in range(1, int(rings) + 1) for s in range(8 * k)]


def tap_count(rings):
    return 1 + 4 * int(rings) * (int(rings) + 1)


def radius(depth, focus, coc_scale, max_coc):
    """(a): r per pixel; never negative, never a NaN."""
    z, focus, scale, cap = np.ascontiguousarray(depth, F32), F32(focus), F32(coc_scale), F32(max_coc)
    with np.errstate(all="ignore"):
        hit = (z > ZERO) & ~(z == F32(np.inf))
        a = np.where(z == F32(np.inf), ONE, np.where(hit, np.abs(z - focus) / np.where(hit, z, ONE), ZERO))
        r = a * scale
        return np.where(~(r < cap), cap if scale > ZERO else ZERO, r).astype(F32)


def tile_max(r):
    """(b): [tilesY, tilesX], the greatest r of every 32 x 32 tile."""
    H, W = r.shape
    out = np.zeros(((H + TILE - 1) // TILE, (W + TILE - 1) // TILE), F32)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            out[ty, tx] = r[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].max()
    return out


def nb_max(tiles):
    """(c): per tile the greatest of the 3 x 3 tiles around it that exist."""
    out = np.zeros_like(tiles)
    for ty in range(tiles.shape[0]):
        for tx in range(tiles.shape[1]):
            out[ty, tx] = tiles[max(ty - 1, 0):ty + 2, max(tx - 1, 0):tx + 2].max()
    return out


def blur(colour, depth, focus=DEFAULTS["focus"], coc_scale=DEFAULTS["coc_scale"], max_coc=DEFAULTS["max_coc"], rings=DEFAULTS["rings"],
         depth_softness=DEFAULTS["depth_softness"], with_parts=False):
    """out [H, W, 3] f32; with_parts: a dict with "out" and the intermediate results -- "r" (a), "tile_max" (b), "nb_max" (c), "gathered"
    (which pixels take the gather arm of (d)), "taps" (how many ring taps each pixel summed)."""
    colour, depth = np.ascontiguousarray(colour, F32), np.ascontiguousarray(depth, F32)
    H, W = depth.shape
    with np.errstate(all="ignore"):
        r = radius(depth, focus, coc_scale, max_coc)
        tiles = tile_max(r)
        nb = nb_max(tiles)
        y, x = np.indices((H, W))
        R = nb[y >> 5, x >> 5]
        gathered = R >= HALF
        if not gathered.any():  # (every pixel copies: the taps below would be computed and thrown away)
            out = colour.copy()
            return dict(out=out, r=r, tile_max=tiles, nb_max=nb, gathered=gathered, taps=np.zeros((H, W), np.int32)) if with_parts else out
        rp = np.where(r < HALF, HALF, r)
        zp = depth
        j = ((x & 1) * 2 + (y & 1) * 3) & 3
        jit = (j.astype(F32) - F32(1.5)) * F32(0.25)
        wsum = ONE / (rp * rp)
        total = colour * wsum[..., None]
        px, py = x.astype(F32) + HALF, y.astype(F32) + HALF
        soft, n, used = F32(depth_softness), F32(rings), np.zeros((H, W), np.int32)
        for k, s in taps(rings):
            v, m = s // k, s % k
            f = F32(m) / F32(k)
            ux, uy = V[v, 0] + (V[v + 1, 0] - V[v, 0]) * f, V[v, 1] + (V[v + 1, 1] - V[v, 1]) * f
            rad = ((F32(k) + jit) / n) * R
            ox, oy = ux * rad, uy * rad
            X, Y = px + ox, py + oy
            ok = (X >= ZERO) & (X < F32(W)) & (Y >= ZERO) & (Y < F32(H))
            qx, qy = np.where(ok, X, ZERO).astype(np.int32), np.where(ok, Y, ZERO).astype(np.int32)
            d = np.sqrt(ox * ox + oy * oy)
            rq = r[qy, qx]
            rq = np.where(rq < HALF, HALF, rq)
            zq = depth[qy, qx]
            e = soft * np.where(zp < zq, zp, zq)
            fr = sdc(zq, zp, e)
            m2 = np.where(rq < rp, rq, rp)
            reff = rq * fr + m2 * (ONE - fr)
            w = clamp01((reff - d) + HALF) / (reff * reff)
            wsum = np.where(ok, wsum + w, wsum)
            total = np.where(ok[..., None], total + colour[qy, qx] * w[..., None], total)
            used += ok & gathered
        out = np.where(gathered[..., None], total / wsum[..., None], colour)
    if not with_parts:
        return out
    return dict(out=out, r=r, tile_max=tiles, nb_max=nb, gathered=gathered, taps=used)


def focal_pixels(eye_to_top_left, left_to_right, top_to_bottom):
    """The distance from the eye to the image plane over the pixel pitch, in float64 with + - * / and sqrt (lane 3 not read)."""
    tl, lr, tb = (np.asarray(v, F32).astype(F64) for v in (eye_to_top_left, left_to_right, top_to_bottom))

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    with np.errstate(all="ignore"):
        n = (lr[1] * tb[2] - lr[2] * tb[1], lr[2] * tb[0] - lr[0] * tb[2], lr[0] * tb[1] - lr[1] * tb[0])
        h = dot(tl, n)
        if h < 0:
            h = -h
        return (h / np.sqrt(dot(n, n))) / np.sqrt(dot(lr, lr)), h / np.sqrt(dot(n, n)), np.sqrt(dot(lr, lr))


def lens(camera, aperture, focus):
    """rtHipDepthOfFieldLens: (focus, cocScale) as float32, or None where the call refuses.  `camera`: a dict with eye_to_top_left,
    left_to_right and top_to_bottom."""
    fp, plane, pitch = focal_pixels(camera["eye_to_top_left"], camera["left_to_right"], camera["top_to_bottom"])
    if not (np.isfinite(plane) and plane > 0 and np.isfinite(pitch) and pitch > 0):
        return None
    with np.errstate(all="ignore"):
        focus = F32(focus)
        scale = F32((F64(F32(aperture)) * fp) / F64(focus))
    if not (np.isfinite(focus) and focus > 0 and np.isfinite(scale) and 0 <= scale <= 4096):
        return None
    return focus, scale
