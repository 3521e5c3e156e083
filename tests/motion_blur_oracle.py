"""The vector motion blur of include/raytrace_hip.h ("MOTION BLUR") restated in numpy: fp32 throughout, the header's order of operations,
vectorised over the image per tap.  The device (tests/test_motion_blur_gpu.py) and the kernel's per-pixel code compiled for the host
(tests/test_motion_blur.py) are compared with this bit for bit; a NaN on both sides counts as equal."""
import numpy as np

F32 = np.float32
DEFAULTS = dict(shutter=0.5, max_blur=16.0, taps=15, depth_softness=0.05)
TILE = 32
ZERO, HALF, ONE, TWO, THREE = F32(0.0), F32(0.5), F32(1.0), F32(2.0), F32(3.0)


def same_bits(a, b):
    """Elementwise: the same fp32 bit pattern, or a NaN on both sides."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def clamp01(r):
    return np.where(~(r > ZERO), ZERO, np.where(r > ONE, ONE, r))


def velocity(motion, shutter, max_blur):
    """(a): vx, vy, l per pixel, and which pixels the cap shortened."""
    s = F32(shutter) * HALF
    cap = F32(max_blur)
    vx, vy = motion[..., 0] * s, motion[..., 1] * s
    l2 = vx * vx + vy * vy
    still = ~(l2 < F32(np.inf))
    vx, vy = np.where(still, ZERO, vx), np.where(still, ZERO, vy)
    l = np.where(still, ZERO, np.sqrt(np.where(still, ZERO, l2)))
    over = l > cap
    k = cap / np.where(over, l, ONE)
    return np.where(over, vx * k, vx), np.where(over, vy * k, vy), np.where(over, cap, l), over


def tile_max(vx, vy, l):
    """(b): [tilesY, tilesX, 3] -- per tile the first pixel in row-major order of the greatest l, (0, 0, 0) where nothing moves."""
    H, W = l.shape
    out = np.zeros(((H + TILE - 1) // TILE, (W + TILE - 1) // TILE, 3), F32)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            box = (slice(ty * TILE, (ty + 1) * TILE), slice(tx * TILE, (tx + 1) * TILE))
            at = np.unravel_index(int(np.argmax(l[box])), l[box].shape)  # (argmax: the first of the greatest; l holds no NaN)
            if l[box][at] > ZERO:
                out[ty, tx] = (vx[box][at], vy[box][at], l[box][at])
    return out


def nb_max(tiles):
    """(c): per tile the greatest of its 3 x 3 neighbourhood, rows outer, columns inner, replaced only by a strictly greater l."""
    out = np.zeros_like(tiles)
    for ty in range(tiles.shape[0]):
        for tx in range(tiles.shape[1]):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    qy, qx = ty + dy, tx + dx
                    if 0 <= qy < tiles.shape[0] and 0 <= qx < tiles.shape[1] and tiles[qy, qx, 2] > out[ty, tx, 2]:
                        out[ty, tx] = tiles[qy, qx]
    return out


def blur(colour, motion, depth, shutter=DEFAULTS["shutter"], max_blur=DEFAULTS["max_blur"], taps=DEFAULTS["taps"],
         depth_softness=DEFAULTS["depth_softness"], with_parts=False):
    """out [H, W, 3] f32; with_parts: a dict with "out" and the intermediate results -- "l", "clamped" (a), "tile_max" (b), "nb_max"
    (c), "gathered" (which pixels take the gather arm of (d)), "taps" (how many taps each pixel summed)."""
    colour, motion, depth = (np.ascontiguousarray(a, F32) for a in (colour, motion, depth))
    H, W = depth.shape
    with np.errstate(all="ignore"):
        vx, vy, l, over = velocity(motion, shutter, max_blur)
        tiles = tile_max(vx, vy, l)
        nb = nb_max(tiles)
        y, x = np.indices((H, W))
        nx, ny, nl = (nb[y >> 5, x >> 5, c] for c in range(3))
        gathered = nl >= HALF
        lp = np.where(l < HALF, HALF, l)
        zp = depth
        wsum = ONE / lp
        total = colour * wsum[..., None]
        j = ((x & 1) * 2 + (y & 1) * 3) & 3
        jit = (j.astype(F32) - F32(1.5)) * F32(0.25)
        px, py = x.astype(F32) + HALF, y.astype(F32) + HALF
        soft, n, used = F32(depth_softness), F32(taps), np.zeros((H, W), np.int32)

        def sdc(a, b, e):
            return np.where(a == b, ONE, clamp01(ONE - (a - b) / e))

        def cone(d, length):
            return clamp01(ONE - d / length)

        def cyl(d, length):
            r = clamp01((d - F32(0.95) * length) / (F32(1.05) * length - F32(0.95) * length))
            return ONE - (r * r) * (THREE - TWO * r)

        for i in range(int(taps)):
            u = ((F32(i) + HALF) + jit) / n
            sg = u * TWO - ONE
            X, Y = px + nx * sg, py + ny * sg
            ok = (X >= ZERO) & (X < F32(W)) & (Y >= ZERO) & (Y < F32(H))
            qx, qy = np.where(ok, X, ZERO).astype(np.int32), np.where(ok, Y, ZERO).astype(np.int32)
            d = np.abs(sg) * nl
            lq = l[qy, qx]
            lq = np.where(lq < HALF, HALF, lq)
            zq = depth[qy, qx]
            e = soft * np.where(zp < zq, zp, zq)
            f, bk = sdc(zq, zp, e), sdc(zp, zq, e)
            w = (f * cone(d, lq) + bk * cone(d, lp)) + (cyl(d, lq) * cyl(d, lp)) * TWO
            wsum = np.where(ok, wsum + w, wsum)
            total = np.where(ok[..., None], total + colour[qy, qx] * w[..., None], total)
            used += ok & gathered
        out = np.where(gathered[..., None], total / wsum[..., None], colour)
    if not with_parts:
        return out
    return dict(out=out, l=l, clamped=over, tile_max=tiles, nb_max=nb, gathered=gathered, taps=used)
