"""The variance-guided filter of include/raytrace_hip.h ("VARIANCE-GUIDED FILTER") restated in numpy float32: (a) the moments accumulation,
(b) the variance estimate, (c) the guided iterations, every loop in the header's order, vectorised over pixels.  Every operation is an IEEE
fp32 + - * /, floor, abs, sqrt (guides) or compare, so the device output must equal this bit for bit (up to the payload of a NaN).

Skipped and refused taps are masked with np.where on clipped indices, never by multiplying by 0 (adding +0 to a sum is exact; 0 * inf is
not)."""
import numpy as np

import denoise_oracle as DO
import temporal_oracle as TO

F = np.float32
B = DO.B
G = np.array([1 / 4, 1 / 2, 1 / 4], np.float32)
DEFAULTS = dict(iterations=4, luminance_sigma2=4.0, variance_floor=1e-8, albedo_inv_sigma2=100.0, normal_power_log2=7, spatial_below=4.0)
same_bits = TO.same_bits


def lum(c):
    """(0.2126f*r + 0.7152f*g) + 0.0722f*b"""
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def variance_of(m1, m2):
    """v = m2 - m1*m1; v > 0 ? v : 0 (a NaN gives 0)."""
    with np.errstate(all="ignore"):
        v = m2 - m1 * m1
        return np.where(v > 0, v, F(0)).astype(F)


def empty_history(H, W):
    """A history that holds nothing: count 0 everywhere."""
    return dict(TO.empty_history(H, W), moments=np.zeros((H, W, 2), F))


def accumulate(colour, motion, prev_t, triangle, history, max_history=TO.DEFAULTS["max_history"],
               depth_tolerance=TO.DEFAULTS["depth_tolerance"]):
    """(a): {"colour" [H, W, 3], "count" [H, W], "moments" [H, W, 2], "variance" [H, W]}, all f32.  The colour and count arithmetic is
    TEMPORAL ACCUMULATION's, restated here with the moments on the same taps."""
    H, W, _ = np.shape(colour)
    c = TO._arr(colour, F, (H, W, 3), "colour")
    m = TO._arr(motion, F, (H, W, 2), "motion")
    pt = TO._arr(prev_t, F, (H, W), "prev_t")
    tri = TO._arr(triangle, np.uint32, (H, W), "triangle")
    hc = TO._arr(history["colour"], F, (H, W, 3), "history colour")
    hn = TO._arr(history["count"], F, (H, W), "history count")
    ht = TO._arr(history["t"], F, (H, W), "history t")
    htri = TO._arr(history["triangle"], np.uint32, (H, W), "history triangle")
    hm = TO._arr(history["moments"], F, (H, W, 2), "history moments")
    maxh, tol = F(max_history), F(depth_tolerance)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        l = lum(c)
        l2 = l * l
        cur = np.stack([l, l2], -1)
        gx = ((xs.astype(F) + F(0.5)) + m[..., 0]) - F(0.5)
        gy = ((ys.astype(F) + F(0.5)) + m[..., 1]) - F(0.5)
        ok = (pt > 0) & (gx >= F(-1.0)) & (gx < F(W)) & (gy >= F(-1.0)) & (gy < F(H))
        gxs, gys = np.where(ok, gx, F(0)), np.where(ok, gy, F(0))
        x0f, y0f = np.floor(gxs), np.floor(gys)
        ax, ay = gxs - x0f, gys - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        sw = np.zeros((H, W), F)
        s = np.zeros((H, W, 3), F)
        sn = np.zeros((H, W), F)
        sm = np.zeros((H, W, 2), F)
        limit = tol * pt
        for j in range(2):
            qy = y0 + j
            for k in range(2):
                qx = x0 + k
                inside = ok & (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                b = (ax if k else F(1.0) - ax) * (ay if j else F(1.0) - ay)
                qn, qt = hn[cy, cx], ht[cy, cx]
                accept = inside & (qn >= F(1.0)) & (htri[cy, cx] == tri) & ((qt == pt) | (np.abs(qt - pt) <= limit))
                sw = np.where(accept, sw + b, sw)
                s = np.where(accept[..., None], s + b[..., None] * hc[cy, cx], s)
                sn = np.where(accept, sn + b * qn, sn)
                sm = np.where(accept[..., None], sm + b[..., None] * hm[cy, cx], sm)
        use = ok & (sw > 0)
        den = np.where(use, sw, F(1))
        h = s / den[..., None]
        hmom = sm / den[..., None]
        n = sn / den + F(1.0)
        n = np.where(n > maxh, maxh, n)
        a = F(1.0) / n
        blend = (use & (n != F(1.0)))[..., None]
        out = dict(colour=np.where(blend, h + (c - h) * a[..., None], c).astype(F), count=np.where(use, n, F(1.0)).astype(F),
                   moments=np.where(blend, hmom + (cur - hmom) * a[..., None], cur).astype(F))
    out["variance"] = variance_of(out["moments"][..., 0], out["moments"][..., 1])
    assert all(v.dtype == F for v in out.values()) and hmom.dtype == F and b.dtype == F
    return out


def next_history(out, t, triangle):
    """The history the next call reads: this call's outputs and this frame's t and triangle maps."""
    return dict(TO.next_history(out, t, triangle), moments=out["moments"])


def _weights(nh, z, a, nq, zq, aq, E):
    """(wn, da) of the DENOISER block, per pixel against its tap."""
    e = a - aq
    da = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    dot = (nh[..., 0] * nq[..., 0] + nh[..., 1] * nq[..., 1]) + nh[..., 2] * nq[..., 2]
    dot = np.where(dot > 0, dot, F(0))
    for _ in range(E):
        dot = dot * dot
    return np.where(z & zq, F(1), dot), da


def estimate(colour, normal, albedo, moments=None, count=None, albedo_inv_sigma2=DEFAULTS["albedo_inv_sigma2"],
             normal_power_log2=DEFAULTS["normal_power_log2"], spatial_below=DEFAULTS["spatial_below"], with_arm=False):
    """(b): V^0 [H, W] f32; with_arm: (V^0, spatial [H, W] bool, the pixels that took the 7x7 window)."""
    c = DO._f32(colour, "colour")
    a = DO._f32(albedo, "albedo")
    H, W, _ = c.shape
    assert (moments is None) == (count is None), "moments and count: both or neither"
    with np.errstate(all="ignore"):
        if moments is None:
            l = lum(c)
            mom, cnt = np.stack([l, l * l], -1), np.ones((H, W), F)
        else:
            mom, cnt = TO._arr(moments, F, (H, W, 2), "moments"), TO._arr(count, F, (H, W), "count")
        nh, z = DO.guides(normal)
        ia, sb = F(albedo_inv_sigma2), F(spatial_below)
        temporal = cnt >= sb
        ys, xs = np.mgrid[0:H, 0:W]
        sw = np.zeros((H, W), F)
        s = np.zeros((H, W, 2), F)
        for dy in range(-3, 4):
            qy = ys + dy
            for dx in range(-3, 4):
                qx = xs + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                wn, da = _weights(nh, z, a, nh[cy, cx], z[cy, cx], a[cy, cx], normal_power_log2)
                w = wn / (F(1) + da * ia)
                sw = np.where(inside, sw + w, sw)
                s = np.where(inside[..., None], s + w[..., None] * mom[cy, cx], s)
        pos = sw > 0
        M = s / np.where(pos, sw, F(1))[..., None]
        v = variance_of(M[..., 0], M[..., 1])
        spatial = np.where(pos, v * np.where(cnt >= F(1.0), F(4.0) / cnt, F(4.0)), F(0))
        v0 = np.where(temporal, variance_of(mom[..., 0], mom[..., 1]), spatial).astype(F)
    assert v0.dtype == F and w.dtype == F and M.dtype == F
    return (v0, ~temporal) if with_arm else v0


def iterate(colour, variance, normal, albedo, iterations=DEFAULTS["iterations"], luminance_sigma2=DEFAULTS["luminance_sigma2"],
            variance_floor=DEFAULTS["variance_floor"], albedo_inv_sigma2=DEFAULTS["albedo_inv_sigma2"],
            normal_power_log2=DEFAULTS["normal_power_log2"]):
    """(c): (C^K [H, W, 3], V^K [H, W]) from (C^0, V^0)."""
    c = DO._f32(colour, "colour").copy()
    v = DO._f32(variance, "variance").copy()
    a = DO._f32(albedo, "albedo")
    H, W, _ = c.shape
    nh, z = DO.guides(normal)
    ls, fl, ia = F(luminance_sigma2), F(variance_floor), F(albedo_inv_sigma2)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        for i in range(iterations):
            h = 1 << i
            gs, gw = np.zeros((H, W), F), np.zeros((H, W), F)
            for j in range(3):
                qy = ys + j - 1
                for k in range(3):
                    qx = xs + k - 1
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    gs = np.where(inside, gs + (G[j] * G[k]) * v[cy, cx], gs)
                    gw = np.where(inside, gw + G[j] * G[k], gw)
            il = F(1.0) / (ls * (gs / gw) + fl)
            lp = lum(c)
            sw = np.zeros((H, W), F)
            s = np.zeros((H, W, 3), F)
            sv = np.zeros((H, W), F)
            for j in range(5):
                qy = ys + (j - 2) * h
                for k in range(5):
                    qx = xs + (k - 2) * h
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    cq = c[cy, cx]
                    wn, da = _weights(nh, z, a, nh[cy, cx], z[cy, cx], a[cy, cx], normal_power_log2)
                    dl = lp - lum(cq)
                    w = ((B[j] * B[k]) * wn) / ((F(1) + (dl * dl) * il) * (F(1) + da * ia))
                    sw = np.where(inside, sw + w, sw)
                    s = np.where(inside[..., None], s + w[..., None] * cq, s)
                    sv = np.where(inside, sv + (w * w) * v[cy, cx], sv)
            pos = sw > 0
            den = np.where(pos, sw, F(1))
            c = np.where(pos[..., None], s / den[..., None], c)
            v = np.where(pos, sv / (den * den), v)
            assert c.dtype == F and v.dtype == F and il.dtype == F and w.dtype == F
    return c, v


def denoise(colour, normal, albedo, moments=None, count=None, **params):
    """(b) then (c): (C^K, V^K).  Keywords as DEFAULTS."""
    p = dict(DEFAULTS, **params)
    v0 = estimate(colour, normal, albedo, moments, count, p["albedo_inv_sigma2"], p["normal_power_log2"], p["spatial_below"])
    return iterate(colour, v0, normal, albedo, p["iterations"], p["luminance_sigma2"], p["variance_floor"], p["albedo_inv_sigma2"],
                   p["normal_power_log2"])
