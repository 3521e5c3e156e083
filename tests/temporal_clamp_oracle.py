"""The clamped temporal accumulation of include/raytrace_hip.h ("TEMPORAL CLAMP") restated in numpy float32: the whole pixel --
TEMPORAL ACCUMULATION's four taps in the header's order (restated here, as variance_oracle.py restates them), the 3x3 colour box of the
current frame, the clamp, the blend -- with and without the luminance moments of VARIANCE-GUIDED FILTER (a), vectorised over pixels.  Every
operation is an IEEE fp32 + - * /, floor, abs, sqrt or compare, so the device output must equal this bit for bit (up to the payload of a
NaN).

Skipped and refused taps are masked with np.where on clipped indices, never by multiplying by 0."""
import numpy as np

import temporal_oracle as TO
import variance_oracle as VO

F = np.float32
MINMAX, VARIANCE, BOTH = 1, 2, 3
DEFAULTS = dict(mode=BOTH, gamma=1.0)
same_bits = TO.same_bits


def box(colour, mode=DEFAULTS["mode"], gamma=DEFAULTS["gamma"]):
    """(lo, hi), [H, W, 3] f32 each: per pixel and channel the box of the 3x3 neighbourhood, taps dy = -1..1 outer, dx = -1..1 inner,
    those outside the image skipped."""
    assert mode in (MINMAX, VARIANCE, BOTH), mode
    H, W, _ = np.shape(colour)
    c = TO._arr(colour, F, (H, W, 3), "colour")
    g = F(gamma)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        cnt = np.zeros((H, W), F)
        s1, s2 = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
        mn, mx = np.full((H, W, 3), np.inf, F), np.full((H, W, 3), -np.inf, F)
        for dy in (-1, 0, 1):
            qy = ys + dy
            for dx in (-1, 0, 1):
                qx = xs + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                v = c[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
                m = inside[..., None]
                cnt = cnt + inside.astype(F)  # (small whole numbers: exact)
                s1 = np.where(m, s1 + v, s1)
                s2 = np.where(m, s2 + v * v, s2)
                mn = np.where(m & (v < mn), v, mn)
                mx = np.where(m & (v > mx), v, mx)
        mu, ex2 = s1 / cnt[..., None], s2 / cnt[..., None]
        var = ex2 - mu * mu
        var = np.where(var > 0, var, F(0))
        e = g * np.sqrt(var)
        if mode == MINMAX:
            lo, hi = mn, mx
        elif mode == VARIANCE:
            lo, hi = mu - e, mu + e
        else:
            lo, hi = np.where(mu - e > mn, mu - e, mn), np.where(mu + e < mx, mu + e, mx)
    assert lo.dtype == F and hi.dtype == F and e.dtype == F and cnt.dtype == F
    return lo, hi


def accumulate(colour, motion, prev_t, triangle, history, max_history=TO.DEFAULTS["max_history"],
               depth_tolerance=TO.DEFAULTS["depth_tolerance"], mode=DEFAULTS["mode"], gamma=DEFAULTS["gamma"]):
    """{"colour" [H, W, 3] f32, "count" [H, W] f32, "used" [H, W] bool: the history was blended in (so the clamp ran), "moved" [H, W, 3] f32:
    how far the clamp moved each channel of the history colour, clamped minus fetched, 0 where it did not (or did not run)}; with
    "moments" in the history also "moments" [H, W, 2] f32 and "variance" [H, W] f32, accumulated from the unclamped taps."""
    H, W, _ = np.shape(colour)
    c = TO._arr(colour, F, (H, W, 3), "colour")
    m = TO._arr(motion, F, (H, W, 2), "motion")
    pt = TO._arr(prev_t, F, (H, W), "prev_t")
    tri = TO._arr(triangle, np.uint32, (H, W), "triangle")
    hc = TO._arr(history["colour"], F, (H, W, 3), "history colour")
    hn = TO._arr(history["count"], F, (H, W), "history count")
    ht = TO._arr(history["t"], F, (H, W), "history t")
    htri = TO._arr(history["triangle"], np.uint32, (H, W), "history triangle")
    with_moments = "moments" in history
    hm = TO._arr(history["moments"], F, (H, W, 2), "history moments") if with_moments else np.zeros((H, W, 2), F)
    maxh, tol = F(max_history), F(depth_tolerance)
    lo, hi = box(c, mode, gamma)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        l = VO.lum(c)
        cur = np.stack([l, l * l], -1)
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
        fetched = s / den[..., None]
        hmom = sm / den[..., None]
        n = sn / den + F(1.0)
        n = np.where(n > maxh, maxh, n)
        a = F(1.0) / n
        blend = (use & (n != F(1.0)))[..., None]
        h = np.where(fetched < lo, lo, fetched)  # the clamp, in the header's order
        h = np.where(h > hi, hi, h)
        pulled = blend & ~same_bits(h, fetched)
        out = dict(colour=np.where(blend, h + (c - h) * a[..., None], c).astype(F), count=np.where(use, n, F(1.0)).astype(F),
                   used=blend[..., 0], moved=np.where(pulled, h - fetched, F(0)).astype(F))
        if with_moments:
            out["moments"] = np.where(blend, hmom + (cur - hmom) * a[..., None], cur).astype(F)
            out["variance"] = VO.variance_of(out["moments"][..., 0], out["moments"][..., 1])
    assert all(v.dtype == F for k, v in out.items() if k != "used") and h.dtype == F and b.dtype == F
    return out


def next_history(out, t, triangle):
    """The history the next call reads: this call's outputs (its moments, if it has them) and this frame's t and triangle maps."""
    hist = TO.next_history(out, t, triangle)
    if "moments" in out:
        hist["moments"] = out["moments"]
    return hist


def outside_minmax(accumulated, frame):
    """[H, W] bool: a channel of `accumulated` lies outside the 3x3 min/max box of `frame` (a NaN lies in no box and is not counted)."""
    lo, hi = box(frame, MINMAX)
    with np.errstate(all="ignore"):
        return ((accumulated < lo) | (accumulated > hi)).any(-1)
