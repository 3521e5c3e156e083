"""The temporal accumulation of include/raytrace_hip.h ("TEMPORAL ACCUMULATION") restated in numpy float32: the four taps in the header's
order, vectorised over pixels.  Every operation is an IEEE fp32 + - * /, floor, abs or compare, so the device output must equal this bit
for bit (up to the payload of a NaN).

Skipped and refused taps are masked with np.where on clipped indices, never by multiplying by 0 (adding +0 to a sum is exact; 0 * inf is
not)."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
DEFAULTS = dict(max_history=32.0, depth_tolerance=0.05)


def _arr(a, dtype, shape, name):
    a = np.asarray(a)
    if dtype == np.uint32 and a.dtype == np.int32:
        a = a.view(np.uint32)
    assert a.dtype == dtype and a.shape == shape, f"{name}: expected {np.dtype(dtype).name} {shape}, got {a.dtype} {a.shape}"
    return a


def empty_history(H, W):
    """A history that holds nothing: count 0 everywhere."""
    return dict(colour=np.zeros((H, W, 3), F), count=np.zeros((H, W), F), t=np.zeros((H, W), F), triangle=np.zeros((H, W), np.uint32))


def accumulate(colour, motion, prev_t, triangle, history, max_history=DEFAULTS["max_history"], depth_tolerance=DEFAULTS["depth_tolerance"],
               with_taps=False):
    """{"colour" [H, W, 3] f32, "count" [H, W] f32}; with_taps: also "taps" [H, W] u8, the number of accepted taps, "inside" [H, W] u8,
    the number of taps that lie inside the image (0 where the range test fails), "live" [H, W] u8, those of them whose history count is
    >= 1 (live - taps: refused by the triangle or depth test), and "used" [H, W] bool: the history was blended in (false: the pixel
    starts again)."""
    H, W, _ = np.shape(colour)
    c = _arr(colour, F, (H, W, 3), "colour")
    m = _arr(motion, F, (H, W, 2), "motion")
    pt = _arr(prev_t, F, (H, W), "prev_t")
    tri = _arr(triangle, np.uint32, (H, W), "triangle")
    hc = _arr(history["colour"], F, (H, W, 3), "history colour")
    hn = _arr(history["count"], F, (H, W), "history count")
    ht = _arr(history["t"], F, (H, W), "history t")
    htri = _arr(history["triangle"], np.uint32, (H, W), "history triangle")
    maxh, tol = F(max_history), F(depth_tolerance)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        gx = ((xs.astype(F) + F(0.5)) + m[..., 0]) - F(0.5)
        gy = ((ys.astype(F) + F(0.5)) + m[..., 1]) - F(0.5)
        ok = (pt > 0) & (gx >= F(-1.0)) & (gx < F(W)) & (gy >= F(-1.0)) & (gy < F(H))
        gxs, gys = np.where(ok, gx, F(0)), np.where(ok, gy, F(0))  # (only so that the conversions below are defined; masked by ok later)
        x0f, y0f = np.floor(gxs), np.floor(gys)
        ax, ay = gxs - x0f, gys - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        sw = np.zeros((H, W), F)
        s = np.zeros((H, W, 3), F)
        sn = np.zeros((H, W), F)
        taps = np.zeros((H, W), np.uint8)
        inside_taps = np.zeros((H, W), np.uint8)
        live_taps = np.zeros((H, W), np.uint8)
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
                taps += accept
                inside_taps += inside
                live_taps += inside & (qn >= F(1.0))
        use = ok & (sw > 0)
        den = np.where(use, sw, F(1))
        h = s / den[..., None]
        n = sn / den + F(1.0)
        n = np.where(n > maxh, maxh, n)
        a = F(1.0) / n
        blended = h + (c - h) * a[..., None]
        out = dict(colour=np.where((use & (n != F(1.0)))[..., None], blended, c).astype(F), count=np.where(use, n, F(1.0)).astype(F))
    assert out["colour"].dtype == F and blended.dtype == F and b.dtype == F
    if with_taps:
        out["taps"], out["inside"], out["live"], out["used"] = taps, inside_taps, live_taps, use
    return out


def next_history(out, t, triangle):
    """The history the next call reads: this call's outputs and this frame's t and triangle maps."""
    return dict(colour=out["colour"], count=out["count"], t=np.asarray(t, F), triangle=np.asarray(triangle).view(np.uint32))


def same_bits(got, want):
    """Element-wise: equal bit patterns, or a NaN on both sides."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype == np.uint32 or got.dtype == np.int32:
        return got.view(np.uint32) == want.view(np.uint32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
