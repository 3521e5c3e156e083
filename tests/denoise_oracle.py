"""The denoiser of include/raytrace_hip.h ("DENOISER") restated in numpy float32: the taps in the header's order, vectorised over pixels.
Every operation is an IEEE fp32 + - * /, sqrt or compare, so the device output must equal this bit for bit.

Skipped taps are masked with np.where on clipped indices, never by multiplying by 0 (adding +0 to a sum is exact; 0 * inf is not)."""
import numpy as np

F = np.float32
B = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)


def _f32(a, name):
    a = np.asarray(a)
    assert a.dtype == np.float32, f"{name}: expected float32, got {a.dtype}"
    return a


def guides(normal):
    """n^ [H, W, 3] and z [H, W]: m = (nx*nx + ny*ny) + nz*nz; m > 0: n / sqrt(m), else (0, 0, 0) and z."""
    n = _f32(normal, "normal")
    m = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
    ok = m > 0
    with np.errstate(all="ignore"):
        r = np.sqrt(np.where(ok, m, F(1)))
        nh = np.where(ok[..., None], n / r[..., None], F(0))
    return _f32(nh, "n^"), ~ok


def denoise(colour, normal, albedo, iterations=4, colour_inv_sigma2=4.0, albedo_inv_sigma2=100.0, normal_power_log2=7):
    """C^K for [H, W, 3] float32 colour, normal and albedo."""
    c = _f32(colour, "colour").copy()
    a = _f32(albedo, "albedo")
    H, W, _ = c.shape
    nh, z = guides(normal)
    ic, ia = F(colour_inv_sigma2), F(albedo_inv_sigma2)
    ys, xs = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        for i in range(iterations):
            h = 1 << i
            sw = np.zeros((H, W), np.float32)
            s = np.zeros((H, W, 3), np.float32)
            for j in range(5):
                qy = ys + (j - 2) * h
                for k in range(5):
                    qx = xs + (k - 2) * h
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    cy, cx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    cq, nq, aq, zq = c[cy, cx], nh[cy, cx], a[cy, cx], z[cy, cx]
                    d = c - cq
                    dc = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    e = a - aq
                    da = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                    dot = (nh[..., 0] * nq[..., 0] + nh[..., 1] * nq[..., 1]) + nh[..., 2] * nq[..., 2]
                    dot = np.where(dot > 0, dot, F(0))
                    for _ in range(normal_power_log2):
                        dot = dot * dot
                    wn = np.where(z & zq, F(1), dot)
                    w = ((B[j] * B[k]) * wn) / ((F(1) + dc * ic) * (F(1) + da * ia))
                    sw = np.where(inside, sw + w, sw)
                    s = np.where(inside[..., None], s + w[..., None] * cq, s)
            c = np.where((sw > 0)[..., None], s / sw[..., None], c)
            _f32(c, f"C^{i + 1}")
            ic = ic * F(4)
    return c


def quantise(colour):
    """u16 planes R, G, B of C^K: v = C * 65535; !(v > 0) -> 0, v >= 65534.5 -> 65535, else (u16)(v + 0.5)."""
    v = _f32(colour, "colour") * F(65535.0)
    with np.errstate(invalid="ignore"):
        u = np.where(~(v > 0), F(0), np.where(v >= F(65534.5), F(65535), np.trunc(v + F(0.5))))
    return [u[..., ch].astype(np.uint16) for ch in range(3)]


def inputs(sc_planes, normal, albedo):
    """What rtHipSceneDenoise gathers, from the host read-backs: u16 planes ([H, W] each) / 65535 and the normal / albedo means."""
    colour = np.stack([np.asarray(p, np.uint16) for p in sc_planes], -1).astype(np.float32) / F(65535.0)
    return colour, _f32(normal, "normal"), _f32(albedo, "albedo")
