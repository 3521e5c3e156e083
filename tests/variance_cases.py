"""Inputs shared by the variance-guided filter's tests (tests/test_variance.py shows on the oracle alone that they are not vacuous,
tests/test_variance_gpu.py runs them on the device): seeded synthetic fields for the moments accumulation -- temporal_cases.fields with a
moments history -- and for the estimate and the filter."""
import numpy as np

import temporal_cases as TC
import variance_oracle as VO

F32 = np.float32
SIZES = TC.SIZES  # (W, H): a single pixel; odd; no multiple of the 16 x 16 patch, wider than a tile, and with room for taps at h = 32
# What the filter fields must hold, as shares of their pixels (conditions on the inputs, checked by tests/test_variance.py): each arm of
# the estimate at the default spatialBelow, V^0 > 0, and C^K different from both the input and the result with V = +inf.
MIN_ARM, MIN_POSITIVE, MIN_CHANGED = 0.2, 0.5, 0.5
SPECIALS = ("NaN colour", "count 0", "count NaN", "count inf", "m2 < m1^2", "infinite m1", "infinite m2", "zero normal")


def moment_fields(W, H, seed=1):
    """temporal_cases.fields(W, H) with "moments" in the history: means of a luminance and of its square, and, sprinkled over them,
    m2 < m1^2, infinite and NaN moments."""
    colour, motion, prev_t, tri, hist = TC.fields(W, H, seed)
    rng = np.random.default_rng(2000 * seed + 7 * W + H)
    m1 = rng.random((H, W), dtype=F32)
    m2 = m1 * m1 + F32(0.05) * rng.random((H, W), dtype=F32)
    kind = rng.integers(0, 60, (H, W))
    m2[kind == 0] = F32(0.5) * m1[kind == 0] * m1[kind == 0]
    m2[kind == 1] = np.inf
    m1[kind == 2] = np.inf
    m1[kind == 3] = np.nan
    m1[kind == 4] = -np.inf
    return colour, motion, prev_t, tri, dict(hist, moments=np.stack([m1, m2], -1))


def special_pixels(W, H):
    """{name: (y, x)}: where the filter fields hold their specials; a few single pixels, far enough apart that most of the image never
    sees one (a NaN stalls the pixels whose taps reach it)."""
    if W * H == 1:
        return {}
    return {name: ((3 + 5 * i) % H, (7 + 11 * i) % W) for i, name in enumerate(SPECIALS)}


def filter_fields(W, H, seed=1):
    """dict(colour, normal, albedo, moments, count) for a W x H image: three surfaces with unnormalised normals, an albedo edge, a shading
    edge no guide sees, noise that grows downwards and shrinks with the history length, history lengths on both sides of the default
    spatialBelow, and the specials of special_pixels."""
    rng = np.random.default_rng(3000 * seed + 7 * W + H)
    ys, xs = np.mgrid[0:H, 0:W]
    albedo = np.where((xs < 0.6 * W)[..., None], F32([0.8, 0.7, 0.6]), F32([0.3, 0.4, 0.7])).astype(F32)
    albedo += F32(0.01) * rng.random((H, W, 3), dtype=F32)  # a texture within the albedo guide's reach
    normal = np.zeros((H, W, 3), F32)
    normal[...] = (0.0, 0.0, 1.0)
    normal[..., 0] += (0.1 * np.sin(xs / 9.0)).astype(F32)  # a curved back wall
    normal[xs < 0.3 * W] = (1.0, 0.0, 0.2)
    normal[ys > 0.7 * H] = (0.0, 1.0, 0.0)
    normal *= (0.5 + 1.5 * rng.random((H, W, 1))).astype(F32)  # sums over samples: not unit length
    shade = np.where(xs + ys < 0.4 * (W + H), 1.0, 0.45)  # a shadow edge inside the materials
    clean = albedo * shade[..., None].astype(F32)
    count = np.where(rng.random((H, W)) < 0.4, rng.integers(1, 4, (H, W)), 4.0 + 28.0 * rng.random((H, W))).astype(F32)
    sigma = (0.02 + 0.25 * ys / max(H, 1)) / np.sqrt(count)
    colour = (clean + sigma[..., None] * rng.standard_normal((H, W, 3))).astype(F32)
    m1 = (VO.lum(clean) + sigma * rng.standard_normal((H, W))).astype(F32)
    m2 = (m1 * m1 + (sigma * sigma * count * (0.5 + rng.random((H, W)))).astype(F32)).astype(F32)
    sp = special_pixels(W, H)
    for name, (y, x) in sp.items():
        if name == "NaN colour":
            colour[y, x] = np.nan
        elif name == "count 0":
            count[y, x] = 0.0
        elif name == "count NaN":
            count[y, x] = np.nan
        elif name == "count inf":
            count[y, x] = np.inf
        elif name == "m2 < m1^2":
            m2[y, x] = F32(0.5) * m1[y, x] * m1[y, x]
        elif name == "infinite m1":
            m1[y, x] = np.inf
        elif name == "infinite m2":
            m2[y, x] = np.inf
        elif name == "zero normal":
            normal[y, x] = 0.0
    return dict(colour=colour, normal=normal, albedo=albedo, moments=np.stack([m1, m2], -1), count=count)


def shares(f, **params):
    """(spatial arm, temporal arm, V^0 > 0, C^K differs from the input and from the V = +inf result) as shares of the pixels."""
    p = dict(VO.DEFAULTS, **params)
    v0, spatial = VO.estimate(f["colour"], f["normal"], f["albedo"], f["moments"], f["count"], p["albedo_inv_sigma2"], p["normal_power_log2"],
                              p["spatial_below"], with_arm=True)
    rest = {k: p[k] for k in ("iterations", "luminance_sigma2", "variance_floor", "albedo_inv_sigma2", "normal_power_log2")}
    out, _ = VO.iterate(f["colour"], v0, f["normal"], f["albedo"], **rest)
    flat, _ = VO.iterate(f["colour"], np.full_like(v0, np.inf), f["normal"], f["albedo"], **rest)
    differs = lambda a, b: (~VO.same_bits(a, b)).any(-1)  # noqa: E731
    return float(spatial.mean()), float((~spatial).mean()), float((v0 > 0).mean()), float((differs(out, f["colour"]) & differs(out, flat)).mean())
