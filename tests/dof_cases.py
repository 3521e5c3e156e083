"""Shapes, synthetic fields, the parameter grid and the measured bounds of the depth-of-field tests (tests/test_dof.py runs the kernel's
per-pixel code on the host and shows on the oracle alone that the inputs are not vacuous; tests/test_dof_gpu.py runs the same cases on the
device).  Oracle results are computed once per case and shared (reference()); nobody changes them."""
import functools
import itertools

import numpy as np

import dof_oracle as DO

F32 = np.float32
DENORMAL = float(np.nextafter(F32(0), F32(1)))  # the smallest denormal, 1.4e-45
# (W, H): one pixel; one column; one row; a partial 8-row block and a partial tile; two tiles each way, the second one pixel wide; two tiles
# by two with a partial one
SHAPES = ((1, 1), (1, 7), (7, 1), (31, 9), (33, 33), (64, 40))
# seven tile columns: wide enough for tiles whose whole neighbourhood is in focus beside tiles that are not, so that `split` runs the copy
# arm and the gather arm in ONE launch
WIDE = (200, 40)
# 4 x 3 tiles: tiles (1, 1) and (2, 1) have all eight neighbours, so (c) takes a maximum over a full 3 x 3 and a tile has one above AND below
INTERIOR = (97, 70)
# 1 x 257 tiles: the second workgroup of (c) (one lane per tile, 256 lanes) and block indices of (d) far past the first tile row.  W = 2,
# so the numpy oracle stays cheap (16 400 pixels); it runs the ORDINARY settings only (grid_of)
TALL = (2, 8200)
FOCUS = 4.0  # what the fields call "in focus"
FIELDS = ("focus", "constant", "near_sharp", "near_blurred", "ramp", "misses", "specials", "bright", "layers", "split")
CASES = (tuple(("ramp", W, H) for W, H in SHAPES + (WIDE,)) + tuple(("layers", W, H) for W, H in ((31, 9), (33, 33), (64, 40), WIDE))
         + tuple((f, W, H) for f in ("focus", "near_sharp", "misses", "specials", "bright") for W, H in ((33, 33), (64, 40)))
         + tuple((f, W, H) for f in ("constant", "near_blurred") for W, H in ((31, 9), (64, 40))) + (("split",) + WIDE,)
         + tuple((f,) + INTERIOR for f in ("layers", "near_sharp")) + tuple((f,) + TALL for f in ("ramp", "layers")))

# The grid: the issue's extremes as a full product, and ordinary settings (every ring count; a cap of one pixel; a wide cap with a hard
# depth test; an odd cap).  cocScale 0 and the smallest denormal copy the frame except where a depth makes `a` infinite.
EXTREMES = tuple(dict(rings=r, max_coc=m, coc_scale=c, focus=f, depth_softness=s)
                 for r, m, c, f, s in itertools.product(range(1, 7), (1.0, 32.0), (0.0, DENORMAL, 4096.0), (DENORMAL, 3e38), (0.0, 3e38)))
ORDINARY = (tuple(dict(rings=r, max_coc=16.0, coc_scale=8.0, focus=FOCUS, depth_softness=0.05) for r in range(1, 7))
            + (dict(rings=3, max_coc=32.0, coc_scale=24.0, focus=FOCUS, depth_softness=0.0),
               dict(rings=2, max_coc=1.0, coc_scale=3.0, focus=FOCUS, depth_softness=0.05),
               dict(rings=4, max_coc=7.5, coc_scale=12.0, focus=2.5, depth_softness=0.5)))
GRID = ORDINARY + EXTREMES
DEFAULT_LIKE = ORDINARY[2]  # rings 3, maxCoc 16, cocScale 8, focus FOCUS, depthSoftness 0.05


def grid_of(W, H):
    """The settings a case of W x H runs: the whole GRID, the ORDINARY ones alone at the tall shape."""
    return ORDINARY if (W, H) == TALL else GRID


# Scene path (tests/test_dof_gpu.py, and the dof steps of tests/session_cases.py): a moderate blur, and the widest one with a hard depth
# test; the focus is the median depth of the frame's hits
SCENE_PARAMS = (dict(coc_scale=12.0, max_coc=8.0, rings=3), dict(coc_scale=40.0, max_coc=32.0, rings=6, depth_softness=0.0))

# Non-vacuity (test_dof.py asserts it on the oracle's intermediate results): `split` at 200 x 40 puts at least this share of its pixels
# into each arm under DEFAULT_LIKE.  Measured: copy 0.320 (tile columns 0 and 1: column 2 neighbours column 3, which the boundary
# x = 100 cuts), gather 0.680.
MIN_COPY, MIN_GATHER = 0.20, 0.20
SPLIT_SHARES = (0.320, 0.680)

# A constant finite colour (0.3, 0.55, 0.8125) under every field but `specials` at the shapes (33, 33), (64, 40) and WIDE and every
# ORDINARY setting and every EXTREMES setting with cocScale 4096: the oracle's greatest |out - colour| was 45 ulp of the colour
# (`near_sharp` 33 x 33, rings 6, maxCoc 16, cocScale 8, focus 4, depthSoftness 0.05) -> 180 ulp allowed, four times that, as the
# motion blur's test does.  (No weight is negative, so nothing cancels, but the weights of one pixel span 1 / 0.25 .. 1 / 256: sum and
# wsum are sums of at most 169 terms of very different size with a rounding each.)
CONSTANT_COLOUR_MEASURED_ULP = 45
CONSTANT_COLOUR_ULP = 4 * CONSTANT_COLOUR_MEASURED_ULP


def _layers(rng, W, H):
    """Depths in 8 x 8 blocks drawn from a near layer, one within 5 % of the focus, the focus, a far one and the background."""
    pick = rng.integers(0, 5, ((H + 7) // 8, (W + 7) // 8))
    z = np.asarray([1.0, FOCUS * 1.03, FOCUS, 25.0, np.inf], F32)[pick]
    return np.ascontiguousarray(np.repeat(np.repeat(z, 8, 0), 8, 1)[:H, :W])


@functools.lru_cache(maxsize=None)
def fields(name, W, H, seed=17):
    """(colour [H, W, 3], depth [H, W]) of field `name`, read-only."""
    rng = np.random.default_rng([seed, W, H, FIELDS.index(name)])
    colour = rng.random((H, W, 3), dtype=F32)
    depth = np.full((H, W), FOCUS, F32)
    y, x = np.indices((H, W))
    if name == "focus":  # everything in focus: a copy
        pass
    elif name == "constant":  # a constant colour under a uniform defocus
        colour[...] = (0.3, 0.55, 0.8125)
        depth[...] = 2 * FOCUS
    elif name == "near_sharp":  # a sharp near object (a disc in focus) in front of a defocused far plane
        depth[...] = 40.0
        depth[(x - W // 2) ** 2 + (y - H // 2) ** 2 <= (min(W, H) // 3) ** 2] = FOCUS
    elif name == "near_blurred":  # a defocused near object (a bar) in front of a sharp plane
        depth[:, W // 3:2 * W // 3 + 1] = 1.0
    elif name == "ramp":  # depths through the focus: FOCUS / 4 .. 4 FOCUS from left to right, tilted a little from top to bottom
        u = (x.astype(F32) + F32(0.25) * y.astype(F32)) / F32(max(W + 0.25 * H - 1, 1))
        depth = (F32(FOCUS / 4) * np.exp2(F32(4) * u)).astype(F32)
    elif name == "misses":  # misses (+inf) beside hits, in 5 x 3 blocks
        depth = np.where(((x // 5) + (y // 3)) % 3 == 0, F32(np.inf), F32(FOCUS) + F32(0.5) * (x % 7).astype(F32)).astype(F32)
    elif name == "specials":
        depth = _layers(rng, W, H)
        flat_z, flat_c = depth.reshape(-1), colour.reshape(-1, 3)
        odd_z = [np.nan, 0.0, -1.0, -np.inf, DENORMAL, 3e38, -0.0, np.inf]
        odd_c = [np.nan, 3e38, -3e38, np.inf]
        for k, at in enumerate(rng.choice(W * H, min(160, W * H), replace=False)):
            if k % 2 == 0:
                flat_z[at] = odd_z[(k // 2) % len(odd_z)]
            else:
                flat_c[at, (k // 2) % 3 if k % 4 == 1 else slice(None)] = odd_c[(k // 4) % len(odd_c)]
    elif name == "bright":  # an isolated bright pixel on black under a uniform defocus: its footprint is the octagon
        colour[...] = 0
        colour[H // 2, W // 2] = (1000.0, 500.0, 250.0)
        depth[...] = 2 * FOCUS
    elif name == "layers":
        depth = _layers(rng, W, H)
    elif name == "split":  # the left half in focus, the right half far behind it
        depth = np.where(x >= W // 2, F32(40.0), F32(FOCUS)).astype(F32)
    else:
        raise KeyError(name)
    out = (colour, np.ascontiguousarray(depth, F32))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, W, H, params):
    out = DO.blur(*fields(name, W, H), **dict(params))
    out.setflags(write=False)
    return out


def reference(name, W, H, params):
    """The oracle's output for a case under `params` (a dict of GRID), computed once."""
    return _reference(name, W, H, tuple(sorted(params.items())))


def shares(parts):
    """(copy share, gather share) of an oracle result with_parts."""
    g = float(parts["gathered"].mean())
    return 1.0 - g, g


# Degenerate cameras the lens helper refuses, and ordinary ones (eye_to_top_left, left_to_right, top_to_bottom).
LENS_CAMERAS = dict(
    soup=((-0.5, 0.28125, 1.0), (1.0 / 1920, 0.0, 0.0), (0.0, -1.0 / 1920, 0.0)),
    oblique=((-0.37, 0.61, 2.3), (0.0031, 0.0002, -0.0011), (0.0004, -0.0032, 0.0005)),
    behind=((0.4, -0.3, -1.5), (0.002, 0.0, 0.0), (0.0, -0.002, 0.0)),
)
LENS_DEGENERATE = dict(
    zero_pitch=((-0.5, 0.3, 1.0), (0.0, 0.0, 0.0), (0.0, -0.001, 0.0)),
    parallel=((-0.5, 0.3, 1.0), (0.001, 0.0, 0.0), (0.002, 0.0, 0.0)),  # the pixel vectors span no plane
    in_plane=((0.5, 0.3, 0.0), (0.001, 0.0, 0.0), (0.0, -0.001, 0.0)),  # the eye lies in the image plane
    nan=((-0.5, np.nan, 1.0), (0.001, 0.0, 0.0), (0.0, -0.001, 0.0)),
    inf=((-0.5, 0.3, 1.0), (np.inf, 0.0, 0.0), (0.0, -0.001, 0.0)),
)
LENS_SETTINGS = ((0.01, 4.0), (0.0, 1.0), (0.05, 0.25), (1e-3, 3e38), (2.0, 1.0), (1e-30, 1e-30), (100.0, 1.0), (0.01, 1e-46))  # (the last two: refused)


def camera_dict(vectors):
    tl, lr, tb = (np.asarray(tuple(v) + (0.0,), F32) for v in vectors)
    return dict(eye=np.zeros(4, F32), eye_to_top_left=tl, left_to_right=lr, top_to_bottom=tb, pixel_size_inv=1.0)
