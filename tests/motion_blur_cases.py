"""Shapes, synthetic fields, the parameter grid and the measured shares of the motion blur tests (tests/test_motion_blur.py runs the
kernel's per-pixel code on the host and shows on the oracle alone that the inputs are not vacuous; tests/test_motion_blur_gpu.py runs
the same cases on the device).  Oracle results are computed once per case and shared (reference()); nobody changes them."""
import functools
import itertools

import numpy as np

import motion_blur_oracle as BO
import motion_cases as MC

F32 = np.float32
# one pixel; a partial workgroup; exactly one workgroup; tiles crossed in x and in y; a partial tile in both; a 4 x 3 tile grid whose tile
# (1, 1) and (2, 1) have all eight neighbours
SHAPES = ((1, 1), (31, 7), (32, 8), (33, 33), (65, 34), (97, 70))
# seven tile columns: wide enough for tiles whose whole neighbourhood stands still beside tiles that move, so that `split` runs the copy
# arm and the gather arm in ONE image (in a 4 x 3 grid every tile neighbours the moving half)
WIDE = (200, 40)
FIELDS = ("uniform", "split", "random", "ties")
SPECIALS_SHAPE = (65, 34)
TAPS, SHUTTERS, MAX_BLURS, SOFTNESS = (1, 2, 15, 64), (0.0, 0.5, 4.0), (1.0, 7.5, 32.0), (0.0, 0.05)
GRID = tuple(dict(taps=t, shutter=s, max_blur=m, depth_softness=d) for t, s, m, d in itertools.product(TAPS, SHUTTERS, MAX_BLURS, SOFTNESS))
# 1 x 257 tiles: the second workgroup of (c) (one lane per tile, 256 lanes) and block indices of (d) far past the first tile row.  W = 2
# keeps the numpy oracle cheap (16 400 pixels); it runs TALL_GRID, every tap count once with the other settings varied (grid_of)
TALL = (2, 8200)
TALL_GRID = tuple(dict(taps=t, shutter=s, max_blur=m, depth_softness=d)
                  for t, s, m, d in ((1, 0.5, 7.5, 0.05), (2, 4.0, 32.0, 0.0), (15, 0.5, 32.0, 0.05), (64, 4.0, 7.5, 0.0)))
CASES = (tuple((f, W, H) for W, H in SHAPES for f in FIELDS) + (("specials",) + SPECIALS_SHAPE, ("split",) + WIDE, ("random",) + WIDE)
         + (("random",) + TALL, ("ties",) + TALL))


def grid_of(W, H):
    """The settings a case of W x H runs: the whole GRID, TALL_GRID at the tall shape."""
    return TALL_GRID if (W, H) == TALL else GRID


# Non-vacuity conditions (test_motion_blur.py asserts them on the oracle's intermediate results): `split` and `random` each put this
# share of the pixels of some tested case into the copy arm and into the gather arm, and `random` clamps this share.
MIN_COPY, MIN_GATHER, MIN_CLAMPED = 0.20, 0.20, 0.10
# Measured on the oracle at shutter 0.5, maxBlur 7.5 (copy share, gather share, clamped share):
#   split  200 x 40: 0.320, 0.680, 0.000 -- tile columns 0 and 1 copy, 2 neighbours the column the boundary x = 100 cuts, 3..6 move
#   split  97 x 70:  0.000, 1.000, 0.000 -- every tile neighbours a moving one: both arms in one image need the wide shape
#   random 200 x 40: 0.000, 1.000, 0.621 -- every tile holds a fast pixel, so its copy arm is the shutter-0 case (1.000, 0.000, 0.000);
#                    lengths above 30 px are capped: 1 - 30/80
#   random 97 x 70:  0.000, 1.000, 0.631
MEASURED = {("split", 200, 40): (0.320, 0.680, 0.000), ("random", 200, 40): (0.000, 1.000, 0.621)}

# Bounds measured on the oracle and given 4 x margin (test_motion_blur.py prints what it measures):
#   a constant finite colour (0.3, 0.55, 0.8125) under every field but `specials`, every shape and the whole GRID: the largest
#   |out - colour| was 12 ulp of the colour (`random` 65 x 34, 64 taps, shutter 0.5, maxBlur 32, depthSoftness 0) -> 48 ulp.  (No
#   weight is negative, so nothing cancels: sum and wsum are sums of at most 65 terms with a rounding each, which is what is seen.)
CONSTANT_COLOUR_ULP = 48
#   a still near object (depth 1) beside a fast far background (depth 10, motion (20, 0), shutter 0.5 -> a half-extent of 5 px):
#   interior pixels (farther than 5 px from the silhouette, +1 for the dither) stayed within 2^-23 of their own colour (colours in
#   [0, 1)) -> 2^-21.  The far taps weigh exactly zero there -- f = 0 (they lie behind by far more than depthSoftness), the cone and the
#   cylinder of the object's own 0.5 px streak end within a pixel -- so what is left is the rounding of sum / wsum over the taps that
#   land on the pixel itself.
STILL_INTERIOR_BOUND = 2.0 ** -21

# Scene path (tests/test_motion_blur_gpu.py): the share of pixels in the gather arm per step at the parameters SCENE_PARAMS, measured on
# the CPU with motion_oracle.motion; the condition is MIN_GATHER in at least one step per scene.
SCENE_PARAMS = (dict(), dict(shutter=1.0, max_blur=32.0, taps=7, depth_softness=0.0))
CAMERA_SCENES = dict(MC.CAMERA_SCENES)
GEOMETRY_SCENE = "mirror_hall"
SCENE_GATHER_SHARES = {}  # filled below


def _layers(rng, W, H):
    """Depths in 8 x 8 blocks drawn from a near layer, one within 5 % of it, a far one and the background."""
    pick = rng.integers(0, 4, ((H + 7) // 8, (W + 7) // 8))
    z = np.asarray([1.0, 1.03, 2.5, np.inf], F32)[pick]
    return np.ascontiguousarray(np.repeat(np.repeat(z, 8, 0), 8, 1)[:H, :W])


@functools.lru_cache(maxsize=None)
def fields(name, W, H, seed=11):
    """(colour [H, W, 3], motion [H, W, 2], depth [H, W]) of field `name`, read-only."""
    rng = np.random.default_rng([seed, W, H, FIELDS.index(name) if name in FIELDS else 9])
    colour = rng.random((H, W, 3), dtype=F32)
    motion = np.zeros((H, W, 2), F32)
    depth = _layers(rng, W, H)
    y, x = np.indices((H, W))
    if name == "uniform":  # every tile moves: all pixels take the gather arm
        motion[...] = (9.0, -4.0)
    elif name == "split":  # the left half stands still at depth 1, the right half moves at depth 5
        right = x >= W // 2
        motion[right] = (0.0, 14.0)
        depth = np.where(right, F32(5.0), F32(1.0))
    elif name == "random":  # lengths 0..80 px in every direction: the cap, and ties among capped pixels (l == maxBlur exactly)
        length, angle = rng.random((H, W), dtype=F32) * F32(80.0), rng.random((H, W), dtype=F32) * F32(2 * np.pi)
        if (W, H) == TALL:  # two pixels wide: only a velocity within a degree of the vertical keeps its taps inside the image, up or down
            angle = (F32(np.pi / 2) + np.floor(angle / F32(np.pi)) * F32(np.pi) + (angle % F32(0.04) - F32(0.02))).astype(F32)
        motion[..., 0], motion[..., 1] = length * np.cos(angle), length * np.sin(angle)
    elif name == "ties":  # one length everywhere, signs that differ from pixel to pixel and from tile origin to tile origin
        across = F32(0.25) if (W, H) == TALL else F32(6.0)  # (two pixels wide: nearly vertical, so that taps stay inside the image)
        motion[..., 0] = np.where((x * 7 + y * 3) % 5 < 2, across, -across)
        motion[..., 1] = np.where((x + y * 11) % 3 == 0, F32(6.0), F32(-6.0))
    elif name == "specials":
        length, angle = rng.random((H, W), dtype=F32) * F32(24.0), rng.random((H, W), dtype=F32) * F32(2 * np.pi)
        motion[..., 0], motion[..., 1] = length * np.cos(angle), length * np.sin(angle)
        flat_m, flat_z, flat_c = motion.reshape(-1, 2), depth.reshape(-1), colour.reshape(-1, 3)
        odd_m = [(np.nan, 1.0), (2.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (np.inf, -np.inf), (1e-40, -1e-40), (1e30, 1e30), (-1e30, 3.0),
                 (1e-40, 0.0), (3e19, 3e19)]
        odd_z = [0.0, -1.0, np.nan, np.inf, -np.inf, -0.0, 1e-40, 1e30]
        for k, at in enumerate(rng.choice(W * H, 160, replace=False)):
            if k % 3 == 0:
                flat_m[at] = odd_m[(k // 3) % len(odd_m)]
            elif k % 3 == 1:
                flat_z[at] = odd_z[(k // 3) % len(odd_z)]
            else:
                flat_c[at, k % 3 if k % 2 else slice(None)] = np.nan if k % 4 else np.inf
    else:
        raise KeyError(name)
    out = (colour, motion, np.ascontiguousarray(depth, F32))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, W, H, params):
    out = BO.blur(*fields(name, W, H), **dict(params))
    out.setflags(write=False)
    return out


def reference(name, W, H, params):
    """The oracle's output for a case under `params` (a dict of GRID), computed once."""
    return _reference(name, W, H, tuple(sorted(params.items())))


def shares(parts):
    """(copy share, gather share, clamped share) of an oracle result with_parts."""
    g = float(parts["gathered"].mean())
    return 1.0 - g, g, float(parts["clamped"].mean())


# (kind, name) -> the gather share per step at SCENE_PARAMS[0] (the defaults).  Every scene has a step at or above MIN_GATHER, so none
# was swapped: at these crops (at most 5 x 5 tiles of 32 pixels) one moving pixel per neighbourhood puts a whole tile into the gather arm.
# reindex moves nothing and is the scenes' copy-arm step.
SCENE_GATHER_SHARES.update({
    ("camera", "mirror_hall"): {"pan": 1.0, "orbit90": 1.0, "inside": 1.0, "home": 1.0},
    ("camera", "axis_near_axis_mixed"): {"pan": 1.0, "orbit90": 1.0, "inside": 1.0, "home": 1.0},
    ("camera", "axis_class_sun"): {"pan": 1.0, "orbit90": 1.0, "inside": 1.0, "home": 1.0},
    ("geometry", "mirror_hall"): {"reindex": 0.0, "translate": 1.0, "twist": 1.0, "collapse": 1.0},
})
