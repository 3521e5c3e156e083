"""Inputs shared by the temporal clamp's tests (tests/test_temporal_clamp.py shows on the oracle alone that they are not vacuous,
tests/test_temporal_clamp_gpu.py runs them on the device): the synthetic fields of temporal_cases.py with the history colour perturbed,
the same with special values sprinkled over frame and history, and the relight chain's scene and light sets."""
import numpy as np

import temporal_cases as TC

F32 = np.float32
# (W, H): a single pixel; smaller than a block; one column and one row short of a 32 x 8 block; the block; one pixel into a second block
# either way; 2 x 2 blocks and one pixel more; 4 x 4 blocks with partly filled last ones
SHAPES = ((1, 1), (3, 2), (31, 7), (32, 8), (33, 9), (64, 16), (65, 17), (97, 25))
SPECIAL_SHAPE = (65, 17)
MODES = (1, 2, 3)
GAMMAS = (0.0, 1.0, 2.5)
# Conditions on the perturbed fields, as shares of the pixels that blend history in (tests/test_temporal_clamp.py checks them on the
# oracle for every mode at gamma = 1 on the shapes of at least MIN_PIXELS pixels).  Measured on the oracle, (moved, unmoved): mode 1
# 0.426 .. 0.535, 0.465 .. 0.574; mode 2 0.474 .. 0.586, 0.414 .. 0.526; mode 3 0.494 .. 0.586, 0.414 .. 0.506.
MIN_MOVED, MIN_UNMOVED, MIN_PIXELS = 0.10, 0.10, 200
FAR_SHARE, NEAR, FAR = 0.25, 0.1, 3.0


def fields(W, H, seed=1, moments=False):
    """temporal_cases.fields(W, H) with the history colour perturbed: every finite history colour is drawn towards mid-grey (0.5 + NEAR
    * (value - 0.5): inside the 3x3 box of a frame of uniform random colours, whether min/max or mean +- sigma), and FAR_SHARE of the
    history pixels, seeded, are then pushed by +-FAR in every channel: far outside every box.  The NaN and infinite history colours of
    the special band stay.  moments: "moments" in the history (variance_cases.moment_fields')."""
    if moments:
        import variance_cases as VC
        colour, motion, prev_t, tri, hist = VC.moment_fields(W, H, seed)
    else:
        colour, motion, prev_t, tri, hist = TC.fields(W, H, seed)
    rng = np.random.default_rng(3000 * seed + 7 * W + H)
    old = hist["colour"]
    far = np.where(rng.random((H, W)) < FAR_SHARE, np.where(rng.random((H, W)) < 0.5, F32(FAR), F32(-FAR)), F32(0))
    with np.errstate(all="ignore"):
        new = (F32(0.5) + F32(NEAR) * (old - F32(0.5))) + far[..., None]
    hist = dict(hist, colour=np.where(np.isfinite(old), new, old).astype(F32))
    return colour, motion, prev_t, tri, hist


def special_fields(W, H, seed=1, moments=False):
    """fields(W, H) with NaN, +inf, -inf and subnormal colours sprinkled over single channels of the frame and of the history, a few per
    cent each, so that boxes hold them as a tap, as the centre, as the minimum and as the maximum."""
    colour, motion, prev_t, tri, hist = fields(W, H, seed, moments)
    rng = np.random.default_rng(4000 * seed + 7 * W + H)
    colour, hc = colour.copy(), hist["colour"].copy()
    for a in (colour, hc):
        kind = rng.integers(0, 40, a.shape)
        a[kind == 0] = np.nan
        a[kind == 1] = np.inf
        a[kind == 2] = -np.inf
        a[kind == 3] = 1e-40
        a[kind == 4] = -1e-40
        a[kind == 5] = -0.0
        a[kind == 6] = 3e38  # (its square overflows)
    return colour, motion, prev_t, tri, dict(hist, colour=hc)


def moved_shares(out):
    """(share with a channel moved, share with none moved) of the pixels that blend history in."""
    used = out["used"]
    moved = (out["moved"] != 0).any(-1) & used
    total = max(int(used.sum()), 1)
    return float(moved.sum() / total), float((used & ~moved).sum() / total)


# ---- the relight chain ----------------------------------------------------------------------------------------------------------------
# A soup cropped to 2 x 2 tiles of 128 x 128, the right-hand and the lower ones partly filled (motion_cases.base_scene).
RELIGHT_SCENE, RELIGHT_SIZE = "odd_size_multi_tile", (160, 136)


def relight_lights():
    """(the first frame's lights, the second frame's): edit_cases' sun, and the same sun dimmed to a quarter."""
    from edit_cases import ONE_SUN
    dimmed = [dict(ONE_SUN[0], col=tuple(0.25 * c for c in ONE_SUN[0]["col"]))]
    return ONE_SUN, dimmed
