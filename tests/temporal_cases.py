"""Inputs shared by the temporal accumulation tests (tests/test_temporal.py shows on the oracle alone that they are not vacuous,
tests/test_temporal_gpu.py runs them on the device): seeded synthetic fields, and chains of frames over the scenes and change sequences of
motion_cases.py.

A chain is what a host's loop makes: frame 0 at the base state, then one frame per change; every frame is reprojected against the frame
before it, because rtHipSceneTemporal marks the scene after itself."""
import numpy as np

import motion_cases as MC
import motion_oracle as MO
import temporal_oracle as TO

F32 = np.float32
NONE = 0xFFFFFFFF
SIZES = ((1, 1), (37, 29), (130, 70))  # (W, H): a single pixel; odd; no multiple of the 8 x 8 block and wider than a tile
# What the fields must hold, as shares of their pixels (conditions on the inputs, checked by tests/test_temporal.py).  Measured on the
# oracle with the defaults, (all four taps accepted, some but not all, reset): 37 x 29: 0.306, 0.402, 0.293; 130 x 70: 0.302, 0.430, 0.268.
MIN_ALL_TAPS, MIN_SOME_TAPS, MIN_RESET = 0.25, 0.10, 0.10
# Scene chains: of the pixels that hit, the share that accepts history in at least one step, and the pixels that the triangle or depth
# test refuses a tap of in at least one step.  Measured on the oracle (accepting share, refused pixels): camera chains mirror_hall 0.831,
# 309; axis_near_axis_mixed 0.862, 16056; axis_class_sun 0.904, 15488; geometry chain mirror_hall 0.990, 381.
MIN_ACCEPT = 0.20
CAMERA_SCENES = MC.CAMERA_SCENES
GEOMETRY_SCENE = "mirror_hall"


def depth(qx, qy):
    """The synthetic history's t map, as a function of the history pixel (float64 in, exact enough: it only has to be smooth)."""
    return 5.0 + 0.02 * qx + 0.03 * qy


def ids(qx, qy):
    """The synthetic history's triangle map: blocks of 6 x 5 pixels, so that many 2 x 2 footprints straddle an edge."""
    return (np.floor(qx / 6.0) + 64.0 * np.floor(qy / 5.0)).astype(np.int64).astype(np.uint32) + np.uint32(7)


def fields(W, H, seed=1):
    """(colour, motion, prev_t, triangle, history) for a W x H image: a smooth fractional flow whose footprints land inside one id block
    (all taps accepted) or across an edge (some), a band of rows whose flow points outside the image, a band whose depth disagrees,
    pixels without history, and a band of specials -- NaN, infinite and huge motion, prev_t <= 0 and NaN, a missed pixel over a missed
    history, infinite and NaN history counts, NaN and infinite colours, flows that land exactly on the range test's limits."""
    rng = np.random.default_rng(1000 * seed + 7 * W + H)
    ys, xs = np.mgrid[0:H, 0:W]
    colour = rng.random((H, W, 3), dtype=F32)
    hist = dict(colour=rng.random((H, W, 3), dtype=F32),
                count=(1.0 + 40.0 * rng.random((H, W))).astype(F32),  # some above the default maxHistory
                t=depth(xs.astype(np.float64), ys.astype(np.float64)).astype(F32), triangle=ids(xs.astype(np.float64), ys.astype(np.float64)))
    hist["count"][rng.random((H, W)) < 0.08] = 0.0  # no history here
    hist["count"][rng.random((H, W)) < 0.03] = 0.75  # nor here: below 1
    # the flow: smooth, fractional, a little different in every pixel; every 9th pixel moves by whole pixels (weights 1, 0, 0, 0)
    motion = np.stack([1.3 + 0.011 * xs - 0.004 * ys, -0.7 + 0.006 * xs + 0.013 * ys], -1).astype(F32)
    whole = (xs + 2 * ys) % 9 == 0
    motion[whole] = np.round(motion[whole])
    if W * H == 1:
        motion[:] = 0.0  # (any other flow leaves a single pixel's image)
    gx = xs.astype(np.float64) + motion[..., 0].astype(np.float64)
    gy = ys.astype(np.float64) + motion[..., 1].astype(np.float64)
    # the pixel shows the surface the nearest history pixel showed, at the depth the history's map has there, within 2 %
    triangle = ids(np.clip(np.round(gx), 0, W - 1), np.clip(np.round(gy), 0, H - 1))
    prev_t = (depth(gx, gy) * (1.0 + 0.02 * (rng.random((H, W)) - 0.5))).astype(F32)
    band = ys % 11
    motion[band == 3, 0] += F32(2.0 * W) * np.where(xs[band == 3] % 2 == 0, F32(1), F32(-1))  # points outside, to either side
    prev_t[band == 5] *= F32(1.25)  # the depth disagrees: hidden a frame ago
    sp = (band == 8) & (H > 1)
    kind = (xs + ys // 11) % 16
    with np.errstate(all="ignore"):
        motion[sp & (kind == 0)] = np.nan
        motion[sp & (kind == 1), 0] = np.inf
        motion[sp & (kind == 2), 1] = -1e30
        prev_t[sp & (kind == 3)] = 0.0
        prev_t[sp & (kind == 4)] = -2.5
        prev_t[sp & (kind == 5)] = np.nan
        miss = sp & (kind == 6)  # a missed pixel whose flow (a whole pixel to the left) points at a missed history pixel
        motion[miss] = (-1.0, 0.0)
        prev_t[miss] = np.inf
        triangle[miss] = NONE
        mx = np.clip(xs[miss] - 1, 0, W - 1)
        hist["t"][ys[miss], mx] = np.inf
        hist["triangle"][ys[miss], mx] = NONE
        hist["count"][ys[miss], mx] = 3.0
        hist["count"][sp & (kind == 7)] = np.inf
        hist["count"][sp & (kind == 8)] = np.nan
        hist["colour"][sp & (kind == 9)] = np.nan
        hist["colour"][sp & (kind == 10), 1] = np.inf
        colour[sp & (kind == 11)] = np.nan
        edge = sp & (kind == 12)  # gx = -1 exactly: inside the range, only the right-hand taps exist
        motion[edge, 0] = (-1.0 - xs[edge]).astype(F32)
        edge = sp & (kind == 13)  # gx = W exactly: outside
        motion[edge, 0] = (W - xs[edge]).astype(F32)
        edge = sp & (kind == 14)  # gy just below H: the lower taps lie outside
        motion[edge, 1] = (H - 0.25 - ys[edge]).astype(F32)
        prev_t[sp & (kind == 15)] = 1e-40  # subnormal, > 0
    return colour, motion, prev_t, triangle, hist


def shares(out):
    """(all four taps accepted, some but not all, reset) as shares of the pixels of accumulate(..., with_taps=True)."""
    used, taps = out["used"], out["taps"]
    return float((used & (taps == 4)).mean()), float((used & (taps < 4)).mean()), float((~used).mean())


def camera_chain(sc, sequence=MC.CAMERA_SEQUENCE):
    """[(label, current Scene, reference Scene)]: the home pose first, measured against itself, then every pose against the one before."""
    chain, cur = [("home", sc, sc)], sc
    for pose, _ in sequence:
        nxt = MC.posed(sc, pose)
        chain.append((pose, nxt, cur))
        cur = nxt
    return chain


def geometry_chain(sc, sequence=MC.GEOMETRY_SEQUENCE):
    """[(label, arrays or None, current Scene, reference Scene)]: the base shape first, then every deformation against the one before."""
    chain, cur = [("base", None, sc, sc)], sc
    for name, _ in sequence:
        arrays, nxt = MC.shaped(sc, name)
        chain.append((name, arrays, nxt, cur))
        cur = nxt
    return chain


def chain_flows(states):
    """MO.motion of every (current, reference) pair of a chain."""
    return [MO.motion(cur, ref) for cur, ref in states]


def chain_shares(flows):
    """(share of the hit pixels that accept history in at least one step, pixels refused a tap by the triangle or depth test in at least one
    step) over a chain's flows.  Acceptance does not depend on the colour, so the frames are left black here."""
    H, W = flows[0]["t"].shape
    black = np.zeros((H, W, 3), F32)
    hist = TO.empty_history(H, W)
    accepted, refused, hit = np.zeros((H, W), bool), np.zeros((H, W), bool), np.zeros((H, W), bool)
    for i, f in enumerate(flows):
        out = TO.accumulate(black, f["motion"], f["prev_t"], f["triangle"], hist, with_taps=True)
        if i:
            now = f["triangle"] != NONE
            hit |= now
            accepted |= now & out["used"]
            refused |= out["live"] > out["taps"]
        hist = TO.next_history(out, f["t"], f["triangle"])
    return float(accepted.sum() / max(int(hit.sum()), 1)), int(refused.sum())
