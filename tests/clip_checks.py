"""Checks of a resident scene's ray-clip bound (csrc/rt_ray_clip.h), shared by tests/test_ray_clip_gpu.py and the session tests
(tests/session_cases.py): the occupied cells read from the device's block table, and the kept planes against every corner of them."""
import numpy as np

import prep_oracle as P


def occupied_cells(rs):
    """[n, 3] cell coordinates (x, y, z) of the occupied cells, from the block table {word lo, word hi, rank} at 3 * (bx | by << 8 | bz << 16)."""
    table = rs.scene_view("block_sparse").reshape(-1, 3)
    b = np.arange(64)
    idx = (b[None, None, :] | (b[None, :, None] << 8) | (b[:, None, None] << 16)).reshape(-1)  # [bz][by][bx]
    words = table[idx, 0].astype(np.uint64) | (table[idx, 1].astype(np.uint64) << np.uint64(32))
    cells = []
    for bit in range(64):
        has = np.flatnonzero((words >> np.uint64(bit)) & np.uint64(1))
        if has.size:
            bx, by, bz = has & 63, (has >> 6) & 63, has >> 12
            cells.append(np.stack([bx * 4 + (bit & 3), by * 4 + ((bit >> 2) & 3), bz * 4 + (bit >> 4)], 1))
    return np.concatenate(cells) if cells else np.zeros((0, 3), np.int64)


def assert_bound(rs, box_min, label):
    """Every corner of every occupied cell satisfies every kept plane (float64 arithmetic on the float32 values); returns the planes and the
    share of the 32^3 lattice of cell centres (cells 4, 12, .. 252 per axis) they cut off."""
    planes = P.planes_of(box_min).astype(np.float64)
    kept = rs.clip_planes().astype(np.float64)
    cells = occupied_cells(rs)
    assert cells.shape[0] > 0, label
    lo = np.stack([planes[w][cells[:, w]] for w in range(3)], 1)
    hi = np.stack([planes[w][cells[:, w] + 1] for w in range(3)], 1)
    for k, (nx, ny, nz, off) in enumerate(kept):
        assert abs(nx * nx + ny * ny + nz * nz - 1.0) < 1e-5, (label, k)
        n = np.array([nx, ny, nz])
        worst = (np.where(n >= 0, hi, lo) * n).sum(1).max()  # (the corner furthest along n is the one that decides)
        assert worst <= off, f"{label}: plane {k} {kept[k]} is passed by an occupied cell's corner ({worst} > {off})"
    c = np.arange(32) * 8 + 4
    centre = [0.5 * (planes[w][c] + planes[w][c + 1]) for w in range(3)]
    X, Y, Z = np.meshgrid(*centre, indexing="ij")
    cut = np.zeros(X.shape, bool)
    for nx, ny, nz, off in kept:
        cut |= nx * X + ny * Y + nz * Z > off
    return kept, float(cut.mean())
