"""Inputs and comparers shared by test_scene_prep.py (no GPU) and test_scene_prep_gpu.py: synthetic grids built cell by cell, and the two
checks every dense view goes through -- array equality with prep_oracle.dense_view and the consumer's decode of every non-empty cell."""
import numpy as np

import prep_oracle as O


def cell_id(cx, cy, cz):
    return cx + 256 * cy + 65536 * cz


def grid_from_cells(lists):
    """{cell id: [triangle ids]} -> (grid_start [256^3 + 1] u32, grid_list u32); any monotone start array with entries below the triangle
    count is a legal grid, whether or not the triangles touch the cells."""
    counts = np.zeros(O.CELLS + 1, np.uint32)
    cells = sorted(lists)
    for c in cells:
        counts[c + 1] = len(lists[c])
    start = np.cumsum(counts, dtype=np.uint64).astype(np.uint32)
    flat = [t for c in cells for t in lists[c]]
    return start, np.asarray(flat, np.uint32).reshape(-1)


CORNERS = ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255))


def synthetic_grids(T, seed=20260):
    """name -> {cell id: [triangle ids < T]}.  By construction: "counts" has cells with exactly 1, 2, 14, 15, 16 and 300 candidates, one
    triangle repeated inside a cell and one triangle in many cells, a block with all 64 cells occupied, blocks with only bit 0 and only
    bit 63, and the five corner cells (so the very last block is non-empty); "last_block_empty" ends well before the last block;
    "random" is a seeded scatter that leaves the last block empty too; "empty" has no pair and "single" exactly one."""
    rng = np.random.default_rng(seed)
    ids = lambda n: [int(v) for v in rng.integers(0, T, n)]
    counts = {}
    for n, at in ((1, (9, 3, 200)), (2, (10, 3, 200)), (14, (11, 3, 200)), (15, (12, 3, 200)), (16, (13, 3, 200)), (300, (77, 130, 5)),
                  (13, (14, 3, 200)), (17, (15, 3, 200)), (31, (16, 3, 200))):
        counts[cell_id(*at)] = ids(n)
    counts[cell_id(40, 41, 42)] = [T - 1] * 20                       # the same triangle twenty times in one cell
    counts[cell_id(41, 41, 42)] = [5, 7, 5, 7, 5]
    for i in range(90):                                             # the same triangle in many cells, along a diagonal
        counts.setdefault(cell_id(100 + i, 20 + i, 30 + 2 * i), []).append(3)
    for z in range(4):                                              # a block with all 64 cells occupied: bit 63 set
        for y in range(4):
            for x in range(4):
                counts[cell_id(4 * 20 + x, 4 * 21 + y, 4 * 22 + z)] = ids(1 + (x + 2 * y + 3 * z) % 4)
    counts[cell_id(4 * 30, 4 * 31, 4 * 32)] = ids(3)                 # only bit 0
    counts[cell_id(4 * 33 + 3, 4 * 31 + 3, 4 * 32 + 3)] = ids(2)     # only bit 63
    counts[cell_id(4 * 63 + 3, 4 * 31 + 3, 4 * 32 + 3)] = ids(1)     # bit 63 of a block at the far x edge
    for i, c in enumerate(CORNERS):
        counts[cell_id(*c)] = ids(1 + i)
    last_empty = {cell_id(0, 0, 0): ids(2), cell_id(3, 3, 3): ids(16), cell_id(255, 255, 251): ids(15), cell_id(251, 255, 255): ids(1),
                  cell_id(255, 251, 255): ids(14), cell_id(128, 128, 128): ids(40)}
    random = {}
    for c in rng.integers(0, cell_id(0, 0, 250), 3000):
        random[int(c)] = ids(int(rng.choice([1, 1, 1, 2, 3, 14, 15, 16, 60])))
    return {"counts": counts, "last_block_empty": last_empty, "random": random, "empty": {}, "single": {cell_id(200, 100, 50): [T // 2]}}


def compare_views(got, want):
    """Names of the dense view's arrays that differ between two views (every element compared)."""
    bad = []
    for key in ("words", "sparse", "pair_rec"):
        if got[key].shape != want[key].shape or not np.array_equal(got[key], want[key]):
            bad.append(key)
    return bad


def decode_faults(view, grid_start, grid_list, cells, empties=()):
    """The cells of `cells` (non-empty) whose decode_cell differs from grid_list[grid_start[c]:grid_start[c + 1]], and the cells of `empties`
    that do not decode to nothing.  A decode that runs off the arrays counts as a fault."""
    bad = []
    for c in list(cells) + list(empties):
        want = [int(t) for t in grid_list[int(grid_start[c]):int(grid_start[c + 1])]]
        try:
            got = O.decode_cell(view, *O.cell_xyz(c))
        except IndexError:
            got = None
        if got != want:
            bad.append(int(c))
    return bad


def empty_sample(grid_start, n=2000, seed=7):
    """A fixed sample of empty cells: seeded picks, the corner cells, and the neighbours of every non-empty cell's id (where empty)."""
    rng = np.random.default_rng(seed)
    counts = np.diff(np.asarray(grid_start, np.uint32).astype(np.int64))
    full = np.flatnonzero(counts)
    near = np.concatenate([full[:n] - 1, full[:n] + 1, full[:n] + 256, full[:n] - 65536]) if len(full) else np.zeros(0, np.int64)
    pick = np.concatenate([rng.integers(0, O.CELLS, n), near, [cell_id(*c) for c in CORNERS]])
    pick = np.unique(pick[(pick >= 0) & (pick < O.CELLS)])
    return pick[counts[pick] == 0]
