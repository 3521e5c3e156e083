"""The scene upload's device arrays restated in numpy, from the layout comments of opencl_render_amd/csrc/rt_device.h (RtDevScene)
and include/raytrace_hip.h -- not from the kernels that make them (rt_scene_prep.hip, rt_prepare_triangles, rt_gather_pair_records).

``tile_major_ranges``  the per-pixel candidate ranges of an instance's tiles, index slot*128*128 + ly*128 + lx
``triangle_records``   triRec [T,16] and triShade [T,24] in float32 with the operation order of rt_devfuncs.h (dot3, cross3)
``dense_view``         the producer's side of the dense grid view: block words, sparse block table, pair records
``decode_cell``        the CONSUMER's side of the same view: a cell's triangle ids read back the way the trace kernel finds them
``cell_lut`` / ``planes_tame``  the two host loops of build_grid

Everything is exact: the library is built without fp contraction and with correctly rounded division, so float32 numpy gives the
same bits, and the tests compare words, not values.
"""
import numpy as np

TILE = 128
TILE_PIXELS = TILE * TILE
GRID = 256
CELLS = GRID ** 3
BLOCKS = (GRID // 4) ** 3
SPARSE_WORDS = 3 * ((63 << 16 | 63 << 8 | 63) + 1)
PAIR_MANY = 15
PAIR_LIMIT = 1 << 28

ERR_TRI_INDEX, ERR_TRI_MATERIAL, ERR_CAM_ENTRY, ERR_CAM_RANGE, ERR_GRID_MONOTONE, ERR_GRID_ENTRY = 1, 2, 4, 8, 16, 32
# the sentence rtHipLastError() carries for each bit ("scene rejected (0x<mask>): <sentence>; <sentence>; ...")
ERR_TEXT = {
    ERR_TRI_INDEX: "a triangle references a vertex that does not exist;",
    ERR_TRI_MATERIAL: "a triangle uses a material >= materialCount;",
    ERR_CAM_ENTRY: "a camera list entry is not a triangle;",
    ERR_CAM_RANGE: "a camera list range exceeds the list size;",
    ERR_GRID_MONOTONE: "scenePixelTriangleListStart is not monotone;",
    ERR_GRID_ENTRY: "a grid list entry is not a triangle;",
}


def rejection_text(mask):
    """The whole rtHipLastError() text of a scene refused with exactly the bits of `mask`."""
    return "scene rejected (0x%x):" % mask + "".join(" " + ERR_TEXT[b] for b in sorted(ERR_TEXT) if mask & b)


# ---------------------------------------------------------------------------------------------------------------
# tile-major candidate ranges
# ---------------------------------------------------------------------------------------------------------------

def tile_major_ranges(W, H, tile_ids, cam_start, cam_end, list_size):
    """(start, end, error bits) for the tiles `tile_ids` of a W x H image, tile t covering pixels (t % tilesX)*128.., (t // tilesX)*128..
    A range with end < start is the empty range start..start, a pixel of a tile that lies outside the image has 0..0, a range that
    ends past the list has 0..0 and raises ERR_CAM_RANGE."""
    tiles_x = (W + TILE - 1) // TILE
    ids = np.asarray(tile_ids, np.int64).reshape(-1)
    ly, lx = np.divmod(np.arange(TILE_PIXELS, dtype=np.int64), TILE)
    gx = (ids % tiles_x)[:, None] * TILE + lx[None, :]
    gy = (ids // tiles_x)[:, None] * TILE + ly[None, :]
    inside = (gx < W) & (gy < H)
    p = np.where(inside, gy * W + gx, 0)
    cs = np.asarray(cam_start, np.uint32).astype(np.int64)
    ce = np.asarray(cam_end, np.uint32).astype(np.int64)
    a = np.where(inside, cs[p], 0)
    b = np.maximum(np.where(inside, ce[p], 0), a)
    bad = b > int(list_size)
    a[bad] = 0
    b[bad] = 0
    return a.astype(np.uint32).ravel(), b.astype(np.uint32).ravel(), (ERR_CAM_RANGE if bad.any() else 0)


# ---------------------------------------------------------------------------------------------------------------
# triangle records
# ---------------------------------------------------------------------------------------------------------------

def _dot3(a, b):  # rt_devfuncs.h dot3: (a0*b0 + a1*b1) + a2*b2
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross3(a, b):  # rt_devfuncs.h cross3
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def triangle_records(vertex, tri_index, tri_material, tri_uv, tri_normal):
    """triRec [T,16] = a.xyz | ab.xyz | ac.xyz | n.xyz (= cross(ac, ab)) | abab abac acac 1/(abac^2 - abab*acac) and
    triShade [T,24] = b.xyz c.xyz | nA nB nC | uvA uvB uvC | material id (its bits) | two zero words, both float32.
    Only lanes x, y, z of tri_index are read."""
    v = np.asarray(vertex, np.float32)
    idx = np.asarray(tri_index, np.int32)
    T = idx.shape[0]
    a, b, c = (v[idx[:, k].astype(np.int64), :3] for k in range(3))
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        n = _cross3(ac, ab)
        abab, abac, acac = _dot3(ab, ab), _dot3(ab, ac), _dot3(ac, ac)
        inv = np.float32(1) / (abac * abac - abab * acac)
    rec = np.concatenate([a, ab, ac, n, abab[:, None], abac[:, None], acac[:, None], inv[:, None]], 1).astype(np.float32)
    shade = np.zeros((T, 24), np.float32)
    shade[:, 0:3], shade[:, 3:6] = b, c
    shade[:, 6:15] = np.asarray(tri_normal, np.float32).reshape(T, 3, -1)[:, :, :3].reshape(T, 9)
    shade[:, 15:21] = np.asarray(tri_uv, np.float32).reshape(T, 6)
    shade.view(np.uint32)[:, 21] = np.asarray(tri_material, np.int32).view(np.uint32)
    assert rec.dtype == np.float32 and rec.shape == (T, 16)
    return np.ascontiguousarray(rec), shade


def same_float_words(got, want):
    """Bit equality of two float32 arrays, except that a word which is NaN on both sides counts as equal (numpy and the GPU need not
    agree on a NaN's sign and payload).  Returns the boolean array of matching words."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


# ---------------------------------------------------------------------------------------------------------------
# dense grid view
# ---------------------------------------------------------------------------------------------------------------

def _block_major(a):
    """[256^3] in cell order cx + 256*cy + 65536*cz -> [BLOCKS, 64]: block (cx>>2) + 64*(cy>>2) + 4096*(cz>>2), bit (cx&3) | (cy&3)<<2 | (cz&3)<<4."""
    return a.reshape(64, 4, 64, 4, 64, 4).transpose(0, 2, 4, 1, 3, 5).reshape(BLOCKS, 64)


def pair_words(tri_rec, tri, info):
    """The 16 words of pair records for triangles `tri` with count words `info`: {a.xyz, id} {n.xyz, count} {ab.xyz, abac} {ac.xyz, inv}."""
    r = np.asarray(tri_rec, np.float32).view(np.uint32).reshape(-1, 16)[np.asarray(tri, np.int64)]
    out = np.empty((len(tri), 16), np.uint32)
    out[:, 0:3], out[:, 3] = r[:, 0:3], tri
    out[:, 4:7], out[:, 7] = r[:, 9:12], info
    out[:, 8:11], out[:, 11] = r[:, 3:6], r[:, 13]
    out[:, 12:15], out[:, 15] = r[:, 6:9], r[:, 15]
    return out


def dense_view(grid_start, grid_list, tri_rec):
    """dict(words [BLOCKS] u64, sparse [SPARSE_WORDS] u32, pair_rec [pairs,16] u32, cells): the dense view of a grid as the RtDevScene
    comment describes it.  Non-empty cells get dense ids in block order, bit order inside a block; record k < cells is the first
    candidate of cell k with the count word min(n, 15) | rest << 4; the further candidates of cell k sit, in list order, at
    rest .. rest + n - 2, cells laid out one after the other from index `cells`; the first further record of a cell carries n."""
    start = np.asarray(grid_start, np.uint32).astype(np.int64)
    glist = np.asarray(grid_list, np.uint32)
    counts = _block_major(np.diff(start))
    occupied = counts > 0
    words = np.packbits(occupied, axis=1, bitorder="little").view("<u8").reshape(BLOCKS).astype(np.uint64)
    per_block = occupied.sum(1, dtype=np.int64)
    rank = np.cumsum(per_block) - per_block
    b = np.arange(BLOCKS, dtype=np.int64)
    at = 3 * ((b & 63) | ((b >> 6) & 63) << 8 | (b >> 12) << 16)
    sparse = np.zeros(SPARSE_WORDS, np.uint32)
    sparse[at] = (words & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    sparse[at + 1] = (words >> np.uint64(32)).astype(np.uint32)
    sparse[at + 2] = rank.astype(np.uint32)
    dense = np.flatnonzero(occupied.ravel())                                   # block-major position of dense cell k
    cell = _block_major(np.arange(CELLS, dtype=np.uint32)).ravel()[dense].astype(np.int64)
    n = counts.ravel()[dense]
    s = start[cell]
    cells = len(dense)
    further = n - 1
    rest = cells + np.cumsum(further) - further
    tri = np.empty(len(glist), np.uint32)
    info = np.zeros(len(glist), np.uint32)
    tri[:cells] = glist[s]
    info[:cells] = (np.minimum(n, PAIR_MANY) | (rest << 4)).astype(np.uint32)
    owner = np.repeat(np.arange(cells, dtype=np.int64), further)             # the cell of each further record, in layout order
    i = np.arange(len(owner), dtype=np.int64) - np.repeat(rest - cells, further) + 1  # its index in the cell's list (1 .. n - 1)
    tri[cells:] = glist[s[owner] + i]
    info[cells:] = np.where(i == 1, n[owner], 0).astype(np.uint32)
    assert cells + len(owner) == len(glist) == start[-1]
    return dict(words=words, sparse=sparse, pair_rec=pair_words(tri_rec, tri, info), cells=cells)


def decode_cell(view, cx, cy, cz):
    """The triangle ids of cell (cx, cy, cz), in list order, read from view["sparse"] and view["pair_rec"] alone, the way a consumer of
    the view finds them: block entry at 3*((cx>>2) | (cy>>2)<<8 | (cz>>2)<<16), the cell's bit in the entry's word, dense id = rank +
    popcount(word below the bit), the first record's count word min(n, 15) | rest << 4, the exact count in the first further record
    when that field reads 15."""
    sparse, pairs = view["sparse"], view["pair_rec"]
    e = 3 * ((cx >> 2) | (cy >> 2) << 8 | (cz >> 2) << 16)
    word = int(sparse[e]) | int(sparse[e + 1]) << 32
    bit = (cx & 3) | (cy & 3) << 2 | (cz & 3) << 4
    if not (word >> bit) & 1:
        return []
    k = int(sparse[e + 2]) + bin(word & ((1 << bit) - 1)).count("1")
    count_word = int(pairs[k, 7])
    n, rest = count_word & 15, count_word >> 4
    if n == PAIR_MANY:
        n = int(pairs[rest, 7])
    return [int(pairs[k, 3])] + [int(t) for t in pairs[rest:rest + n - 1, 3]]


def cell_xyz(cell):
    return int(cell) & 255, (int(cell) >> 8) & 255, int(cell) >> 16


# ---------------------------------------------------------------------------------------------------------------
# the host loops of build_grid
# ---------------------------------------------------------------------------------------------------------------

def planes_of(box_min):
    """[257,4] sceneBoxMin -> [3,257] float32, one array of split planes per axis."""
    return np.ascontiguousarray(np.asarray(box_min, np.float32)[:, :3].T)


def cell_lut(planes):
    """[3,256] u8: per axis, the cell that holds the middle of the i-th of 256 equal steps across the grid's box -- lo + (i + 0.5) * step
    with step = (hi - lo) / 256 in float32; the cell only ever moves up, past every plane that lies below the point, and stops at 255."""
    planes = np.asarray(planes, np.float32)
    lut = np.zeros((3, 256), np.uint8)
    with np.errstate(all="ignore"):
        for w in range(3):
            pw = planes[w]
            lo, step = pw[0], (pw[GRID] - pw[0]) / np.float32(256)
            c = 0
            for i in range(256):
                x = lo + (np.float32(i) + np.float32(0.5)) * step
                while c < GRID - 1 and pw[c + 1] < x:
                    c += 1
                lut[w, i] = c
    return lut


def planes_tame(planes):
    """1 when every plane is 0 or has 2^-60 <= |p| <= 2^39, else 0."""
    m = np.abs(np.asarray(planes, np.float32))
    return int(np.all((m == 0) | ((m >= np.float32(2.0 ** -60)) & (m <= np.float32(2.0 ** 39)))))
