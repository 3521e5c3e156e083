"""The MATTES definition of include/raytrace_hip.h restated on the host (test infrastructure only).

``sample_ids``  the primary-hit triangle of every sample of every pixel: the oracle's generator and rt_oracle_ray_triangle over the scene's
                camera lists -- the loop of surface_definition in test_surface_passes_gpu.py without the shading.  The ctypes loop is the
                slow part: compute it once per scene and derive every variant from it.
``mattes``      the four outputs in numpy from those ids and a table that maps a triangle to its id for the kind.
"""
import ctypes as C

import numpy as np

import oracle_lib as O

NONE = 0xFFFFFFFF
F32 = np.float32


def sample_ids(sc, N, f, C_):
    """[H*W, C] uint32: the triangle sample j = 0..C-1 (sample id f + 1 + j, seed p*N + id) of pixel p hits first, NONE on a miss."""
    L = O.oracle()
    f3 = C.c_float * 3
    W, H = sc.width, sc.height
    eye_c = f3(*[float(v) for v in np.asarray(sc.eye, F32)[:3]])
    tl, lr, tb = (np.asarray(v, F32)[:3] for v in (sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom))
    verts = {}

    def tri_verts(t):
        if t not in verts:
            verts[t] = [f3(*[float(c) for c in sc.vertex[int(i)][:3]]) for i in sc.tri_index[t][:3]]
        return verts[t]

    ids = np.full((H * W, C_), NONE, np.uint32)
    t, l1, l2 = C.c_float(), C.c_float(), C.c_float()
    for p in range(H * W):
        cands = [int(c) for c in sc.cam_list[int(sc.cam_start[p]):int(sc.cam_end[p])]]
        if not cands:
            continue
        x, y = p % W, p // W
        for j in range(C_):
            state = C.c_uint64(p * N + f + 1 + j)
            kx = F32(x) + F32(L.rt_oracle_randf(C.byref(state), 0.0, 1.0))
            ky = F32(y) + F32(L.rt_oracle_randf(C.byref(state), 0.0, 1.0))
            d = tl + lr * kx
            d = d + tb * ky
            dc = f3(*[float(v) for v in d])
            best, best_t = NONE, float("inf")
            for c in cands:
                if L.rt_oracle_ray_triangle(eye_c, dc, 0.0, best_t, *tri_verts(c), C.byref(t), C.byref(l1), C.byref(l2)):
                    best, best_t = c, t.value
            ids[p, j] = best
    return ids


def table_ids(ids, table):
    """The samples' ids for a kind: table[triangle] (a u32 per triangle; None = the triangle itself), NONE where the sample missed."""
    if table is None:
        return ids
    table = np.asarray(table, np.uint32)
    hit = ids != NONE
    out = np.full(ids.shape, NONE, np.uint32)
    out[hit] = table[ids[hit]]
    return out


def material_table(tri_material):
    """Kind MATERIAL's table: every negative id reads as NONE."""
    m = np.asarray(tri_material, np.int64)
    return np.where(m < 0, NONE, m).astype(np.uint32)


def pixel_layers(row, K):
    """One pixel's samples in order -> (slots [(id, count)] in insertion order, rest, none): the definition, literally."""
    slots, rest, none = [], 0, 0
    for g in (int(v) for v in row):
        if g == NONE:
            none += 1
            continue
        for s in slots:
            if s[0] == g:
                s[1] += 1
                break
        else:
            if len(slots) < K:
                slots.append([g, 1])
            else:
                rest += 1
    return slots, rest, none


def mattes(ids, table, select, K, C_, shape=None):
    """{"select" [M, P] f32, "layer_id" [K, P] u32, "layer_coverage" [K, P] f32, "rest" [P] f32, and the integer "layer_count" [K, P],
    "rest_count" [P], "none_count" [P]} for ids [P, C]; with shape = (H, W) the planes are reshaped to [.., H, W]."""
    g = table_ids(np.asarray(ids, np.uint32), table)
    P = g.shape[0]
    assert g.shape[1] == C_
    den = F32(C_)
    sel = np.stack([(g == np.uint32(s)).sum(1) for s in select]).astype(np.uint32) if len(select) else np.zeros((0, P), np.uint32)
    lid = np.full((K, P), NONE, np.uint32)
    lcnt = np.zeros((K, P), np.uint32)
    rest = np.zeros(P, np.uint32)
    none = (g == NONE).sum(1).astype(np.uint32)
    for p in np.flatnonzero(none < C_):
        slots, rest[p], _ = pixel_layers(g[p], K)
        slots.sort(key=lambda s: (-s[1], s[0]))
        for k, (i, c) in enumerate(slots):
            lid[k, p], lcnt[k, p] = i, c
    out = dict(select=sel.astype(F32) / den, layer_id=lid, layer_coverage=lcnt.astype(F32) / den, rest=rest.astype(F32) / den,
               layer_count=lcnt, rest_count=rest, none_count=none)
    if shape is not None:
        out = {k: v.reshape(v.shape[:-1] + tuple(shape)) for k, v in out.items()}
    return out


def distinct_histogram(ids):
    """How many pixels have 0, 1, 2, .. distinct ids among their samples (NONE not counted)."""
    n = np.array([len(set(int(v) for v in row if v != NONE)) for row in ids])
    return np.bincount(n).tolist()
