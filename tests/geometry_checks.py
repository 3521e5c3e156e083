"""Checks of a resident scene after a geometry update, shared by tests/test_geometry_move_gpu.py and the session tests
(tests/session_cases.py): the update that hands over only what differs, and the device arrays against prep_oracle's restatements."""
import numpy as np

import prep_oracle as P


def update_to(rs, want):
    """The update that makes `want` resident: the index array and the normals are handed over only where they differ from what the scene
    holds (or nothing is retained yet), so the NULL forms of both run wherever they are legal."""
    log = rs.geometry_log()
    first = log["thread"] + log["group"] == 0 and want.triangle_count > 0
    idx = want.tri_index if first or rs.scene.tri_index.tobytes() != want.tri_index.tobytes() else None
    nrm = want.tri_normal if rs.scene.tri_normal.tobytes() != want.tri_normal.tobytes() else None
    rs.set_vertices(want.vertex, idx, nrm)
    return idx is None, nrm is None


def prep_of(want):
    """prep_oracle's (records, shading records, dense view) of a Scene with a grid: what assert_device_arrays compares with.  They
    depend on the shape and its grid alone, so a caller that checks one shape many times may make them once."""
    rec, shade = P.triangle_records(want.vertex, want.tri_index, want.tri_material, want.tri_uv, want.tri_normal)
    return rec, shade, P.dense_view(want.grid_start, want.grid_list, rec)


def assert_device_arrays(rs, want, label, prep=None):
    """TRI_REC, TRI_SHADE, GRID_BITS, BLOCK_SPARSE, PAIR_REC, CELL_LUT and the header equal prep_oracle's for the oracle grid (prep:
    prep_of(want), where the caller has made it already)."""
    if want.triangle_count == 0:  # (prep_oracle.triangle_records does not take an empty scene)
        assert rs.scene_header()["pair_count"] == 0 == len(want.grid_list) and not rs.scene_view("grid_bits").any(), label
        return
    rec, shade, view = prep if prep is not None else prep_of(want)
    for name, got, exp in (("tri_rec", rs.scene_view("tri_rec"), rec), ("tri_shade", rs.scene_view("tri_shade"), shade)):
        assert got.shape == exp.shape, (label, name)
        rows = np.flatnonzero(~P.same_float_words(got, exp).all(1))
        assert rows.size == 0, f"{label}: {name} differs in {rows.size} rows, first {rows[:4]}"
    assert np.array_equal(rs.scene_view("grid_bits"), view["words"]), f"{label}: gridBits"
    assert np.array_equal(rs.scene_view("block_sparse"), view["sparse"]), f"{label}: gridBlockSparse"
    pr, wr = rs.scene_view("pair_rec"), view["pair_rec"]
    assert pr.shape == wr.shape, f"{label}: {pr.shape[0]} pair records, the oracle grid has {wr.shape[0]}"
    ids = [3, 7]
    floats = [i for i in range(16) if i not in ids]
    if not np.array_equal(pr, wr):  # (records equal in every bit pass both; the column copies below take seconds on millions of pairs)
        assert np.array_equal(pr[:, ids], wr[:, ids]), f"{label}: pair order or count words"
        assert P.same_float_words(pr[:, floats].view(np.float32), wr[:, floats].view(np.float32)).all(), f"{label}: pair record floats"
    planes = P.planes_of(want.box_min)
    assert np.array_equal(rs.scene_view("cell_lut"), np.asarray(P.cell_lut(planes)).reshape(-1)), f"{label}: cellLut"
    h = rs.scene_header()
    assert h["planes_tame"] == P.planes_tame(planes) and h["triangle_count"] == want.triangle_count and h["pair_count"] == len(want.grid_list), (label, h)
