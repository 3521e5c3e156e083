"""The shading row as the device stores it (csrc/rt_device.h, triShade: one 128-byte line per triangle -- the 24 packed words, a copy of
quad 0 of the triangle's triRec record, four zero words), after every writer: the scene upload (rt_prepare_triangles), a geometry update into
either record set with and without new normals (rtg_records), a material-id edit (rte_store_ids) and a device-to-device clone.

T = 1, 3 and 257: 257 crosses a 256-thread block and leaves a partial one.  The yardstick of the packed words and of the records is
prep_oracle.triangle_records, a numpy restatement that knows nothing of the row's pitch; the row's own extra words are compared with the
device's tri_rec view, which the same restatement pins."""
import numpy as np
import pytest

import prep_oracle as P
from opencl_render_amd import raytrace as R, scene as S

pytestmark = pytest.mark.gpu

TWO_COLOURS = [dict(color=(200, 200, 200), reflection=(0, 0, 0), transparency=(0, 0, 0), bump=(0, 0, 0), luminance=(0, 0, 0)),
               dict(color=(220, 40, 30), reflection=(0, 0, 0), transparency=(0, 0, 0), bump=(0, 0, 0), luminance=(0, 0, 0))]


@pytest.fixture(autouse=True)
def fresh_tuning():
    R.tune("reset", 0)
    yield
    R.tune("reset", 0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_rows(rs, sc, vertex, normal, ids, label):
    """The four properties, for the shape (vertex, sc.tri_index), the corner normals and the material ids the scene should hold now."""
    T = sc.triangle_count
    rec, shade = P.triangle_records(vertex, sc.tri_index, ids, sc.tri_uv, normal)
    packed, row, dev_rec = rs.scene_view("tri_shade"), rs.scene_view("tri_shade_row"), rs.scene_view("tri_rec")
    assert packed.shape == (T, 24) and row.shape == (T, 32) and dev_rec.shape == (T, 16), label
    # (no float word is a NaN -- word 21 is the id's bits, no float -- so bit equality below is the whole comparison)
    assert not np.isnan(np.delete(shade, 21, axis=1)).any() and not np.isnan(rec[:, :4]).any(), label
    assert np.array_equal(bits(packed), bits(shade)), f"{label}: tri_shade differs from prep_oracle in rows {np.flatnonzero((bits(packed) != bits(shade)).any(1))[:4]}"
    assert np.array_equal(bits(dev_rec)[:, :4], bits(rec)[:, :4]), f"{label}: tri_rec quad 0 differs from prep_oracle"
    assert np.array_equal(bits(row)[:, :24], bits(packed)), f"{label}: words 0..23 of the stored row are not the packed view"
    assert np.array_equal(bits(row)[:, 24:28], bits(dev_rec)[:, 0:4]), f"{label}: words 24..27 are not quad 0 of the triangle's record"
    assert not bits(row)[:, 28:].any(), f"{label}: words 28..31 are not zero"
    if T >= 3:  # a range that starts inside the array: the packed view is gathered from the pitched rows
        part = rs.scene_view("tri_shade", 1, T - 2)
        assert np.array_equal(bits(part), bits(shade)[1:T - 1]), f"{label}: tri_shade[1:T-1]"
        assert np.array_equal(bits(rs.scene_view("tri_shade_row", T - 1, 1)), bits(row)[T - 1:]), f"{label}: tri_shade_row[T-1]"


@pytest.mark.parametrize("T", [1, 3, 257])
def test_every_writer_leaves_whole_rows(T):
    sc = S.make_soup(24, 16, T, 0.5, seed=900 + T, samples=1, materials=TWO_COLOURS, material_ids=(np.arange(T) % 2).astype(np.int32))
    R.build_lists(sc)
    v0, n0, ids0 = sc.vertex.copy(), sc.tri_normal.copy(), sc.tri_material.copy()
    scale = lambda f: np.concatenate([(v0[:, :3].astype(np.float64) * np.array(f)).astype(np.float32), v0[:, 3:]], 1)
    v1, v2, v3 = scale((1.25, 0.8, 1.1)), scale((0.9, 1.3, 1.0)), scale((1.1, 1.1, 0.7))
    n1 = n0.copy()
    n1[:, :3] = -n0[:, :3][:, ::-1]  # other corner normals in every row
    ids1 = np.where(np.arange(T) % 3 == 0, -1, 1 - ids0).astype(np.int32)
    assert not np.array_equal(ids1, ids0) and not np.array_equal(bits(n1), bits(n0)) and not np.array_equal(bits(v1), bits(v0))
    clones = []
    rs = R.ResidentScene(sc, 0)
    try:
        check_rows(rs, sc, v0, n0, ids0, f"T={T}, created")
        clones.append(R.ResidentScene(rs.scene, 0, like=rs))  # a copy of the parts the scene was created with
        check_rows(clones[-1], sc, v0, n0, ids0, f"T={T}, clone of the created scene")
        first_set = rs.pointers()[1]
        rs.set_vertices(v1, sc.tri_index, n1)  # into the first spare set, with new normals
        assert rs.pointers()[1] != first_set
        check_rows(rs, sc, v1, n1, ids0, f"T={T}, first update (new normals)")
        second_set = rs.pointers()[1]
        rs.set_vertices(v2)  # into the other set, the normals carried over from the rows in use
        assert rs.pointers()[1] != second_set
        check_rows(rs, sc, v2, n1, ids0, f"T={T}, second update (normals kept)")
        rs.set_materials(tri_material=ids1)
        check_rows(rs, sc, v2, n1, ids1, f"T={T}, material ids edited")
        rs.set_vertices(v3, None, n0)  # back into the set of the first update: ids from the edited rows, normals new
        assert rs.pointers()[1] == second_set
        check_rows(rs, sc, v3, n0, ids1, f"T={T}, third update (new normals, edited ids)")
        clones.append(R.ResidentScene(rs.scene, 0, like=rs))  # a copy of a record set of the updated scene
        check_rows(clones[-1], sc, v3, n0, ids1, f"T={T}, clone of the updated scene")
    finally:
        for c in clones:
            c.close()
        rs.close()
