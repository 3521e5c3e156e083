"""File input of the headless front-end (rt_fileio.cpp): OBJ / MTL, PPM / BMP, and the projected UVs of ShdProjectPoint
(reference source/render.cpp:495-673) against an independent numpy restatement.  Nothing of render.cpp compiles without the Maxon
SDK and the reference holds no fixtures: parity unpinned (libm acos / atan / sin / cos are this machine's)."""
import os

import numpy as np
import pytest

from conftest import ROOT
from opencl_render_amd import frontend as F, raytrace as R

DATA = os.path.join(ROOT, "tests", "data")


def test_obj_reader_gives_the_polygon_objects_the_front_end_takes():
    mesh, mats = F.read_obj(os.path.join(DATA, "scene.obj"))
    assert mesh.points.shape == (22, 3) and mesh.polygons.shape == (13, 4)     # 1 + 5 quads, 4 triangles, a pentagon fanned into 3
    assert [m["name"] for m in mats] == ["floor", "glass", "rough", "lamp"]     # in order of first use / definition
    pol = mesh.polygons
    assert pol[0].tolist() == [0, 1, 2, 3] and pol[1].tolist() == [4, 5, 6, 7]                   # quads keep a,b,c,d
    assert pol[6].tolist() == [12, 13, 16, 16] and pol[9].tolist() == [15, 12, 16, 16]           # triangles: c == d; negative indices resolved
    assert pol[10].tolist() == [17, 18, 19, 19] and pol[12].tolist() == [17, 20, 21, 21]         # the pentagon's fan
    assert mesh.polygon_material.tolist() == [0] + [1] * 5 + [2] * 4 + [3] * 3
    assert np.array_equal(mesh.corner_uv[0], np.float32([[0, 0], [3, 0], [3, 3], [0, 3]]))
    assert np.array_equal(mesh.corner_uv[6], np.float32([[0, 0], [3, 0], [0.5, 1], [0.5, 1]]))   # (vt 1, 2, 5; the triangle's 4th corner repeats the 3rd)
    assert np.array_equal(mesh.corner_uv[1], np.zeros((4, 2), np.float32))                       # a face without vt
    assert np.array_equal(mesh.corner_normals[0], np.float32([[0, 1, 0]] * 4)) and not mesh.corner_normals[1].any()
    floor, glass, rough, lamp = mats
    assert floor["color"].shape == (8, 8, 3) and tuple(np.float32(floor["rgb"])) == tuple(np.float32([0.8, 0.8, 0.7]))
    assert glass["transparency"].reshape(-1).tolist() == [153] * 3 and glass["reflection"].reshape(-1).tolist() == [77] * 3  # 1 - d, refl (0.3f * 255 = 76.500003)
    assert rough["bump"].shape == (4, 6, 3) and lamp["luminance"].reshape(-1).tolist() == [255, 229, 153]  # (0.9f * 255 = 229.49998)


def test_image_readers_ppm_and_bmp(tmp_path):
    tex = F.read_image(os.path.join(DATA, "checker.ppm"))
    raw = open(os.path.join(DATA, "checker.ppm"), "rb").read()
    assert tex.shape == (8, 8, 3) and tex.tobytes() == raw[-192:]
    assert tex[0, 0].tolist() == [255, 40, 40]
    bump = F.read_image(os.path.join(DATA, "bump.bmp"))
    assert bump.shape == (4, 6, 3) and (bump[:, :, 0] == bump[:, :, 1]).all()
    # a round trip through the library's own BMP writer (bottom-up rows, BGR, 4-byte row padding) and a plain PPM
    img = np.random.default_rng(1).integers(0, 256, (5, 7, 3), dtype=np.uint8)
    planes = [img[:, :, c].astype(np.uint16) * 256 for c in range(3)]
    F.write_bmp(str(tmp_path / "a.bmp"), *planes)
    assert np.array_equal(F.read_image(str(tmp_path / "a.bmp")), img)
    (tmp_path / "b.ppm").write_text("P3\n# plain\n2 1\n15\n15 0 3  1 2 15\n")
    assert F.read_image(str(tmp_path / "b.ppm")).tolist() == [[[255, 0, 51], [17, 34, 255]]]
    (tmp_path / "c.ppm").write_bytes(b"P6\n2 2\n255\n\x00\x01")  # truncated
    with pytest.raises(OSError):
        F.read_image(str(tmp_path / "c.ppm"))
    with pytest.raises(OSError):
        F.read_image(str(tmp_path / "missing.bmp"))


def _project_numpy(proj, p, n, ox, oy, lenx, leny, tile, start):
    """Independent restatement of ShdProjectPoint (render.cpp:495-673) in float64."""
    px, py, pz = (np.float64(v) for v in p)
    lenxinv = 1.0 / lenx if lenx != 0 else 0.0
    lenyinv = 1.0 / leny if leny != 0 else 0.0
    u, v = np.float64(start[0]), np.float64(start[1])
    sq = np.sqrt(px * px + pz * pz)
    wrap_u = None
    if proj == F.PROJ_VOLUMESHADER:
        return np.float32([px, py]), True
    if proj in (F.PROJ_FRONTAL, F.PROJ_UVW):
        pass
    elif proj == F.PROJ_SHRINKWRAP:
        if sq == 0:
            u, v = 0.0, (0.0 if py > 0 else 1.0)
        else:
            u = np.arccos(px / sq) / (2 * np.pi)
            if pz < 0: u = 1.0 - u
            v = 0.5 - np.arctan(py / sq) / np.pi
        sn, cs = np.sin(u * 2 * np.pi), np.cos(u * 2 * np.pi)
        u, v = (0.5 + 0.5 * cs * v - ox) * lenxinv, (0.5 + 0.5 * sn * v - oy) * lenyinv
    elif proj == F.PROJ_CYLINDRICAL:
        if sq == 0:
            u = 0.0
        else:
            u = np.arccos(px / sq) / (2 * np.pi)
            if pz < 0: u = 1.0 - u
            u -= ox
            if lenx > 0 and u < 0: u += 1.0
            elif lenx < 0 and u > 0: u -= 1.0
            u *= lenxinv
        v = -(py * 0.5 + oy) * lenyinv
    elif proj in (F.PROJ_FLAT, F.PROJ_SPATIAL):
        u, v = (px * 0.5 - ox) * lenxinv, -(py * 0.5 + oy) * lenyinv
    elif proj == F.PROJ_CUBIC:
        ax, ay, az = (abs(np.float64(c)) for c in n)
        axis = (0 if ax > az else 2) if ax > ay else (1 if ay > az else 2)
        if axis == 0:
            u = ((-pz if n[0] < 0 else pz) * 0.5 - ox) * lenxinv
            v = -(py * 0.5 + oy) * lenyinv
        elif axis == 1:
            v = ((pz if n[1] < 0 else -pz) * 0.5 - oy) * lenyinv
            u = (px * 0.5 - ox) * lenxinv
        else:
            u = ((px if n[2] < 0 else -px) * 0.5 - ox) * lenxinv
            v = -(py * 0.5 + oy) * lenyinv
    else:  # spherical and every unknown number
        if sq == 0:
            u, v = 0.0, (0.5 if py > 0 else -0.5)
        else:
            u = np.arccos(px / sq) / (2 * np.pi)
            if pz < 0: u = 1.0 - u
            u -= ox
            if lenx > 0 and u < 0: u += 1.0
            elif lenx < 0 and u > 0: u -= 1.0
            u *= lenxinv
            v = 0.5 + np.arctan(py / sq) / np.pi
        v = -(v - oy) * lenyinv
    return np.float32([u, v]), bool(tile or (0 <= u <= 1 and 0 <= v <= 1))


def test_projected_uvs_match_a_numpy_restatement():
    rng = np.random.default_rng(11)
    projs = [F.PROJ_SPHERICAL, F.PROJ_CYLINDRICAL, F.PROJ_FLAT, F.PROJ_CUBIC, F.PROJ_FRONTAL, F.PROJ_SPATIAL, F.PROJ_UVW, F.PROJ_SHRINKWRAP,
             F.PROJ_VOLUMESHADER, 99]
    points = [rng.uniform(-2, 2, 3) for _ in range(40)] + [np.array([0.0, 1.0, 0.0]), np.array([0.0, -2.0, 0.0]), np.array([1.0, 0.0, 0.0]),
                                                           np.array([-1.0, 0.3, -0.0]), np.array([0.5, 0.5, -1e-30])]
    worst = 0.0
    for proj in projs:
        for p in points:
            p = np.float32(p)
            n = np.float32(rng.uniform(-1, 1, 3))
            for ox, oy, lenx, leny, tile in [(0, 0, 1, 1, True), (0.25, -0.1, 0.5, 2.0, False), (0.9, 0.2, -1.0, 0.0, False), (0, 0, 0, 1, True)]:
                got, inside = F.project_uv(proj, p, n, (ox, oy), (lenx, leny), tile, start=(0.125, -7.0))
                want, want_inside = _project_numpy(proj, p, n, np.float32(ox), np.float32(oy), np.float32(lenx), np.float32(leny), tile, (0.125, -7.0))
                assert inside == want_inside, (proj, p, ox, oy, lenx, leny)
                # same formulas in double on both sides; only libm's last bit may differ before the cast to float
                assert np.allclose(got, want, rtol=0, atol=2e-7 * max(1.0, float(np.abs(want).max()))), (proj, p, got, want)
                worst = max(worst, float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))
    # the cubic projection follows the dominant axis of the normal, ties to the later axis (render.cpp:600-611)
    assert F.project_uv(F.PROJ_CUBIC, (1, 2, 3), (1, 1, 0))[0].tolist() == [0.5, -1.5]          # |x| > |y| fails -> y vs z -> y axis: v = -z/2
    assert F.project_uv(F.PROJ_CUBIC, (1, 2, 3), (0, 1, 1))[0].tolist() == [-0.5, -1.0]         # |y| > |z| fails -> z axis, v.z > 0
    assert F.project_uv(F.PROJ_FRONTAL, (1, 2, 3), (0, 0, 1), start=(0.25, 0.5))[0].tolist() == [0.25, 0.5]  # untouched, as in the reference


# ---- the readers whole: a valid corpus, a table of malformed files and random mutations (include/raytrace_hip.h, "FILE INPUT") -------
# tests/fileio_oracle.py is an independent reader written from the rules stated there; tests/fileio_cases.py makes the files.  Arrays,
# records and files are compared for equal bytes.  tests/fileio_host.cpp is the readers in a program of its own, built once as is and
# once under the address and undefined-behaviour sanitizers; no sanitizer is loaded into Python.
import ctypes as C
import subprocess

import fileio_cases as FC
import fileio_oracle as FO

FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", os.path.join(ROOT, "include"),
         "-I", os.path.join(ROOT, "opencl_render_amd", "csrc")]
SOURCES = [os.path.join(ROOT, "tests", "fileio_host.cpp"), os.path.join(ROOT, "opencl_render_amd", "csrc", "rt_fileio.cpp"),
           os.path.join(ROOT, "opencl_render_amd", "csrc", "rt_frontend.cpp")]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("fileio_corpus"))
    return root, FC.write_corpus(root)


def _lib_obj(path):
    """rtHipObjRead through ctypes -> (rc, the bytes of *out after the call, the arrays as fileio_oracle.obj_arrays lays them out)."""
    L = F._lib()
    d = F._ObjData()
    C.memset(C.byref(d), 0x5A, C.sizeof(d))
    rc = L.rtHipObjRead(path.encode(), C.byref(d))
    raw = bytes(d)
    if rc != 0:
        return rc, raw, None
    P, N, M = d.pointCount, d.polygonCount, d.materialCount
    at = lambda ptr, n: None if not ptr else C.string_at(ptr, n)
    arrays = dict(points=at(d.points, 16 * P), polygons=at(d.polygons, 16 * N), normals=at(d.cornerNormals, 64 * N), uv=at(d.cornerUv, 32 * N),
                  material=at(d.polygonMaterial, 4 * N), records=C.string_at(d.materials, C.sizeof(F._ObjMaterial) * M))
    L.rtHipObjFree(C.byref(d))
    assert bytes(d) == bytes(C.sizeof(d))
    return rc, raw, arrays


def _lib_image(path):
    """rtHipImageRead through ctypes -> (rc, width, height, pixels pointer value, the texels' bytes or None)."""
    L = F._lib()
    w, h, px = C.c_uint32(0x5A5A5A5A), C.c_uint32(0x5A5A5A5A), C.c_void_p(1)
    rc = L.rtHipImageRead(path.encode(), C.byref(w), C.byref(h), C.byref(px))
    if rc != 0:
        return rc, w.value, h.value, px.value, None
    data = C.string_at(px.value, 4 * w.value * h.value)
    R.lib().rtHipFree(px)
    return rc, w.value, h.value, px.value, data


def _same_material(got: dict, want: dict):
    assert set(got) == set(want)
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert isinstance(got[k], np.ndarray) and got[k].dtype == v.dtype and got[k].shape == v.shape and got[k].tobytes() == v.tobytes(), k
        elif k == "rgb":
            assert np.float32(got[k]).tobytes() == np.float32(v).tobytes()
        else:
            assert got[k] == v and type(got[k]) is type(v), k


def test_valid_objs_equal_the_reference_reader(corpus):
    root, files = corpus
    names = sorted(n for n in files if n.endswith(".obj"))
    assert len(names) >= 12
    seen = dict(none=0, uv=0, normals=0, unmapped=0)
    for name in names:
        path = os.path.join(root, name)
        want = FO.read_obj(path)
        rc, raw, got = _lib_obj(path)
        assert rc == 0, name
        exp = FO.obj_arrays(want)
        for k in exp:
            assert got[k] == exp[k], (name, k)
        mesh, mats = F.read_obj(path)
        assert mesh.points.dtype == np.float32 and mesh.points.tobytes() == want.points.tobytes(), name
        assert mesh.polygons.dtype == np.int32 and mesh.polygons.tobytes() == want.polygons.tobytes(), name
        assert mesh.polygon_material.tobytes() == want.polygon_material.tobytes(), name
        for a, b in ((mesh.corner_normals, want.corner_normals), (mesh.corner_uv, want.corner_uv)):
            assert (a is None) == (b is None) and (a is None or (a.shape == b.shape and np.ascontiguousarray(a).tobytes() == b.tobytes())), name
        want_mats = FO.material_dicts(want)
        assert len(mats) == len(want_mats), name
        for a, b in zip(mats, want_mats):
            _same_material(a, b)
        if len(want.polygons):
            vertex, tri_index, tri_material, tri_uv, tri_normal = F.mesh_arrays([mesh], (0.25, 0.5, -3.0))
            assert len(vertex) == len(want.points) and len(tri_index) == int(np.where(want.polygons[:, 2] != want.polygons[:, 3], 2, 1).sum())
        seen["none"] += want.corner_uv is None and want.corner_normals is None and len(want.polygons) > 0
        seen["uv"] += want.corner_uv is not None
        seen["normals"] += want.corner_normals is not None
        seen["unmapped"] += bool(len(want.polygons)) and bool((want.polygon_material == -1).any())
    assert all(seen.values()), seen
    # what the corpus is there to cover, stated on the reference reader's answers
    o = FO.read_obj(os.path.join(root, "blank_names.obj"))
    assert [m["name"] for m in o.materials] == [b"red brick", b"never defined", b"glass", b"lamp", b"maps", b"more\tmaps", b"defined only"]
    assert o.polygon_material.tolist() == [-1, 0, 0, 1, 2, 3, 4, 5]
    by = {m["name"]: m for m in o.materials}
    assert by[b"red brick"]["maps"][0] == os.path.join(root, "tex one.ppm").encode() and by[b"red brick"]["has_reflect"] == 1
    assert by[b"never defined"]["kd"] == [1, 1, 1] and by[b"never defined"]["dissolve"] == 1 and by[b"never defined"]["maps"] == [b""] * 5
    assert by[b"glass"]["dissolve"] == np.float32(0.75) and by[b"glass"]["reflect"] == np.float32(0.3)           # Tr after d
    assert by[b"lamp"]["dissolve"] == np.float32(0.875) and by[b"lamp"]["has_ke"] == 1                            # d after Tr
    assert all(by[b"maps"]["maps"]) and by[b"more\tmaps"]["maps"][3] == os.path.join(root, "bmp24_gap.bmp").encode()  # the last bump wins
    assert by[b"more\tmaps"]["maps"][4] == os.path.join(root, "tex one.ppm").encode() and not by[b"more\tmaps"]["maps"][0]  # absolute; map_kd is no keyword
    o = FO.read_obj(os.path.join(root, "layout.obj"))
    assert o.points.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0]] and o.polygons.tolist() == [[0, 1, 2, 2], [2, 1, 0, 0]]
    assert o.corner_uv[0].tolist() == [[0.25, 0.75], [0.5, 0], [0.25, 0.75], [0.25, 0.75]] and not o.corner_uv[1].any()
    o = FO.read_obj(os.path.join(root, "spellings.obj"))
    assert o.points[:2].tolist() == [[np.float32(1e-3), -0.5, 2.0], [100.0, 0.0, 5.0]] and o.points[2].tobytes() == np.float32([np.inf, -np.inf, np.nan]).tobytes()
    o = FO.read_obj(os.path.join(root, "ngon.obj"))
    assert o.polygons[:3].tolist() == [[0, 1, 2, 2], [0, 2, 3, 3], [0, 3, 4, 4]] and len(o.polygons) == 3 + 7 + 3
    assert o.polygons[3:10].tolist() == [[0, k, k + 1, k + 1] for k in range(1, 8)]


def test_valid_images_equal_the_reference_reader(corpus):
    root, files = corpus
    names = sorted(n for n in files if n.endswith((".ppm", ".bmp")))
    assert len(names) >= 27
    for name in names:
        path = os.path.join(root, name)
        want = FO.read_image(path)
        rc, w, h, px, data = _lib_image(path)
        assert rc == 0 and (h, w, 3) == want.shape and data == FO.image_bytes(want), name
        got = F.read_image(path)
        assert got.dtype == np.uint8 and got.shape == want.shape and got.tobytes() == want.tobytes(), name
    assert FO.read_image(os.path.join(root, "p6_1x6.ppm")).shape == (6, 1, 3) and FO.read_image(os.path.join(root, "p3_6x1.ppm")).shape == (1, 6, 3)
    assert set(np.unique(FO.read_image(os.path.join(root, "p3_6x1.ppm")))) <= {0, 255}                  # maxval 1
    assert set(np.unique(FO.read_image(os.path.join(root, "p6_comments.ppm")))) <= set(range(0, 256, 17))  # maxval 15


def _write_row(directory, name, data, others, tag=None):
    """One row of the malformed table as files; with a tag, under names of its own (several rows share a directory)."""
    stem, ext = os.path.splitext(name)
    for other, text in others.items():
        new = other if tag is None else tag + os.path.splitext(other)[1]
        data = data.replace(other.encode(), new.encode())
        with open(os.path.join(directory, new), "wb") as f:
            f.write(text)
    path = os.path.join(directory, name if tag is None else tag + ext)
    with open(path, "wb") as f:
        f.write(data)
    return path


def _refused(path, want_rc):
    if path.endswith(".obj"):
        rc, raw, arrays = _lib_obj(path)
        assert rc == want_rc and raw == bytes(len(raw)), (rc, raw[:16])
        with pytest.raises(OSError):
            F.read_obj(path)
        with pytest.raises(ValueError, match="malformed"):
            FO.read_obj(path)
    else:
        rc, w, h, px, data = _lib_image(path)
        assert (rc, w, h, px) == (want_rc, 0, 0, None)
        with pytest.raises(OSError):
            F.read_image(path)
        with pytest.raises(ValueError, match="malformed"):
            FO.read_image(path)


TABLE = FC.malformed_table()


@pytest.mark.parametrize("label,name,data,want_rc,others", TABLE, ids=[r[0] for r in TABLE])
def test_malformed_file_is_refused(tmp_path, label, name, data, want_rc, others):
    _refused(_write_row(str(tmp_path), name, data, others), want_rc)


def test_every_prefix_of_a_valid_file(tmp_path):
    accepted = dict(obj=0, ppm=0, bmp=0)
    for label, name, data, want_rc in FC.prefix_table():
        path = _write_row(str(tmp_path), name, data, {})
        if want_rc is None:  # an OBJ prefix: the reference reader decides
            try:
                want = FO.obj_arrays(FO.read_obj(path))
            except ValueError:
                want_rc = -2
        if want_rc == -2:
            _refused(path, -2)
            continue
        accepted[name[-3:]] += 1
        if name.endswith(".obj"):
            rc, raw, got = _lib_obj(path)
            assert rc == 0 and got == want, label
        else:
            rc, w, h, px, got = _lib_image(path)
            ref = FO.read_image(path)
            assert rc == 0 and (h, w, 3) == ref.shape and got == FO.image_bytes(ref), label
    assert accepted["ppm"] == 1 + 2 and accepted["bmp"] == 1 and 10 < accepted["obj"] < len(FC.PREFIX_OBJ)  # P3: with and without its last newline


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run([os.environ.get("CXX", "g++")] + extra + FLAGS + ["-o", str(out)] + SOURCES, check=True)
    return str(out)


def _run(program, directory, env=None):
    done = subprocess.run([program, directory], capture_output=True, text=True, env=env)
    assert done.returncode == 0 and done.stderr == "", (done.returncode, done.stderr[-4000:])
    out = {}
    for line in done.stdout.splitlines():
        f = line.split("\t")
        assert f[0] in ("obj", "img") and int(f[1]) in (0, -2), line
        out[f[-1]] = tuple(f[:-1])
    return out


def _expected_line(path):
    """What fileio_host prints for a file, from the reference reader."""
    hx = lambda b: "-" if b is None else "%016x" % FO.fnv1a(b)
    if path.endswith(".obj"):
        try:
            o = FO.read_obj(path)
        except ValueError:
            return ("obj", "-2", "0", "0", "0") + ("-",) * 6
        a = FO.obj_arrays(o)
        return ("obj", "0", str(len(o.points)), str(len(o.polygons)), str(len(o.materials)), hx(a["points"]), hx(a["polygons"]), hx(a["normals"]),
                hx(a["uv"]), hx(a["material"]), hx(a["records"]))
    try:
        img = FO.read_image(path)
    except ValueError:
        return ("img", "-2", "0", "0", "-")
    return ("img", "0", str(img.shape[1]), str(img.shape[0]), hx(FO.image_bytes(img)))


def _table_directory(tmp_path_factory):
    """The malformed table and the prefixes in one directory, each row under names of its own -> {file name: expected rc or None}."""
    root = str(tmp_path_factory.mktemp("fileio_table"))
    want = {}
    for i, (label, name, data, rc, others) in enumerate(TABLE):
        want[os.path.basename(_write_row(root, name, data, others, tag=f"row_{i:03d}"))] = rc
    for i, (label, name, data, rc) in enumerate(FC.prefix_table()):
        want[os.path.basename(_write_row(root, name, data, {}, tag=f"prefix_{i:04d}"))] = rc
    return root, want


def test_host_program_as_built_agrees_with_the_reference_reader(tmp_path_factory, corpus):
    root, files = corpus
    lines = _run(_build(tmp_path_factory, "fileio_host", ["-O2"]), root)
    names = [n for n in files if n.endswith((".obj", ".ppm", ".bmp"))]
    assert sorted(lines) == sorted(names)
    for n in names:
        assert lines[n] == _expected_line(os.path.join(root, n)) and lines[n][1] == "0", n


def test_host_program_under_address_and_undefined_sanitizers(tmp_path_factory, corpus):
    """The sanitized readers over the corpus, the malformed table with every prefix, and about 2000 seeded mutations of the corpus.  An
    allocation above 64 MB fails the run: a header must not size one before the file is looked at."""
    program = _build(tmp_path_factory, "fileio_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = dict(os.environ, ASAN_OPTIONS="max_allocation_size_mb=64")
    root, files = corpus
    lines = _run(program, root, env)
    for n in files:
        if n.endswith((".obj", ".ppm", ".bmp")):
            assert lines[n] == _expected_line(os.path.join(root, n)) and lines[n][1] == "0", n
    table, want = _table_directory(tmp_path_factory)
    lines = _run(program, table, env)
    assert sorted(lines) == sorted(want)
    for n, rc in want.items():
        assert lines[n] == _expected_line(os.path.join(table, n)), n
        assert rc is None or lines[n][1] == str(rc), n
    mutated = str(tmp_path_factory.mktemp("fileio_mutations"))
    FC.write_corpus(mutated)
    count = FC.write_mutations(mutated, files)
    assert count >= 1900
    lines = _run(program, mutated, env)  # (exit status 0, nothing on stderr, every rc 0 or -2; the program checks what it accepts)
    got = [v for k, v in lines.items() if k.startswith("mut_")]
    assert len(got) == count
    for n, v in lines.items():  # what it accepts, and what it refuses, is what the reference reader accepts and refuses
        assert v == _expected_line(os.path.join(mutated, n)), n
    assert 0.1 * count < sum(v[1] == "0" for v in got) < 0.9 * count  # the mutations reach both sides of the rules


# ---- the pass sinks: PGM, PFM and colour PFM against bytes rebuilt here ----------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (7, 1), (5, 3)])
def test_pass_sinks_round_trip(tmp_path, w, h):
    rng = np.random.default_rng(100 * w + h)
    plane = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    plane.flat[0] = 65535
    F.write_pgm(str(tmp_path / "a.pgm"), plane)
    assert (tmp_path / "a.pgm").read_bytes() == b"P5\n%d %d\n255\n" % (w, h) + (plane >> 8).astype(np.uint8).tobytes()
    special = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x7FA00000], np.uint32)  # NaNs (one signalling), +-inf, -0.0, a denormal
    depth = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32)
    depth.flat[:len(special)] = special[:depth.size]
    F.write_pfm(str(tmp_path / "a.pfm"), depth.view(np.float32))
    assert (tmp_path / "a.pfm").read_bytes() == b"Pf\n%d %d\n-1.0\n" % (w, h) + depth[::-1].astype("<u4").tobytes()
    rgb = rng.integers(0, 2 ** 32, (h, w, 3), dtype=np.uint32)
    rgb.reshape(-1)[-min(len(special), rgb.size):] = special[:min(len(special), rgb.size)]
    F.write_pfm_rgb(str(tmp_path / "b.pfm"), rgb.view(np.float32))
    assert (tmp_path / "b.pfm").read_bytes() == b"PF\n%d %d\n-1.0\n" % (w, h) + rgb[::-1].astype("<u4").tobytes()
