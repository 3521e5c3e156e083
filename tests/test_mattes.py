"""Mattes without a GPU: the numpy restatement (matte_oracle.py) against hand-written id rows with known answers, every refusal of
rtHipMatteCheck and its acceptance at the legal edges, the C ABI's declarations, binding and exports, and the command-line flags.  The
device is checked against the same restatement in test_mattes_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import matte_oracle as MO
from conftest import ROOT
from opencl_render_amd import __main__ as cli
from opencl_render_amd import raytrace as R

NONE = MO.NONE
F32 = np.float32
NEW_SYMBOLS = ["rtHipMatteCheck", "rtHipMatteDefaults", "rtHipSceneSetMatteGroups", "rtHipSceneMattes", "rtHipSceneMattesDevice",
               "rtHipSceneMatteTimes"]


def rows(*r):
    return np.array(r, np.uint32)


def test_first_appearance_insertion_and_ranking():
    # 7 first, then 3 three times, then 9 twice: all fit K = 3; ranked by count, so 3 (3), 9 (2), 7 (1)
    m = MO.mattes(rows([7, 3, 3, 9, 3, 9]), None, [], 3, 6)
    assert m["layer_id"][:, 0].tolist() == [3, 9, 7]
    assert m["layer_count"][:, 0].tolist() == [3, 2, 1]
    assert m["rest_count"].tolist() == [0]
    assert np.array_equal(m["layer_coverage"][:, 0], np.array([3, 2, 1], F32) / F32(6))
    assert m["layer_coverage"].dtype == F32 and m["layer_id"].dtype == np.uint32 and m["rest"].dtype == F32


def test_overflow_keeps_the_first_k_distinct_ids_not_the_largest():
    # K = 2 keeps 7 and 3 (first two in sample order); 9 covers most of the pixel and still goes to rest
    m = MO.mattes(rows([7, 3, 9, 9, 9, 9, 3, 9]), None, [], 2, 8)
    assert m["layer_id"][:, 0].tolist() == [3, 7]
    assert m["layer_count"][:, 0].tolist() == [2, 1]
    assert m["rest_count"].tolist() == [5]
    assert m["rest"][0] == F32(5) / F32(8)
    exact = MO.mattes(rows([7, 3, 9, 9, 9, 9, 3, 9]), None, [], 8, 8)
    assert exact["layer_id"][:, 0].tolist() == [9, 3, 7] + [NONE] * 5 and exact["rest_count"].tolist() == [0]
    assert exact["layer_count"][:, 0].tolist() == [5, 2, 1, 0, 0, 0, 0, 0]


def test_count_ties_are_broken_by_id_ascending():
    m = MO.mattes(rows([50, 4, 50, 4, 20, 20]), None, [], 4, 6)
    assert m["layer_id"][:, 0].tolist() == [4, 20, 50, NONE]
    assert m["layer_count"][:, 0].tolist() == [2, 2, 2, 0]
    big = MO.mattes(rows([0xFFFFFFFE, 0, 0xFFFFFFFE, 0]), None, [], 2, 4)  # ids are compared as unsigned
    assert big["layer_id"][:, 0].tolist() == [0, 0xFFFFFFFE]


def test_none_is_skipped_and_takes_no_slot():
    m = MO.mattes(rows([NONE, 5, NONE, NONE], [NONE] * 4), None, [5, 6], 1, 4)
    assert m["layer_id"][0].tolist() == [5, NONE] and m["layer_count"][0].tolist() == [1, 0]
    assert m["rest_count"].tolist() == [0, 0] and m["none_count"].tolist() == [3, 4]
    assert m["select"][:, 0].tolist() == [0.25, 0.0] and m["select"][:, 1].tolist() == [0.0, 0.0]


def test_selected_counts_with_a_repeated_id_and_a_table():
    ids = rows([0, 1, 2, 3], [3, 3, NONE, 0])
    table = np.array([10, 10, 11, NONE], np.uint32)  # triangles 0, 1 -> group 10, 2 -> 11, 3 in no group
    m = MO.mattes(ids, table, [10, 11, 10, 12], 2, 4)
    assert m["select"][:, 0].tolist() == [0.5, 0.25, 0.5, 0.0]
    assert m["select"][:, 1].tolist() == [0.25, 0.0, 0.25, 0.0]
    assert m["layer_id"][:, 0].tolist() == [10, 11] and m["layer_id"][:, 1].tolist() == [10, NONE]
    assert m["none_count"].tolist() == [1, 3]
    assert MO.material_table([2, -1, 0, -7]).tolist() == [2, NONE, 0, NONE]


def test_conservation_law_on_random_rows():
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 6, (200, 12)).astype(np.uint32)
    ids[rng.random(ids.shape) < 0.3] = NONE
    for K in (0, 1, 2, 5, 8):
        m = MO.mattes(ids, None, [0, 1], K, 12)
        total = m["layer_count"].sum(0).astype(np.int64) + m["rest_count"] + m["none_count"]
        assert np.array_equal(total, np.full(200, 12)), K
        if K >= 6:
            assert not m["rest_count"].any()
        if K == 0:
            assert np.array_equal(m["rest_count"], 12 - m["none_count"])
    assert MO.distinct_histogram(rows([1, 1, NONE], [NONE] * 3, [1, 2, 3])) == [1, 1, 0, 1]


def params(**kw):
    p = R.MatteParams(kind=0, total=8, first=0, samples=8, selectCount=0, layers=4)
    for k, v in kw.items():
        if k == "select":
            p.selectCount = len(v)
            for i, s in enumerate(v):
                p.select[i] = s
        else:
            setattr(p, k, v)
    return p


@pytest.mark.parametrize("bad, text", [
    (dict(kind=3), "kind"), (dict(kind=0xFFFFFFFF), "kind"), (dict(total=0, first=0, samples=1), "total"),
    (dict(samples=0), "samples"), (dict(samples=65537, total=1 << 20), "samples"),
    (dict(total=8, first=1, samples=8), "total"), (dict(total=0xFFFFFFFF, first=0xFFFFFFFF, samples=1), "total"),
    (dict(total=0xFFFFFFFF, first=0xFFFFFFF0, samples=65536), "total"),  # f + C wraps in 32 bits
    (dict(selectCount=17), "selectCount"), (dict(layers=9), "layers"), (dict(selectCount=0, layers=0), "neither"),
    (dict(select=[1, NONE]), "select[1]"),
])
def test_matte_check_refuses(hip_lib, bad, text):
    assert hip_lib.rtHipMatteCheck(C.byref(params(**bad))) == -1
    assert text in R.last_error(), R.last_error()


@pytest.mark.parametrize("good", [
    dict(), dict(samples=65536, total=65536), dict(total=100, first=92, samples=8), dict(total=0xFFFFFFFF, first=0xFFFFFFFF - 8, samples=8),
    dict(total=0xFFFFFFFF, first=0, samples=1), dict(select=list(range(16)), layers=0), dict(layers=8), dict(select=[5, 5], layers=8),
    dict(kind=1), dict(kind=2), dict(select=[0xFFFFFFFE], layers=0), dict(total=1, first=0, samples=1),
])
def test_matte_check_accepts_the_legal_edges(hip_lib, good):
    assert hip_lib.rtHipMatteCheck(C.byref(params(**good))) == 0, R.last_error()


def test_null_arguments_are_refused_without_a_device(hip_lib):
    p = params()
    out = np.zeros(4, F32)
    ptr = out.ctypes.data_as(C.c_void_p)
    assert hip_lib.rtHipMatteCheck(None) == -1 and "null" in R.last_error()
    assert hip_lib.rtHipMatteDefaults(None, C.byref(p)) == -1
    assert hip_lib.rtHipSceneSetMatteGroups(None, ptr, 0) == -1
    assert hip_lib.rtHipSceneMattes(None, C.byref(p), None, ptr, ptr, ptr) == -1 and "null" in R.last_error()
    assert hip_lib.rtHipSceneMattesDevice(None, C.byref(p), None, ptr, ptr, ptr, None) == -1
    assert hip_lib.rtHipSceneMatteTimes(None, None) == -1


def test_header_declares_the_matte_entry_points_and_the_library_exports_them(hip_lib):
    text = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in R.RESIDENT_SYMBOLS
        assert hasattr(hip_lib, name), f"libraytrace_hip.so does not export {name}"
    assert "MATTES" in text
    for name, value in (("RT_HIP_MATTE_TRIANGLE", 0), ("RT_HIP_MATTE_MATERIAL", 1), ("RT_HIP_MATTE_GROUP", 2)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", text), name
    assert R.MATTE_KINDS == dict(triangle=0, material=1, group=2)
    assert C.sizeof(R.MatteParams) == 4 * (5 + 16 + 1)
    assert [f[0] for f in R.MatteParams._fields_] == ["kind", "total", "first", "samples", "selectCount", "select", "layers"]
    for method in ("set_matte_groups", "mattes", "matte_times_ms"):
        assert callable(getattr(R.ResidentScene, method))


def test_matte_chunk_is_a_tuning_key_with_legal_range(hip_lib):
    try:
        for v in (1, 3, 64, 65536):
            R.tune("matte_chunk", v)
        for v in (0, -1, 65537, float("nan")):
            with pytest.raises(ValueError, match="matte_chunk"):
                R.tune("matte_chunk", v)
    finally:
        R.tune("reset", 0)


def test_command_line_flags_parse(capsys):
    args = cli.parse_args(["--mattes", "out/m", "--matte-kind", "material", "--matte-select", "3,0x10,7", "--matte-layers", "8"])
    assert (args.mattes, args.matte_kind, args.matte_select, args.matte_layers) == ("out/m", "material", (3, 16, 7), 8)
    d = cli.parse_args(["--mattes", "m"])
    assert (d.matte_kind, d.matte_select, d.matte_layers) == ("mesh", (), 4)
    assert cli.parse_args([]).mattes is None
    for bad in (["--matte-layers", "2"], ["--mattes", "m", "--matte-layers", "9"], ["--mattes", "m", "--matte-layers", "0"],
                ["--mattes", "m", "--orbit", "3"], ["--mattes", "m", "--matte-select", "1,x"], ["--mattes", "m", "--matte-kind", "group"],
                ["--mattes", "m", "--matte-select", "4294967295"], ["--mattes", "m", "--matte-select", ",".join(["1"] * 17)]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    capsys.readouterr()
