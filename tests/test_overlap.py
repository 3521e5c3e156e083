"""Which arrays the filters' device entry points refuse as overlapping (csrc/rt_overlap.h, rt_first_overlap), without a GPU: a table of
three arrays that are read and two that are written, 64 bytes each, as rtHipDenoiseDevice and its kin build them.  The refusal's text
names the pair this function reports, so the order "every entry x every written entry" is part of the contract."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

READS, WRITES, SIZE = (0, 1, 2), (3, 4), 64
BASE = [0x10000 + 0x1000 * i for i in range(5)]  # far apart: nothing overlaps


@pytest.fixture(scope="module")
def first_overlap(tmp_path_factory):
    """tests/overlap_host.cpp as a host library: first_overlap(addresses) -> (entry, written) or None."""
    out = tmp_path_factory.mktemp("overlap_host") / "liboverlap_host.so"
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-fPIC", "-shared", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "opencl_render_amd", "csrc"),
                    "-o", str(out), os.path.join(ROOT, "tests", "overlap_host.cpp")], check=True)
    lib = C.CDLL(str(out))
    lib.overlap_host.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def run(address, written=WRITES, size=SIZE):
        n = len(address)
        pair = (C.c_int * 2)(-1, -1)
        rc = lib.overlap_host(n, (C.c_uint64 * n)(*address), (C.c_uint64 * n)(*[size] * n), (C.c_int * n)(*[int(i in written) for i in range(n)]), pair)
        assert rc in (0, 1)
        return (pair[0], pair[1]) if rc else None

    return run


def moved(**where):
    """BASE with entry i at where["ei"]."""
    return [where.get(f"e{i}", a) for i, a in enumerate(BASE)]


def test_disjoint_and_adjacent_arrays_do_not_overlap(first_overlap):
    assert first_overlap(BASE) is None
    for w in WRITES:
        for r in READS:
            assert first_overlap(moved(**{f"e{w}": BASE[r] + SIZE})) is None, (w, r)  # starts where the read ends
            assert first_overlap(moved(**{f"e{w}": BASE[r] - SIZE})) is None, (w, r)  # ends where the read starts
    assert first_overlap(moved(e4=BASE[3] + SIZE)) is None and first_overlap(moved(e4=BASE[3] - SIZE)) is None
    assert first_overlap(moved(e1=BASE[0], e2=BASE[0])) is None  # arrays that are only read may share memory


def test_a_write_on_or_into_a_read_is_that_pair(first_overlap):
    for w in WRITES:
        for r in READS:
            for offset in (0, 4, -4, SIZE - 1, 1 - SIZE):  # equal, four bytes in from either side, one last byte shared
                assert first_overlap(moved(**{f"e{w}": BASE[r] + offset})) == (r, w), (w, r, offset)


def test_the_two_writes_on_each_other(first_overlap):
    for offset in (0, 4, -4):
        assert first_overlap(moved(e4=BASE[3] + offset)) == (3, 4), offset  # entry 3 against written entry 4 comes before 4 against 3


def test_an_optional_array_that_is_null_is_skipped(first_overlap):
    assert first_overlap(moved(e1=0)) is None
    assert first_overlap(moved(e1=0, e4=0)) is None  # an optional input and an optional output, both absent
    assert first_overlap(moved(e1=0, e3=32)) is None  # (a null entry has no byte range, whatever its size says)
    assert first_overlap(moved(e4=0, e3=BASE[2])) == (2, 3)  # the others are still checked


def test_of_two_overlaps_the_first_in_entry_times_written_order_is_reported(first_overlap):
    assert first_overlap(moved(e3=BASE[2], e4=BASE[0])) == (0, 4)  # entry 0 comes before entry 2
    assert first_overlap(moved(e3=BASE[0], e4=BASE[0] + 4)) == (0, 3)  # for one entry, written entry 3 comes before 4
    assert first_overlap(moved(e3=BASE[1], e4=BASE[1] + 4)) == (1, 3)
    assert first_overlap(moved(e3=BASE[2], e4=BASE[2] + 4)) == (2, 3)  # 2 x 3 before 2 x 4 and 3 x 4
    assert first_overlap(BASE, written=()) is None and first_overlap(moved(e1=BASE[0]), written=(1,)) == (0, 1)
