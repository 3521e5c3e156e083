"""The owner types of csrc/rt_owned.h (device block, event, pinned block, stream), without a GPU: tests/owned_host.cpp defines the HIP
calls the header makes as counting stand-ins over malloc, one of which can be told to fail its N-th call, and exports the scenarios
driven here.  What a scene's rtHipSceneBytes and its teardown rest on: every owner frees exactly once, make / drop / fit move the running
total by exactly the block's bytes, and a growth that fails leaves the old block, its size and the total alone.  The second half is
DevPart, the list of blocks a scene part (or scratch) is: its sum, a failed add, moves, adopt, and the scene's install / drop_part
modelled on a small struct; the file's own program walks every scenario once more under the address and undefined sanitizers."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

DEVICE, EVENT, PINNED, STREAM = KINDS = (0, 1, 2, 3)
HELD = 4096


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("owned_host") / "libowned_host.so"
    rocm = os.environ.get("ROCM", os.environ.get("ROCM_PATH", "/opt/rocm"))
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-fPIC", "-shared", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", os.path.join(ROOT, "opencl_render_amd", "csrc"), "-o", str(out), os.path.join(ROOT, "tests", "owned_host.cpp")], check=True)
    L = C.CDLL(str(out))
    L.owned_fail.argtypes = [C.c_int, C.c_uint64]
    L.owned_make_drop.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    L.owned_fit.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    L.owned_part_fill.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
    L.owned_part_adopt.argtypes = [C.c_uint64, C.POINTER(C.c_uint64)]
    L.owned_scene_handover.argtypes = [C.c_uint64, C.POINTER(C.c_uint64)]
    L.owned_scene_grow.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    return L


def counts(lib):
    """(made per kind, gone per kind, live, bad frees, when the last device block was allocated, when the last one was freed)"""
    o = (C.c_uint64 * 12)()
    lib.owned_counts(o)
    return list(o[0:4]), list(o[4:8]), o[8], o[9], o[10], o[11]


def settled(lib):
    """everything made has been released, once"""
    made, gone, live, bad, _, _ = counts(lib)
    return made == gone and live == 0 and bad == 0


@pytest.mark.parametrize("kind", KINDS)
def test_going_out_of_scope_frees_once_and_an_empty_owner_frees_nothing(lib, kind):
    lib.owned_reset()
    assert lib.owned_scope(kind, 0) == 0
    assert counts(lib)[:4] == ([0] * 4, [0] * 4, 0, 0)
    lib.owned_reset()
    assert lib.owned_scope(kind, 1) == 0
    made, gone, live, bad, _, _ = counts(lib)
    assert made[kind] == 1 and gone[kind] == 1 and sum(made) == 1 and live == 0 and bad == 0


@pytest.mark.parametrize("kind", KINDS)
def test_a_moved_from_owner_is_empty_and_assignment_frees_what_was_held(lib, kind):
    lib.owned_reset()
    o = (C.c_uint64 * 7)()
    lib.owned_move(kind, o)
    assert o[0] == 1 and o[1] == 1, "move construction: the source is empty, the target holds its handle"
    assert o[2] == 1 and o[3] == 1 and o[4] == 1, "move assignment: the held one is freed there and then, the source is empty"
    if kind == DEVICE:
        assert o[5] == 0 and o[6] == 48  # the size travels with the pointer
    assert counts(lib)[0][kind] == 2 and settled(lib)


def test_make_and_drop_count_the_blocks_bytes_and_the_destructor_counts_nothing(lib):
    lib.owned_reset()
    o = (C.c_uint64 * 5)()
    assert lib.owned_make_drop(96, 500, o) == 0
    assert (o[0], o[1], o[3], o[4]) == (596, 500, 96, 1)
    assert o[2] == 596, "a block that is destroyed without a drop leaves the total alone"
    assert settled(lib)


FIT_CASES = [(HELD, need, exact) for need in (HELD - 1, HELD, HELD + 1) for exact in (0, 1)] + [(0, 0, 0), (0, 0, 1)]


@pytest.mark.parametrize("held,need,exact", FIT_CASES)
def test_fit_keeps_or_replaces_allocating_first(lib, held, need, exact):
    keep = held > 0 and held >= need
    want = max(need if exact else need + need // 8, 64)
    lib.owned_reset()
    o = (C.c_uint64 * 4)()
    assert lib.owned_fit(held, need, exact, o) == 0
    made, gone, _, _, last_made, last_gone = counts(lib)
    assert o[3] == want
    if keep:
        assert (o[0], o[1], o[2]) == (1, held, 1000 + held) and made[DEVICE] == 1
    else:
        assert (o[0], o[1], o[2]) == (0, want, 1000 + want), "replaced: the total moved by new - old"
        assert made[DEVICE] == (2 if held else 1)
        if held:
            assert last_made < last_gone, "the new block is allocated before the old one is freed"
    assert settled(lib)
    # the same with the growth's allocation failing: the old block, its size and the total stay
    lib.owned_reset()
    lib.owned_fail(DEVICE, 2 if held else 1)
    rc = lib.owned_fit(held, need, exact, o)
    if keep:
        assert rc == 0
    else:
        assert rc != 0 and (o[0], o[1], o[2]) == (1, held, 1000 + held)
    assert settled(lib)


@pytest.mark.parametrize("kind", KINDS)
def test_a_failed_make_leaves_the_owner_empty(lib, kind):
    lib.owned_reset()
    lib.owned_fail(kind, 1)
    assert lib.owned_scope(kind, 1) != 0
    assert counts(lib)[:4] == ([0] * 4, [0] * 4, 0, 0)


def test_a_failed_make_leaves_the_total_unchanged(lib):
    lib.owned_reset()
    lib.owned_fail(DEVICE, 1)
    o = (C.c_uint64 * 5)()
    assert lib.owned_make_drop(96, 500, o) != 0
    assert (o[0], o[1], o[3]) == (500, 500, 0) and settled(lib)


@pytest.mark.parametrize("kind,nth", [(DEVICE, n) for n in (0, 1, 2, 3, 5)] + [(EVENT, n) for n in (1, 4)])
def test_a_compound_build_that_fails_part_way_frees_what_it_made(lib, kind, nth):
    """one block, four blocks, four events, then the hand-over -- rtHipSceneSetCamera's first call"""
    lib.owned_reset()
    lib.owned_fail(kind, nth)
    o = (C.c_uint64 * 3)()
    rc = lib.owned_compound(o)
    made, gone, live, bad, _, _ = counts(lib)
    if nth == 0:
        assert rc == 0 and tuple(o) == (4096 + 4 * 256, 5, 4) and made[DEVICE] == 5 and made[EVENT] == 4
    else:
        assert rc != 0 and tuple(o) == (0, 0, 0), "nothing is handed over and nothing is counted"
        assert made[DEVICE] == (nth - 1 if kind == DEVICE else 5) and made[EVENT] == (0 if kind == DEVICE else nth - 1)
    assert made == gone and live == 0 and bad == 0, "as many frees as successful allocations, for blocks and for events"


# ---- DevPart: the blocks of a scene part, or of scratch, and their byte sum -----------------------------------------------------

def part_block(i):
    return 16 * (i + 1)


def part_sum(n):
    return sum(part_block(i) for i in range(n))


@pytest.mark.parametrize("k", [0, 1, 4])
def test_a_part_going_out_of_scope_frees_each_block_once_and_an_empty_part_frees_nothing(lib, k):
    lib.owned_reset()
    o = (C.c_uint64 * 5)()
    assert lib.owned_part_fill(k, o) == 0
    assert (o[0], o[1], o[2], o[3]) == (k, part_sum(k), k, 1), "k blocks in creation order, the sum is their bytes"
    made, gone, live, bad, _, _ = counts(lib)
    assert made[DEVICE] == k and gone[DEVICE] == k and sum(made) == k and live == 0 and bad == 0


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_an_add_that_fails_leaves_the_part_as_it_was(lib, n):
    """block n of 4 cannot be made: the n - 1 earlier blocks and the sum stay, and all of them go at scope end"""
    lib.owned_reset()
    lib.owned_fail(DEVICE, n)
    o = (C.c_uint64 * 5)()
    assert lib.owned_part_fill(4, o) != 0
    assert (o[0], o[1], o[2]) == (n - 1, part_sum(n - 1), n - 1)
    assert o[3] == 1, "the earlier blocks kept pointer and size"
    assert o[4] == 1, "the failed add handed out no pointer"
    assert counts(lib)[0][DEVICE] == n - 1 and settled(lib)


def test_a_moved_from_part_is_empty_with_sum_zero(lib):
    lib.owned_reset()
    o = (C.c_uint64 * 6)()
    lib.owned_part_move(o)
    assert o[0] == 1 and o[1] == part_sum(3), "move construction: the source is empty, sum 0; the target has blocks and sum"
    assert o[2] == 1 and o[3] == part_sum(3) and o[4] == 1 and o[5] == 1, "move assignment: the held block is freed there and then"
    assert counts(lib)[0][DEVICE] == 4 and settled(lib)


@pytest.mark.parametrize("size", [1, 4000])
def test_adopt_takes_a_block_made_elsewhere_and_raises_the_sum_by_its_size(lib, size):
    lib.owned_reset()
    o = (C.c_uint64 * 5)()
    lib.owned_part_adopt(size, o)
    assert o[1] - o[0] == size and o[0] == part_block(0)
    assert o[2] == 1 and o[3] == 1 and o[4] == size, "the block is the part's last one; its maker's owner is empty"
    assert counts(lib)[0][DEVICE] == 2 and settled(lib)


@pytest.mark.parametrize("fail_at", [0, 1, 2, 3])
def test_scene_hand_over_install_drop_and_a_refused_build_beside(lib, fail_at):
    """a scene of two parts (48 + 48 bytes); a part of 240 bytes is built beside part 0 and installed, or its fail_at-th add fails"""
    lib.owned_reset()
    o = (C.c_uint64 * 8)()
    lib.owned_scene_handover(fail_at, o)
    assert o[0] == 96
    if fail_at == 0:
        assert o[7] == 1 and o[1] == 96 + (240 - 48), "install moves the total by new - old"
        assert o[2] == 2, "the old part's blocks are freed before install returns"
        assert o[3] == 0 and o[4] == 4
    else:
        assert o[7] == 0 and o[1] == 96 and o[2] == 0 and o[3] == 1, "the installed part and the total are untouched"
        assert o[4] == 3, "what the refused build had made is gone"
    assert o[5] == o[1] - 48 and o[6] == 1, "drop_part subtracts exactly the part's sum"
    assert counts(lib)[0][DEVICE] == (6 if fail_at == 0 else 3 + fail_at - 1) and settled(lib)


def test_blocks_adopted_into_an_installed_part_are_counted_once_and_freed_once(lib):
    """the lights edit's growth: two blocks made locally join the path-state part"""
    lib.owned_reset()
    o = (C.c_uint64 * 5)()
    lib.owned_scene_grow(4096, 2048, o)
    assert (o[0], o[1], o[2], o[3], o[4]) == (96, 96 + 6144, 48 + 6144, 3, 1)
    assert counts(lib)[0][DEVICE] == 5 and settled(lib)


def test_program_under_address_and_undefined_sanitizers(tmp_path_factory):
    """the stand-ins sit over malloc: a block freed twice, or never, is the sanitizer's to report"""
    out = tmp_path_factory.mktemp("owned_host_san") / "owned_host_san"
    rocm = os.environ.get("ROCM", os.environ.get("ROCM_PATH", "/opt/rocm"))
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-Wall",
                    "-DOWNED_HOST_MAIN", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "opencl_render_amd", "csrc"),
                    "-o", str(out), os.path.join(ROOT, "tests", "owned_host.cpp")], check=True)
    done = subprocess.run([str(out)], capture_output=True, text=True)
    print(done.stdout, done.stderr)
    assert done.returncode == 0 and "all checks passed" in done.stdout, done.stderr or done.stdout
