"""The frame scheduler's arithmetic (csrc/rt_frame_plan.h) without a GPU: tests/frame_plan_host.cpp, a program of its own, checks a
round's layout (mode_for), a planned round's trace and shade grids, the split-round predicate, the folding of a watched batch's round log
into the next plan and the plan's adoption against answers worked out by hand from the rules, and then, over random inputs, that a
planned trace grid lies between 1 and the worst case and never shrinks with more rays and that a planned shade grid is 0 or a multiple
of 64.  It runs once as built and once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from conftest import ROOT

ROCM = os.environ.get("ROCM", os.environ.get("ROCM_PATH", "/opt/rocm"))
# (rt_device.h takes float4 / uint4 from the HIP headers; nothing of the runtime is linked)
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"),
         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "opencl_render_amd", "csrc")]


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run([os.environ.get("CXX", "g++")] + extra + FLAGS + ["-o", str(out), os.path.join(ROOT, "tests", "frame_plan_host.cpp")], check=True)
    return str(out)


def _run(program, *args):
    done = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True)
    print(done.stdout, done.stderr)
    assert done.returncode == 0, done.stderr or done.stdout
    return done.stdout


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory, "frame_plan_host", ["-O2"])


@pytest.mark.parametrize("seed", [1, 2])
def test_known_answers_and_invariants(program, seed):
    out = _run(program, seed, 4000)
    assert "failures 0" in out


def test_under_address_and_undefined_sanitizers(tmp_path_factory):
    program = _build(tmp_path_factory, "frame_plan_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    out = _run(program, 3, 2000)
    assert "failures 0" in out
