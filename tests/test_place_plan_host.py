"""Direct placement's host arithmetic (csrc/rt_frame_plan.h) without a GPU: tests/place_plan_host.cpp, a program of its own, checks
round_goes_direct over the product of its inputs -- planned or watched, the round, ordered or not, the cut, the slices, the path class, the
tuning key, visit_log, the sample batches, and a stamp that is the round's, invalid, or of another layout or sample window -- and
place_table (bases = the exclusive prefix of the counts, class-major, longest class first, total = their sum) against a plain
re-implementation.  It runs once as built and once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT

ROCM = os.environ.get("ROCM", os.environ.get("ROCM_PATH", "/opt/rocm"))
# (rt_device.h takes float4 / uint4 from the HIP headers; nothing of the runtime is linked)
FLAGS = ["-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", os.path.join(ROOT, "include"),
         "-I", os.path.join(ROOT, "opencl_render_amd", "csrc")]


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run([os.environ.get("CXX", "g++")] + extra + FLAGS + ["-o", str(out), os.path.join(ROOT, "tests", "place_plan_host.cpp")], check=True)
    return str(out)


def _run(program):
    done = subprocess.run([program], capture_output=True, text=True)
    print(done.stdout, done.stderr)
    assert done.returncode == 0, done.stderr or done.stdout
    return done.stdout


def test_decision_and_table(tmp_path_factory):
    assert "failures 0" in _run(_build(tmp_path_factory, "place_plan_host", ["-O2"]))


def test_under_address_and_undefined_sanitizers(tmp_path_factory):
    program = _build(tmp_path_factory, "place_plan_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "failures 0" in _run(program)
