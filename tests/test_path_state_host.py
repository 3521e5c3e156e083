"""The ring allocation's index functions (csrc/rt_path_state.h) without a GPU: tests/path_state_host.cpp, a program of its own, walks every
path id of capacities 65 536 and 131 072 and fails if a quad of the class layout -- the camera direction (slot 0, quad 1) or the bounce
record (slot 1, quads 0..2) -- lies outside the 36 * capacity quads of the allocation, if two of them share a quad, if a bounce record
straddles a 128-byte line, or if the general layout is anything but a * 36 + slot * 3 + quad.  It runs once as built and once under the
address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from conftest import ROOT

FLAGS = ["-std=c++17", "-Wall", "-I", os.path.join(ROOT, "opencl_render_amd", "csrc")]


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run([os.environ.get("CXX", "g++")] + extra + FLAGS + ["-o", str(out), os.path.join(ROOT, "tests", "path_state_host.cpp")], check=True)
    return str(out)


def _run(program, *args):
    done = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True)
    print(done.stdout, done.stderr)
    assert done.returncode == 0, done.stderr or done.stdout
    return done.stdout


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory, "path_state_host", ["-O2"])


@pytest.mark.parametrize("capacity", [65536, 131072])
def test_class_quads_inside_distinct_and_line_bound(program, capacity):
    out = _run(program, capacity)
    assert "failures 0" in out


def test_under_address_and_undefined_sanitizers(tmp_path_factory):
    program = _build(tmp_path_factory, "path_state_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    out = _run(program, 65536, 131072)
    assert "failures 0" in out
