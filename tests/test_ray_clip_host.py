"""The ray clip's arithmetic (csrc/rt_ray_clip.h) without a GPU: tests/ray_clip_host.cpp, a program of its own, derives the bound of random
small grids (16^3 to 32^3 cells, non-uniform planes, boxes near and far from the origin) the way the scene build does, walks random rays
with the walk's quotients and tie rule, and fails if an occupied cell is visited after a clipped ray's end cell, if a corner of an occupied
cell lies beyond a kept plane, if a ray the predicate excludes (a zero component, a start outside the box, heads that are no ordinary
numbers) is clipped, or if a grid whose occupied cells hold all eight corners keeps a plane.  Its rays include directions nearly parallel
to an axis or to a family of planes, denormal components, exact diagonals, origins on cell faces and box walls and origins beyond the
bound.  It runs once as built and once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from conftest import ROOT

FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", os.path.join(ROOT, "opencl_render_amd", "csrc")]


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run([os.environ.get("CXX", "g++")] + extra + FLAGS + ["-o", str(out), os.path.join(ROOT, "tests", "ray_clip_host.cpp")], check=True)
    return str(out)


def _run(program, *args):
    done = subprocess.run([program] + [str(a) for a in args], capture_output=True, text=True)
    print(done.stdout, done.stderr)
    assert done.returncode == 0, done.stderr or done.stdout
    return done.stdout


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _build(tmp_path_factory, "ray_clip_host", ["-O2"])


@pytest.mark.parametrize("seed", [1, 2])
def test_no_occupied_cell_behind_the_end_cell(program, seed):
    out = _run(program, seed, 48, 4000)
    assert "failures 0" in out


def test_under_address_and_undefined_sanitizers(tmp_path_factory):
    program = _build(tmp_path_factory, "ray_clip_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    out = _run(program, 3, 16, 2000)
    assert "failures 0" in out
