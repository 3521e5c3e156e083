"""The tile orders (csrc/rt_tile_order.h) without a GPU: tests/tile_order_host.cpp, a program of its own, checks the two host walkers the
read-backs use -- rows of a tile slot, and pixels in the 8x8-block order of the ambient occlusion and motion planes -- against a
restatement by division that does not use the header, over images with partial tiles (1x1, 128x128, 127x129, 129x127, 257x1, 300x200)
and tile lists in order, reversed, every other tile, the last tile alone and none: every in-image pixel of a listed tile exactly once,
from the right index, nothing outside the image; and that the block order is a bijection.  It runs once as built and once under the
address and undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT

# (the header stands alone: no HIP, no other header of the library)
FLAGS = ["-std=c++17", "-Wall", "-I", os.path.join(ROOT, "opencl_render_amd", "csrc")]


def _build(tmp_path_factory, name, extra):
    out = tmp_path_factory.mktemp(name) / name
    subprocess.run([os.environ.get("CXX", "g++")] + extra + FLAGS + ["-o", str(out), os.path.join(ROOT, "tests", "tile_order_host.cpp")], check=True)
    return str(out)


def _run(program):
    done = subprocess.run([program], capture_output=True, text=True)
    print(done.stdout, done.stderr)
    assert done.returncode == 0, done.stderr or done.stdout
    return done.stdout


def test_walkers_against_division(tmp_path_factory):
    out = _run(_build(tmp_path_factory, "tile_order_host", ["-O2"]))
    assert "cases 30, failures 0" in out


def test_under_address_and_undefined_sanitizers(tmp_path_factory):
    out = _run(_build(tmp_path_factory, "tile_order_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]))
    assert "cases 30, failures 0" in out
