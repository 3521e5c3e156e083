"""Seeded fuzz of the hot path against the multi-threaded CPU oracle (scenarios.fuzz_scene): even seeds draw opaque-diffuse class
scenes (the class logic kernel), odd seeds general ones (textures, bump maps, mirrors, transparency, several lights).  Longer runs:
python tests/fuzz_parity.py [first seed] [count]."""
import os

import numpy as np
import pytest

import oracle_lib as O
import scenarios as SC
from opencl_render_amd import raytrace as R

pytestmark = pytest.mark.gpu

SEEDS = list(range(16))


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    if hip_lib.rtHipDeviceCount() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (and the product has no CPU fallback)")


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_scene_matches_oracle(seed):
    sc = SC.fuzz_scene(seed)
    R.build_lists(sc)
    if seed % 2 == 0:
        assert R.path_class(sc) == R.PATH_CLASS_OPAQUE_DIFFUSE, SC.fuzz_summary(sc)
    want = O.oracle_render(sc, threads=os.cpu_count() or 1)
    got = R.render_resident(sc, 0)
    for ch, g, w in zip("RGB", got, want):
        bad = int((np.asarray(g) != w).sum())
        assert bad == 0, f"{SC.fuzz_summary(sc)}: plane {ch} differs from the oracle in {bad}/{w.size} pixels"
