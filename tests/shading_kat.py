"""Shared by tests/test_shading_kat.py (CPU) and tests/test_shading_kat_gpu.py: the fixture tests/golden/kat_shading.npz, how its
queries are classified, and the comparison.  The queries come from tests/golden/make_golden.py (shading_queries)."""
import importlib.util
import os

import numpy as np

from conftest import GOLDEN

# the least number of vectors of each kind the fixture must hold (so that an edit of the generators cannot drift off the edges)
MIN_TEXEL_ONE = 100        # per axis: queries whose positive_modf is 1.0f (the last column / row)
MIN_TEXEL_PER_TABLE = 300
MIN_PROBE_MISS = 300       # per camera and probe
MIN_VERTEX = 300           # per camera
MIN_EDGE = 300
MIN_DEGENERATE = 20
MIN_PER_MATERIAL = 100     # per camera, material -1 included
ZOOMS = (1, 50)


def fixture():
    return np.load(os.path.join(GOLDEN, "kat_shading.npz"))


def make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def same(got, want):
    """Bit for bit, except that a NaN matches any NaN: x86 and the GPU make NaNs with different sign bits (degenerate triangles
    give 0/0 normals on both), and which NaN comes out is not part of the reference's result.  Returns the rows that differ."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    eq = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return np.flatnonzero(~eq.reshape(len(eq), -1).all(1))

