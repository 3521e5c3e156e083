"""Fuzz of the hot path against the CPU oracle on the GPU box, for long runs (the suite runs a few fixed seeds of the same generator:
tests/test_fuzz_parity_gpu.py).  Scenes come from scenarios.fuzz_scene: even seeds opaque-diffuse class scenes, odd seeds general
ones (textures, bump maps, mirrors, transparency, random lights of every type).
usage: python tests/fuzz_parity.py [first seed] [count]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import oracle_lib as O
import scenarios as SC
from opencl_render_amd import raytrace as R

first = int(sys.argv[1]) if len(sys.argv) > 1 else 100
count = int(sys.argv[2]) if len(sys.argv) > 2 else 20
bad = 0
for seed in range(first, first + count):
    sc = SC.fuzz_scene(seed)
    R.build_lists(sc)
    want = O.oracle_render(sc, threads=os.cpu_count() or 1)
    got = R.render_resident(sc, 0)
    diff = sum(int((np.asarray(g).reshape(-1) != np.asarray(x).reshape(-1)).sum()) for g, x in zip(got, want))
    print(f"{SC.fuzz_summary(sc)}: {'OK' if diff == 0 else f'{diff} VALUES DIFFER'}", flush=True)
    bad += diff != 0
print("fuzz:", "all bit-exact" if bad == 0 else f"{bad} scenes differ")
sys.exit(1 if bad else 0)
