"""What the render passes cost: primary stage time (rtHipStageTimes[0], which also holds the surface pass kernel) and whole-frame time
with the passes off ("off"), with alpha, depth and triangle on ("on") and with all five on ("all": normal and albedo too), interleaved
on one resident scene per workload and sample count (bench.py's lambert_1m and primary_100k, 1920x1080, S = 1 and 16).  Also checks
that the beauty planes are the same every way.  One JSON line per workload and sample count.

    python scripts/passes_cost.py [--workloads lambert_1m primary_100k] [--samples 1 16] [--frames 30] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the workload table)
from opencl_render_amd import raytrace as R, scene as S  # noqa: E402


MODES = {"off": {}, "on": dict(alpha=True, depth=True, triangle=True), "all": dict(alpha=True, depth=True, triangle=True, normal=True, albedo=True)}


def make(name, samples):
    w = bench.WORKLOADS[name]
    kw = dict(materials=[S.primary_only_material(256)], lights=[], random_uv=True) if w["kind"] == "primary" else {}
    sc = S.make_soup(w["width"], w["height"], w["triangles"], w["edge"], seed=12345, samples=samples, name=name, **kw)
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    return sc


def frame_ms(rs, frames):
    rs.sync()
    t0 = time.perf_counter()
    for _ in range(frames):
        rs.render()
    rs.sync()
    return 1e3 * (time.perf_counter() - t0) / frames


def primary_ms(rs, frames):
    rs.stage_timing(True)
    for _ in range(frames):
        rs.render()
    rs.sync()
    ms, _ = rs.stage_times_ms()
    rs.stage_timing(False)
    return ms["primary"] / frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["lambert_1m", "primary_100k"])
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    for name in args.workloads:
        for samples in args.samples:
            sc = make(name, samples)
            rs = R.ResidentScene(sc, 0)
            try:
                planes = {}
                for mode, passes in MODES.items():
                    rs.set_passes(**passes)
                    rs.render()
                    planes[mode] = [p.copy() for p in rs.readback()]
                same = all(np.array_equal(a, b) for mode in ("on", "all") for a, b in zip(planes["off"], planes[mode]))
                coverage = float((rs.readback_passes()["alpha"] > 0).mean())
                res = {mode: {"frame": [], "primary": []} for mode in MODES}
                for _ in range(args.rounds):  # interleaved: off, on, all, off, on, all, ...
                    for mode, passes in MODES.items():
                        rs.set_passes(**passes)
                        frame_ms(rs, 3)  # (warm-up after the switch)
                        res[mode]["frame"].append(frame_ms(rs, args.frames))
                        res[mode]["primary"].append(primary_ms(rs, args.frames))
            finally:
                rs.close()
            out = {"workload": name, "samples": samples, "frames": args.frames, "rounds": args.rounds, "planes_identical": same,
                   "coverage": round(coverage, 4)}
            for mode in MODES:
                for k in ("frame", "primary"):
                    v = res[mode][k]
                    out[f"{k}_ms_{mode}"] = round(statistics.median(v), 4)
                    out[f"{k}_ms_{mode}_spread"] = [round(min(v), 4), round(max(v), 4)]
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
