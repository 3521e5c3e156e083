"""What the render passes cost: primary stage time (rtHipStageTimes[0]) and whole-frame time with the passes off and with all of them on,
interleaved A/B on one resident scene per workload (bench.py's lambert_1m and primary_100k, 1920x1080, S=1).  Also checks that the
beauty planes are the same either way.  One JSON line per workload.

    python scripts/passes_cost.py [--workloads lambert_1m primary_100k] [--frames 30] [--rounds 5]
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


def make(name):
    w = bench.WORKLOADS[name]
    kw = dict(materials=[S.primary_only_material(256)], lights=[], random_uv=True) if w["kind"] == "primary" else {}
    sc = S.make_soup(w["width"], w["height"], w["triangles"], w["edge"], seed=12345, samples=1, name=name, **kw)
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
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    for name in args.workloads:
        sc = make(name)
        rs = R.ResidentScene(sc, 0)
        try:
            rs.render()
            off_planes = [p.copy() for p in rs.readback()]
            rs.set_passes(alpha=True, depth=True, triangle=True)
            rs.render()
            on_planes = rs.readback()
            same = all(np.array_equal(a, b) for a, b in zip(off_planes, on_planes))
            coverage = float((rs.readback_passes()["alpha"] > 0).mean())
            res = {"off": {"frame": [], "primary": []}, "on": {"frame": [], "primary": []}}
            for _ in range(args.rounds):  # interleaved: off, on, off, on, ...
                for mode in ("off", "on"):
                    if mode == "off":
                        rs.set_passes()
                    else:
                        rs.set_passes(alpha=True, depth=True, triangle=True)
                    frame_ms(rs, 3)  # (warm-up after the switch)
                    res[mode]["frame"].append(frame_ms(rs, args.frames))
                    res[mode]["primary"].append(primary_ms(rs, args.frames))
        finally:
            rs.close()
        out = {"workload": name, "frames": args.frames, "rounds": args.rounds, "planes_identical": same, "coverage": round(coverage, 4)}
        for mode in ("off", "on"):
            for k in ("frame", "primary"):
                v = res[mode][k]
                out[f"{k}_ms_{mode}"] = round(statistics.median(v), 4)
                out[f"{k}_ms_{mode}_spread"] = [round(min(v), 4), round(max(v), 4)]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
