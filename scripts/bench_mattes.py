"""bench_mattes.py -- the matte pass (rtHipSceneMattesDevice) on the headline 1M-triangle soup at 1920x1080: kind TRIANGLE, K = 4 ranked
layers, no selected id, C = 1 and C = 16 samples per pixel (of a sequence of 16).

Per C: the medians over --reps calls of rtHipSceneMatteTimes' two device times (the count launches, the finish kernel), each call into
device arrays on a stream of its own.  The yardstick from the same run and the same resident scene: the device time of one frame (S = 1,
HIP events around rtHipRenderTiles, the median of --reps planned frames), without and with the NORMAL and ALBEDO passes on -- their
difference is what the surface-passes kernel, which makes the same camera scans and shades on top, adds for one sample per pixel.
Prints one JSON line.  One process; at most 16 CPU threads."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--triangles", type=int, default=1_000_000)
    ap.add_argument("--layers", type=int, default=4)
    args = ap.parse_args()
    import torch
    from opencl_render_amd import raytrace as R, scene as S

    sc = S.make_soup(1920, 1080, args.triangles, 0.004, seed=12345, name="lambert_1m")
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    rs = R.ResidentScene(sc)
    dev = torch.device("cuda", 0)
    run = torch.cuda.Stream(dev)  # a stream of its own: the library takes a NULL stream for the scene's stream
    W, H, K = sc.width, sc.height, args.layers

    def frame_ms():
        times = []
        with torch.cuda.stream(run):
            for i in range(args.reps + 2):  # the first frame discovers the launch plan, the second is the first planned one
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rs.render(run.cuda_stream)
                b.record()
                b.synchronize()
                rs.finish()
                if i >= 2:
                    times.append(a.elapsed_time(b))
        return float(np.median(times))

    plain = frame_ms()
    rs.set_passes(normal=True, albedo=True)
    surface = frame_ms()
    rs.set_passes()

    out = dict(layer_id=torch.empty((K, H, W), dtype=torch.int32, device=dev), layer_coverage=torch.empty((K, H, W), device=dev),
               rest=torch.empty((H, W), device=dev))
    res = {}
    for C_ in (1, 16):
        count, finish = [], []
        for i in range(args.reps + 1):  # (the first call makes the scratch)
            rs.mattes(kind="triangle", layers=K, total=16, first=0, samples=C_, out=out, stream=run.cuda_stream)
            ms = rs.matte_times_ms()
            if i:
                count.append(ms["count"])
                finish.append(ms["finish"])
        torch.cuda.synchronize()
        cov = out["layer_coverage"]
        res[f"samples_{C_}"] = dict(count_ms=round(float(np.median(count)), 4), finish_ms=round(float(np.median(finish)), 4),
                                    count_ms_per_sample=round(float(np.median(count)) / C_, 4),
                                    covered_pixels=round(float((cov[0] > 0).float().mean()), 4),
                                    edge_pixels=round(float(((cov[0] > 0) & (cov[0] < 1)).float().mean()), 4),
                                    overflowing_pixels=round(float((out["rest"] > 0).float().mean()), 6))
    rs.close()
    print(json.dumps(dict(bench="mattes", scene="lambert_1m", triangles=args.triangles, width=W, height=H, kind="triangle", layers=K,
                          selected=0, reps=args.reps, frame_ms=round(plain, 4), frame_with_surface_passes_ms=round(surface, 4),
                          surface_passes_kernel_ms=round(surface - plain, 4), time=time.strftime("%Y-%m-%d %H:%M:%S"), **res)))


if __name__ == "__main__":
    main()
