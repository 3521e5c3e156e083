"""tune_variance.py -- how rtHipVarianceDefaults' luminanceSigma2 was chosen: demo.room_scene at 320x240 with S = 2 under a
short orbit, the accumulated and filtered last frame against a converged render (S = 256) at the last pose, over a small grid of values.
Beside it the unfiltered accumulation and rtHipSceneTemporal with the default fixed-sigma denoiser.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--step", type=float, default=2.0, help="degrees of orbit per frame")
    ap.add_argument("--grid", type=float, nargs="+", default=[0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0])
    ap.add_argument("--spatial-below", type=float, nargs="+", default=[4.0])
    args = ap.parse_args()
    from opencl_render_amd import demo, raytrace as R

    W, H = 320, 240
    eye, centre, fov = np.float64([0.1, 1.3, -2.2]), np.float64([0.0, 0.9, 2.5]), np.radians(60.0)

    def pose(i):
        a, d = np.radians(args.step * i), eye - centre
        return np.float32([centre[0] + d[0] * np.cos(a) + d[2] * np.sin(a), eye[1], centre[2] - d[0] * np.sin(a) + d[2] * np.cos(a)])

    def scene(samples):
        sc = demo.room_scene(W, H, samples=samples)
        R.build_camera_list_device(sc, 0)
        R.build_scene_grid_device(sc, 0)
        return sc

    def last_frame(sc, frames, call, first=0):
        rs = R.ResidentScene(sc, 0)
        try:
            rs.set_passes(normal=True, albedo=True)
            for i in range(first, first + frames):
                rs.look_at(pose(i), np.float32(centre), (0, 1, 0), fov)
                rs.render()
                out = call(rs)
            return out["colour"].astype(np.float64)
        finally:
            rs.close()

    noisy, converged, result = scene(2), scene(256), {}
    for frames in args.frames:
        truth = last_frame(converged, 1, lambda rs: rs.temporal(), first=frames - 1)  # (a first call returns the frame itself)
        mse = lambda c: float(np.mean((c - truth) ** 2))  # noqa: E731
        row = dict(accumulated=mse(last_frame(noisy, frames, lambda rs: rs.temporal())),
                   fixed_sigma=mse(last_frame(noisy, frames, lambda rs: rs.temporal(denoise={}))))
        for sb in args.spatial_below:
            for ls in args.grid:
                row[f"ls={ls:g},below={sb:g}"] = mse(last_frame(noisy, frames, lambda rs: rs.temporal_variance(
                    filter=dict(luminance_sigma2=ls, spatial_below=sb))))
        result[f"frames={frames}"] = {k: float(f"{v:.4g}") for k, v in row.items()}
    print(json.dumps(dict(tune="variance_guided_filter", scene="room", width=W, height=H, samples=2, step_degrees=args.step, mse=result)))


if __name__ == "__main__":
    main()
