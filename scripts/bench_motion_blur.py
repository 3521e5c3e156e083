"""bench_motion_blur.py -- the vector motion blur (include/raytrace_hip.h, "MOTION BLUR") on the headline 1M-triangle soup at 1920x1080,
under a small pan and under a fast one (most tiles in the gather arm).

Per pan: the scene is marked, the camera moved, a frame rendered.  Then, medians of --reps in one process:
  scene:    the three parts of rtHipSceneMotionBlurTimes (motion pass, colour gather, blur with output) over --reps ResidentScene.motion_blur()
  device:   rtHipMotionBlurDevice alone on the same frame, flow and depth left on the device, HIP events around each call on a stream of its own
  floor:    a device-to-device copy of 18 bytes per pixel -- 36 bytes of traffic, what the filter must move at least (it reads colour 12,
            motion 8 and depth 4 and writes 12)
  denoise:  rtHipDenoiseDevice at its default iterations on the same image, as a familiar yardstick
and the share of pixels in the gather arm.  Reported, not gated.  Prints one JSON line.  One process; at most 16 CPU threads."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PANS = dict(small=(0.002, 0.001, 0.0), fast=(0.06, 0.03, 0.0))  # how far the eye moves between the mark and the frame (scene units)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--triangles", type=int, default=1_000_000)
    args = ap.parse_args()
    import torch
    from opencl_render_amd import raytrace as R, scene as S

    sc = S.make_soup(1920, 1080, args.triangles, 0.004, seed=12345, name="lambert_1m")
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    dev = torch.device("cuda", 0)
    run = torch.cuda.Stream(dev)
    W, H = sc.width, sc.height
    n = W * H

    def gpu(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def median_ms(fn):
        times = []
        with torch.cuda.stream(run):
            fn()  # warm-up
            for _ in range(args.reps):
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b))
        return round(float(np.median(times)), 4)

    result = {}
    for name, pan in PANS.items():
        rs = R.ResidentScene(sc)
        try:
            rs.set_passes(normal=True, albedo=True)
            rs.render()
            rs.mark_motion()
            eye = np.asarray(sc.eye, np.float32).copy()
            eye[:3] += np.asarray(pan, np.float32)
            rs.set_camera(eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)
            rs.render()
            parts = []
            rs.motion_blur()  # warm-up: the storage is made here
            for _ in range(args.reps):
                rs.motion_blur()
                parts.append(rs.motion_blur_times_ms())
            flow = rs.motion()
            surf = rs.readback_passes()
            frame = np.stack([p.reshape(H, W) for p in rs.readback()], -1).astype(np.float32) / np.float32(65535.0)
        finally:
            rs.close()
        c, m, z = gpu(frame), gpu(flow["motion"]), gpu(flow["t"])
        out = torch.empty((H, W, 3), device=dev)
        device_ms = median_ms(lambda: R.motion_blur(c, m, z, out=out, stream=run.cuda_stream))
        src, dst = torch.empty(n * 18, dtype=torch.uint8, device=dev), torch.empty(n * 18, dtype=torch.uint8, device=dev)
        floor_ms = median_ms(lambda: dst.copy_(src))
        nrm, alb = gpu(surf["normal"]), gpu(surf["albedo"])
        denoise_ms = median_ms(lambda: R.denoise(c, nrm, alb, stream=run.cuda_stream))
        with np.errstate(all="ignore"):
            length = np.hypot(flow["motion"][..., 0], flow["motion"][..., 1]) * 0.25  # (the default shutter: half of 0.5)
        moving = np.nan_to_num(length, nan=0.0, posinf=0.0) >= 0.5
        ty, tx = (H + 31) // 32, (W + 31) // 32
        tiles = np.zeros((ty * 32, tx * 32), bool)
        tiles[:H, :W] = moving
        tiles = tiles.reshape(ty, 32, tx, 32).any((1, 3))
        near = np.zeros_like(tiles)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                near[max(dy, 0):ty + min(dy, 0), max(dx, 0):tx + min(dx, 0)] |= tiles[max(-dy, 0):ty + min(-dy, 0), max(-dx, 0):tx + min(-dx, 0)]
        gather_share = float(np.repeat(np.repeat(near, 32, 0), 32, 1)[:H, :W].mean())
        result[name] = dict(pan=list(pan), gather_share=round(gather_share, 4),
                            scene_ms={k: round(float(np.median([p[k] for p in parts])), 4) for k in ("motion", "gather", "blur")},
                            device_ms=device_ms, floor_copy_ms=floor_ms, device_over_floor=round(device_ms / floor_ms, 2),
                            denoise_ms=denoise_ms, pixels_per_s=round(n / (device_ms * 1e-3), 1))
    print(json.dumps(dict(bench="motion_blur", scene="lambert_1m", triangles=args.triangles, width=W, height=H, reps=args.reps,
                          params=R.MOTION_BLUR_DEFAULTS, **result, time=time.strftime("%Y-%m-%d %H:%M:%S"))))


if __name__ == "__main__":
    main()
