"""bench_dof.py -- the depth of field (include/raytrace_hip.h, "DEPTH OF FIELD") on the headline 1M-triangle soup at 1920x1080, at the
default parameters (3 rings, 49 taps) and with rings = 6 (169 taps), under two settings:
  sharp:     cocScale 0.45 -- no radius reaches half a pixel, every tile takes the copy arm (in the soup every tile neighbourhood holds a
             miss or a far triangle, so at the default cocScale no focus distance leaves a tile in the copy arm: the copy arm is
             measured with an aperture this small instead)
  defocused: the defaults focused at the median depth of the frame's hits -- every pixel in the gather

Per setting, medians of --reps in one process:
  scene:    the three parts of rtHipSceneDepthOfFieldTimes (gather of colour and depth, blur, output) over --reps ResidentScene.depth_of_field()
  device:   rtHipDepthOfFieldDevice alone on the same frame and depth, left on the device, HIP events around each call on a stream of its own
  floor:    a device-to-device copy of 14 bytes per pixel -- 28 bytes of traffic, what the filter must move at least (it reads colour 12 and
            depth 4 and writes 12)
  denoise:  rtHipDenoiseDevice at its default iterations on the same image, as a familiar yardstick
  motion_blur: rtHipMotionBlurDevice at its defaults on the same image, with the flow of a small pan
and the share of pixels in the gather arm.  Reported, not gated.  Prints one JSON line.  One process; at most 16 CPU threads."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PAN = (0.002, 0.001, 0.0)  # how far the eye moves between the mark and the frame (scene units): the flow the motion blur is timed on


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

    rs = R.ResidentScene(sc)
    result = {}
    try:
        rs.set_passes(depth=True, normal=True, albedo=True)
        rs.render()
        rs.mark_motion()
        eye = np.asarray(sc.eye, np.float32).copy()
        eye[:3] += np.asarray(PAN, np.float32)
        rs.set_camera(eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)
        rs.render()
        surf = rs.readback_passes()
        flow = rs.motion()
        frame = np.stack([p.reshape(H, W) for p in rs.readback()], -1).astype(np.float32) / np.float32(65535.0)
        depth = surf["depth"]
        hits = depth[np.isfinite(depth) & (depth > 0)]
        median = float(np.median(hits)) if hits.size else 1.0
        settings = dict(sharp=dict(focus=median, coc_scale=0.45), defocused=dict(focus=median))
        scene_ms = {}
        for name, base in settings.items():
            for rings in (R.DEPTH_OF_FIELD_DEFAULTS["rings"], 6):
                params = dict(base, rings=rings)
                parts = []
                rs.depth_of_field(**params)  # warm-up: the storage is made here
                for _ in range(args.reps):
                    rs.depth_of_field(**params)
                    parts.append(rs.depth_of_field_times_ms())
                scene_ms[name, rings] = {k: round(float(np.median([p[k] for p in parts])), 4) for k in ("gather", "blur", "output")}
    finally:
        rs.close()
    c, z = gpu(frame), gpu(depth)
    out = torch.empty((H, W, 3), device=dev)
    src, dst = torch.empty(n * 14, dtype=torch.uint8, device=dev), torch.empty(n * 14, dtype=torch.uint8, device=dev)
    floor_ms = median_ms(lambda: dst.copy_(src))
    nrm, alb = gpu(surf["normal"]), gpu(surf["albedo"])
    denoise_ms = median_ms(lambda: R.denoise(c, nrm, alb, stream=run.cuda_stream))
    m, t = gpu(flow["motion"]), gpu(flow["t"])
    motion_blur_ms = median_ms(lambda: R.motion_blur(c, m, t, out=out, stream=run.cuda_stream))
    ty, tx = (H + 31) // 32, (W + 31) // 32
    for name, base in settings.items():
        p = dict(R.DEPTH_OF_FIELD_DEFAULTS, **base)
        with np.errstate(all="ignore"):  # (a) of the definition, for the share of pixels in the gather arm
            a = np.where(depth == np.inf, np.float32(1), np.where(depth > 0, np.abs(depth - np.float32(p["focus"])) / depth, np.float32(0)))
            r = a.astype(np.float32) * np.float32(p["coc_scale"])
            r = np.where(~(r < np.float32(p["max_coc"])), np.float32(p["max_coc"] if p["coc_scale"] > 0 else 0), r)
        tiles = np.zeros((ty * 32, tx * 32), np.float32)
        tiles[:H, :W] = r
        tiles = tiles.reshape(ty, 32, tx, 32).max((1, 3))
        near = np.zeros_like(tiles)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                dst_box = near[max(dy, 0):ty + min(dy, 0), max(dx, 0):tx + min(dx, 0)]
                np.maximum(dst_box, tiles[max(-dy, 0):ty + min(-dy, 0), max(-dx, 0):tx + min(-dx, 0)], out=dst_box)
        gather_share = float((np.repeat(np.repeat(near, 32, 0), 32, 1)[:H, :W] >= 0.5).mean())
        entry = dict(params=base, gather_share=round(gather_share, 4), mean_radius=round(float(r.mean()), 3))
        for rings in (R.DEPTH_OF_FIELD_DEFAULTS["rings"], 6):
            device_ms = median_ms(lambda: R.depth_of_field(c, z, **dict(base, rings=rings), out=out, stream=run.cuda_stream))
            entry[f"rings{rings}"] = dict(taps=1 + 4 * rings * (rings + 1), device_ms=device_ms, scene_ms=scene_ms[name, rings],
                                          device_over_floor=round(device_ms / floor_ms, 2), pixels_per_s=round(n / (device_ms * 1e-3), 1))
        result[name] = entry
    print(json.dumps(dict(bench="dof", scene="lambert_1m", triangles=args.triangles, width=W, height=H, reps=args.reps,
                          defaults=R.DEPTH_OF_FIELD_DEFAULTS, focus=round(median, 4), floor_copy_ms=floor_ms, denoise_ms=denoise_ms,
                          motion_blur_ms=motion_blur_ms, **result, time=time.strftime("%Y-%m-%d %H:%M:%S"))))


if __name__ == "__main__":
    main()
