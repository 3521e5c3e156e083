"""bench_temporal.py -- temporal accumulation on the headline 1M-triangle soup at 1920x1080 under a small pan.

  scene:    --reps times "pan, render, rtHipSceneTemporal"; the medians of rtHipSceneTemporalTimes (motion pass, colour gather, accumulate,
            output) and of the host's clock around the call.
  kernel:   rtHipTemporalDevice alone on device arrays -- the last frame's colour and flow against the history of the frame before -- on a
            stream of its own: HIP events around each call, the median of --reps calls.
  copy:     one device-to-device copy of as many bytes as the kernel must move at least, timed the same way: 48 B read (colour 12, motion
            8, prevT 4, triangle 4 and, taps counted once, history 20) plus 16 B written per pixel; the copy reads and writes each of
            them.  A yardstick, not a threshold.
Prints one JSON line.  One process; at most 16 CPU threads."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--triangles", type=int, default=1_000_000)
    ap.add_argument("--pan", type=float, nargs=3, default=(0.002, 0.001, 0.0), help="how far the eye moves between two frames (scene units)")
    args = ap.parse_args()
    import torch
    from opencl_render_amd import raytrace as R, scene as S

    sc = S.make_soup(1920, 1080, args.triangles, 0.004, seed=12345, name="lambert_1m")
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    rs = R.ResidentScene(sc)
    dev = torch.device("cuda", 0)
    run = torch.cuda.Stream(dev)
    W, H = sc.width, sc.height
    n = W * H
    eye = np.asarray(sc.eye, np.float32).copy()

    def pan():
        eye[:3] += np.asarray(args.pan, np.float32)
        rs.set_camera(eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)

    rs.render()
    rs.mark_motion()
    flow = rs.motion()  # (frame 0 against itself; the call below marks again)
    out = rs.temporal()
    stages, wall = [], []
    for _ in range(args.reps):
        pan()
        rs.render()
        guides, before = flow, out  # the frame before: its t and triangle maps and its accumulation are this frame's history
        flow = rs.motion()  # against the frame before, which the last temporal() marked; the pass itself does not mark
        t0 = time.perf_counter()
        out = rs.temporal()
        wall.append(1e3 * (time.perf_counter() - t0))
        stages.append(rs.temporal_times_ms())
    frame = np.stack([p.reshape(H, W) for p in rs.readback()], -1).astype(np.float32) / np.float32(65535.0)  # the last frame's colour
    accepted = float((out["count"] > 1.0).mean())

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
        return float(np.median(times))

    def gpu(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)

    ins = [gpu(frame), gpu(flow["motion"]), gpu(flow["prev_t"]), gpu(flow["triangle"])]
    hist = dict(colour=gpu(before["colour"]), count=gpu(before["count"]), t=gpu(guides["t"]), triangle=gpu(guides["triangle"]))
    res = dict(colour=torch.empty((H, W, 3), device=dev), count=torch.empty((H, W), device=dev))
    kernel_ms = median_ms(lambda: R.temporal(*ins, hist, out=res, stream=run.cuda_stream))
    torch.cuda.synchronize()
    same = bool(np.array_equal(res["colour"].cpu().numpy().view(np.uint32), out["colour"].view(np.uint32)))
    moved = 64 * n
    src, dst = torch.empty(moved, dtype=torch.uint8, device=dev), torch.empty(moved, dtype=torch.uint8, device=dev)
    copy_ms = median_ms(lambda: dst.copy_(src, non_blocking=True))
    rs.close()
    med = {k: round(float(np.median([s[k] for s in stages])), 4) for k in stages[0]}
    print(json.dumps(dict(bench="temporal_accumulation", scene="lambert_1m", triangles=args.triangles, width=W, height=H, reps=args.reps,
                          pan=list(args.pan), accepted_share=round(accepted, 4), scene_call=dict(stages_ms=med, wall_ms=round(float(np.median(wall)), 3)),
                          kernel=dict(ms=round(kernel_ms, 4), pixels_per_s=round(n / (kernel_ms * 1e-3), 1),
                                      min_bytes_per_s=round(moved / (kernel_ms * 1e-3), 1), equals_scene_call=same),
                          copy=dict(bytes=moved, ms=round(copy_ms, 4), bytes_per_s=round(2 * moved / (copy_ms * 1e-3), 1)),
                          kernel_over_copy=round(kernel_ms / copy_ms, 3), time=time.strftime("%Y-%m-%d %H:%M:%S"))))


if __name__ == "__main__":
    main()
