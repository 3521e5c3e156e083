"""bench_temporal_clamp.py -- the clamped temporal accumulation next to the unclamped one, on the headline 1M-triangle soup at 1920x1080
under a small pan.

Two frames of the resident scene give the inputs: the second frame's colour and flow against the first frame's accumulation and guides,
all left on the device.  On those same arrays, on a stream of its own with HIP events around each call, the median of --reps calls of
  unclamped:  rtHipTemporalDevice (rtt_accumulate_kernel)
  clamped:    rtHipTemporalClampDevice (rtt_clamp_kernel) for modes 1 (min/max), 2 (variance) and 3 (both), gamma 1
  moments:    rtHipTemporalMomentsDevice and rtHipTemporalMomentsClampDevice, mode 3
and the share of the blended pixels in which the mode 3 result differs from the unclamped one.  No threshold: a comparison.
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
    ap.add_argument("--pan", type=float, nargs=3, default=(0.002, 0.001, 0.0), help="how far the eye moves between the two frames (scene units)")
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

    rs.render()
    rs.mark_motion()
    guides = rs.motion()  # frame 0 against itself: its t and triangle maps are the history's guides
    before = rs.temporal()
    eye = np.asarray(sc.eye, np.float32).copy()
    eye[:3] += np.asarray(args.pan, np.float32)
    rs.set_camera(eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)
    rs.render()
    flow = rs.motion()
    frame = np.stack([p.reshape(H, W) for p in rs.readback()], -1).astype(np.float32) / np.float32(65535.0)
    rs.close()

    def gpu(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)

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

    ins = [gpu(frame), gpu(flow["motion"]), gpu(flow["prev_t"]), gpu(flow["triangle"])]
    hist = dict(colour=gpu(before["colour"]), count=gpu(before["count"]), t=gpu(guides["t"]), triangle=gpu(guides["triangle"]))
    lum = (0.2126 * before["colour"][..., 0] + 0.7152 * before["colour"][..., 1] + 0.0722 * before["colour"][..., 2]).astype(np.float32)
    hist_m = dict(hist, moments=gpu(np.stack([lum, lum * lum], -1)))
    res = dict(colour=torch.empty((H, W, 3), device=dev), count=torch.empty((H, W), device=dev))
    plain_ms = median_ms(lambda: R.temporal(*ins, hist, out=res, stream=run.cuda_stream))
    torch.cuda.synchronize()
    plain = {k: v.cpu().numpy() for k, v in res.items()}
    clamped_ms = {}
    for name, mode in R.TEMPORAL_CLAMP_MODES.items():
        clamped_ms[name] = median_ms(lambda: R.temporal(*ins, hist, out=res, stream=run.cuda_stream, clamp=dict(mode=mode, gamma=1.0)))
    torch.cuda.synchronize()
    both = res["colour"].cpu().numpy()
    blended = plain["count"] > 1.0
    differs = (both.view(np.uint32) != plain["colour"].view(np.uint32)).any(-1) & blended
    moments_ms = median_ms(lambda: R.temporal_moments(*ins, hist_m, stream=run.cuda_stream))
    moments_clamped_ms = median_ms(lambda: R.temporal_moments(*ins, hist_m, stream=run.cuda_stream, clamp={}))
    print(json.dumps(dict(bench="temporal_clamp", scene="lambert_1m", triangles=args.triangles, width=W, height=H, reps=args.reps,
                          pan=list(args.pan), blended_share=round(float(blended.mean()), 4),
                          clamp_changed_share_of_blended=round(float(differs.sum() / max(int(blended.sum()), 1)), 4),
                          unclamped_ms=plain_ms, clamped_ms=clamped_ms,
                          clamped_over_unclamped={k: round(v / plain_ms, 3) for k, v in clamped_ms.items()},
                          moments=dict(unclamped_ms=moments_ms, clamped_both_ms=moments_clamped_ms,
                                       clamped_over_unclamped=round(moments_clamped_ms / moments_ms, 3)),
                          pixels_per_s_clamped_both=round(n / (clamped_ms["both"] * 1e-3), 1), time=time.strftime("%Y-%m-%d %H:%M:%S"))))


if __name__ == "__main__":
    main()
