"""bench_variance.py -- the variance-guided filter on the headline 1M-triangle soup at 1920x1080 under a small pan.

  scene:    --reps times "pan, render, rtHipSceneTemporalVariance" with the filter at its defaults; the medians of rtHipSceneTemporalTimes
            (motion pass, gather, moments accumulation, estimate + filter + output) and of the host's clock around the call.  The same loop
            with rtHipSceneTemporal and the fixed-sigma denoiser beside it.
  kernels:  on device arrays, on a stream of its own, HIP events around each call, the median of --reps calls: rtHipTemporalMomentsDevice
            beside rtHipTemporalDevice (the last frame against the history of the frame before), and rtHipDenoiseVarianceDevice beside
            rtHipDenoiseDevice (the last accumulation, both at K = 4).
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
    dev = torch.device("cuda", 0)
    run = torch.cuda.Stream(dev)
    W, H = sc.width, sc.height
    n = W * H

    def loop(call):
        """(medians of the stage times, median wall ms, last flow, flow before, last output, output before, last frame, surfaces)."""
        rs = R.ResidentScene(sc)
        try:
            rs.set_passes(normal=True, albedo=True)
            eye = np.asarray(sc.eye, np.float32).copy()
            rs.render()
            rs.mark_motion()
            flow = rs.motion()
            out = call(rs)
            stages, wall = [], []
            for _ in range(args.reps):
                eye[:3] += np.asarray(args.pan, np.float32)
                rs.set_camera(eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)
                rs.render()
                guides, before = flow, out
                flow = rs.motion()
                t0 = time.perf_counter()
                out = call(rs)
                wall.append(1e3 * (time.perf_counter() - t0))
                stages.append(rs.temporal_times_ms())
            frame = np.stack([p.reshape(H, W) for p in rs.readback()], -1).astype(np.float32) / np.float32(65535.0)
            med = {k: round(float(np.median([s[k] for s in stages])), 4) for k in stages[0]}
            return med, round(float(np.median(wall)), 3), flow, guides, out, before, frame, rs.readback_passes()
        finally:
            rs.close()

    fixed = loop(lambda rs: rs.temporal(denoise={}))
    plain = loop(lambda rs: rs.temporal_variance())  # no filter: the accumulation, its moments and variance
    med, wall, flow, guides, out, before, frame, surf = loop(lambda rs: rs.temporal_variance(filter={}))

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

    # the unfiltered accumulation of the last two frames comes from the loop without a filter (the same frames: the renderer seeds alike)
    acc, acc_before = plain[4], plain[5]
    lum = lambda c: (np.float32(0.2126) * c[..., 0] + np.float32(0.7152) * c[..., 1]) + np.float32(0.0722) * c[..., 2]  # noqa: E731
    l = lum(acc_before["colour"])
    ins = [gpu(frame), gpu(flow["motion"]), gpu(flow["prev_t"]), gpu(flow["triangle"])]
    hist = dict(colour=gpu(acc_before["colour"]), count=gpu(acc_before["count"]), t=gpu(guides["t"]), triangle=gpu(guides["triangle"]))
    # (the scene keeps its moments to itself; for the kernel's timing the history's are rebuilt from its colour and variance)
    hist_m = dict(hist, moments=gpu(np.stack([l, l * l + acc_before["variance"]], -1)))
    res = dict(colour=torch.empty((H, W, 3), device=dev), count=torch.empty((H, W), device=dev))
    temporal_ms = median_ms(lambda: R.temporal(*ins, hist, out=res, stream=run.cuda_stream))
    moments_ms = median_ms(lambda: R.temporal_moments(*ins, hist_m, stream=run.cuda_stream))
    got = R.temporal_moments(*ins, hist_m)
    torch.cuda.synchronize()
    same = bool(np.array_equal(got["colour"].cpu().numpy().view(np.uint32), acc["colour"].view(np.uint32)))
    c, nrm, alb = gpu(acc["colour"]), gpu(surf["normal"]), gpu(surf["albedo"])
    mom, cnt = got["moments"], gpu(acc["count"])
    denoise_ms = median_ms(lambda: R.denoise(c, nrm, alb, stream=run.cuda_stream))
    variance_ms = median_ms(lambda: R.denoise_variance(c, nrm, alb, mom, cnt, stream=run.cuda_stream))
    single_ms = median_ms(lambda: R.denoise_variance(c, nrm, alb, stream=run.cuda_stream))
    spatial_ms = median_ms(lambda: R.denoise_variance(c, nrm, alb, mom, cnt, stream=run.cuda_stream, spatial_below=65537.0))
    print(json.dumps(dict(bench="variance_guided_filter", scene="lambert_1m", triangles=args.triangles, width=W, height=H, reps=args.reps,
                          pan=list(args.pan), accepted_share=round(float((out["count"] > 1.0).mean()), 4),
                          spatial_arm_share=round(float((out["count"] < 4.0).mean()), 4),
                          scene_call=dict(stages_ms=med, wall_ms=wall),
                          scene_call_no_filter=dict(stages_ms=plain[0], wall_ms=plain[1]),
                          scene_temporal_fixed_sigma=dict(stages_ms=fixed[0], wall_ms=fixed[1]),
                          kernels_ms=dict(temporal=round(temporal_ms, 4), temporal_moments=round(moments_ms, 4), denoise_k4=round(denoise_ms, 4),
                                          denoise_variance_k4=round(variance_ms, 4), denoise_variance_k4_single_frame=round(single_ms, 4),
                                          denoise_variance_k4_all_spatial=round(spatial_ms, 4)),
                          moments_colour_equals_scene_call=same, time=time.strftime("%Y-%m-%d %H:%M:%S"))))


if __name__ == "__main__":
    main()
