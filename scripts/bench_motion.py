"""bench_motion.py -- motion vectors (rtHipSceneMotionDevice) on the headline 1M-triangle soup at 1920x1080: mark, then a small pan.

  motion:    the device entry point into device arrays (all four outputs) on a stream of its own: HIP events around each call, the
             median of --reps calls.  One call traces every pixel's centre ray, gathers the reference record and projects it.
  mark:      rtHipSceneMotionMark runs on the scene's own stream, and the next motion call waits for it on the device, so events around
             "mark, then motion" on the idle GPU time both; the mark is that median minus the motion median.  mark_wall_ms is the host's
             clock around mark + rtHipSync, launch and synchronisation included.
  baseline:  the same centre rays, already in device memory, through rtHipSceneIntersectDevice, timed the same way: what a caller
             without the pass pays for the walks alone, before a projection kernel of its own.  Its hits are checked against the pass's
             t and triangle outputs.
Prints one JSON line.  One process; at most 16 CPU threads."""
import argparse
import ctypes as C
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
    ap.add_argument("--pan", type=float, nargs=3, default=(0.02, 0.01, 0.0), help="how far the eye moves after the mark (scene units)")
    args = ap.parse_args()
    import torch
    import motion_oracle as MO
    from opencl_render_amd import raytrace as R, scene as S

    sc = S.make_soup(1920, 1080, args.triangles, 0.004, seed=12345, name="lambert_1m")
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    rs = R.ResidentScene(sc)
    dev = torch.device("cuda", 0)
    L = R.lib()
    run = torch.cuda.Stream(dev)  # a stream of its own: the library takes a NULL stream for the scene's stream
    W, H = sc.width, sc.height

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

    rs.mark_motion()
    eye = np.asarray(sc.eye, np.float32).copy()
    eye[:3] += np.asarray(args.pan, np.float32)
    rs.set_camera(eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)
    out = dict(motion=torch.empty((H, W, 2), dtype=torch.float32, device=dev), t=torch.empty((H, W), dtype=torch.float32, device=dev),
               prev_t=torch.empty((H, W), dtype=torch.float32, device=dev), triangle=torch.empty((H, W), dtype=torch.int32, device=dev))
    ptrs = [C.c_void_p(out[k].data_ptr()) for k in ("motion", "t", "prev_t", "triangle")]

    def motion():
        if L.rtHipSceneMotionDevice(rs.handle, *ptrs, C.c_void_p(run.cuda_stream)):
            raise RuntimeError(R.last_error())

    def mark_then_motion():
        if L.rtHipSceneMotionMark(rs.handle):
            raise RuntimeError(R.last_error())
        motion()

    motion_ms = median_ms(motion)
    both_ms = median_ms(mark_then_motion)
    wall = []
    for _ in range(args.reps):
        rs.sync()
        t0 = time.perf_counter()
        rs.mark_motion()
        rs.sync()
        wall.append(1e3 * (time.perf_counter() - t0))

    # the baseline: the same rays from device memory through the query entry point
    moved = MO.reference((eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom), sc.vertex, sc.tri_index)
    moved.width, moved.height = W, H
    rays = MO.centre_rays(moved)
    n = W * H
    packed = np.empty((n, 8), np.float32)
    packed[:, 0:3], packed[:, 4:7], packed[:, 3], packed[:, 7] = rays["o"], rays["d"], 0.0, np.inf
    rays_dev = torch.from_numpy(packed).to(dev)
    hits = torch.empty((n, 4), dtype=torch.float32, device=dev)

    def query():
        if L.rtHipSceneIntersectDevice(rs.handle, C.c_void_p(rays_dev.data_ptr()), None, n, C.c_void_p(hits.data_ptr()), C.c_void_p(run.cuda_stream)):
            raise RuntimeError(R.last_error())

    query_ms = median_ms(query)
    motion()  # (the marks above made the moved state the reference: t and triangle do not depend on it)
    torch.cuda.synchronize()
    tri = hits[:, 1].view(torch.int32)
    hit = tri != -1
    same = bool(torch.equal(tri, out["triangle"].view(-1)) and torch.equal(hits[:, 0][hit], out["t"].view(-1)[hit]))
    rs.close()
    print(json.dumps(dict(bench="motion_vectors", scene="lambert_1m", triangles=args.triangles, width=W, height=H, reps=args.reps,
                          pan=list(args.pan), hit_share=round(float(hit.float().mean()), 4),
                          motion=dict(ms=round(motion_ms, 4), pixels_per_s=round(n / (motion_ms * 1e-3), 1)),
                          mark=dict(ms=round(both_ms - motion_ms, 4), mark_then_motion_ms=round(both_ms, 4), mark_wall_ms=round(float(np.median(wall)), 4),
                                    reference_bytes=48 * sc.triangle_count),
                          baseline_query=dict(ms=round(query_ms, 4), rays_per_s=round(n / (query_ms * 1e-3), 1)),
                          motion_over_query=round(motion_ms / query_ms, 3), baseline_hits_equal=same,
                          time=time.strftime("%Y-%m-%d %H:%M:%S"))))


if __name__ == "__main__":
    main()
