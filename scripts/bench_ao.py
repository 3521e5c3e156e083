"""bench_ao.py -- ambient occlusion (rtHipSceneAmbientOcclusionDevice) on the headline 1M-triangle soup at 1920x1080, R = 16, Sp = 1.

Two radii: +inf and a short one (0.05 scene units; the soup lies 2 to 4 units deep).  Per radius:
  ao:        the device entry point into a device W x H f32 on a stream of its own: HIP events around each call, the median of --reps
             calls.  One call traces every primary ray, every AO ray and counts them on the device.
  baseline:  the same AO rays (generated on the host by tests/ao_oracle.py from the primary hits ResidentScene.intersect returns, rays
             already on the device) through rtHipSceneIntersectDevice, timed the same way; the image they give, counted with torch on
             the device, is checked against the ao call's.
rays_per_s counts the AO rays that are traced (R per primary hit); the ao figure also pays for the primary rays.
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
    ap.add_argument("--rays", type=int, default=16)
    ap.add_argument("--short", type=float, default=0.05)
    args = ap.parse_args()
    import torch
    import ao_oracle as A
    from opencl_render_amd import raytrace as R, scene as S

    sc = S.make_soup(1920, 1080, args.triangles, 0.004, seed=12345, name="lambert_1m")
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    rs = R.ResidentScene(sc)
    dev = torch.device("cuda", 0)
    L = R.lib()
    run = torch.cuda.Stream(dev)  # a stream of its own: the library takes a NULL stream for the scene's stream
    W, H, Rr = sc.width, sc.height, args.rays

    def median_ms(fn):
        times = []
        with torch.cuda.stream(run):
            fn()  # warm-up
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b))
        return float(np.median(times))

    # the AO rays of every primary hit, generated once (the walk below answers the AO rays with misses: only their directions are wanted)
    answered = []

    def walk(rays):
        if not answered:
            answered.append(True)
            return rs.intersect(rays["o"], rays["d"], rays["tmin"], rays["tmax"], rays["excluded"])
        return dict(triangle=np.full(len(rays["o"]), 0xFFFFFFFF, np.uint32))

    t0 = time.perf_counter()
    _, gen = A.ambient_occlusion(sc, rays=Rr, walk=walk, with_rays=True)
    gen_s = time.perf_counter() - t0
    ao_rays = gen["ao"]
    n = len(ao_rays["o"])
    packed = np.empty((n, 8), np.float32)
    packed[:, 0:3], packed[:, 4:7], packed[:, 3] = ao_rays["o"], ao_rays["d"], 0.0
    rays_dev = torch.from_numpy(packed).to(dev)
    excl_dev = torch.from_numpy(ao_rays["excluded"].view(np.int32).copy()).to(dev)
    pixel_dev = torch.from_numpy(gen["sample"].astype(np.int64)).to(dev)  # Sp = 1: the sample is the pixel
    hits = torch.empty((n, 4), dtype=torch.float32, device=dev)
    del packed, gen, ao_rays

    res = {}
    for name, radius in (("inf", float("inf")), ("short", args.short)):
        p = R.ao_params(rays=Rr, radius=radius)
        out = torch.empty((H, W), dtype=torch.float32, device=dev)

        def ao():
            if L.rtHipSceneAmbientOcclusionDevice(rs.handle, C.byref(p), C.c_void_p(out.data_ptr()), C.c_void_p(run.cuda_stream)):
                raise RuntimeError(R.last_error())

        rays_dev[:, 7] = radius
        torch.cuda.synchronize()

        def query():
            if L.rtHipSceneIntersectDevice(rs.handle, C.c_void_p(rays_dev.data_ptr()), C.c_void_p(excl_dev.data_ptr()), n,
                                           C.c_void_p(hits.data_ptr()), C.c_void_p(run.cuda_stream)):
                raise RuntimeError(R.last_error())

        ao_ms, q_ms = median_ms(ao), median_ms(query)
        torch.cuda.synchronize()
        occluded = (hits[:, 1].view(torch.int32) != -1).to(torch.int64)
        closed = torch.zeros(W * H, dtype=torch.int64, device=dev).index_add_(0, pixel_dev, occluded)
        same = bool(torch.equal((Rr - closed).to(torch.float32) / float(Rr), out.view(-1)))
        res[name] = dict(radius=radius, mean_ao=round(float(out.mean()), 4),
                         ao=dict(ms=round(ao_ms, 4), rays_per_s=round(n / (ao_ms * 1e-3), 1)),
                         baseline_query=dict(ms=round(q_ms, 4), rays_per_s=round(n / (q_ms * 1e-3), 1)),
                         speedup=round(q_ms / ao_ms, 3), baseline_image_equal=same)
    rs.close()
    print(json.dumps(dict(bench="ambient_occlusion", scene="lambert_1m", triangles=args.triangles, width=W, height=H, rays_per_hit=Rr,
                          pixel_samples=1, traced_ao_rays=n, primary_rays=W * H, reps=args.reps, ray_generation_s=round(gen_s, 1),
                          time=time.strftime("%Y-%m-%d %H:%M:%S"), **res)))


if __name__ == "__main__":
    main()
