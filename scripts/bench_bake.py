"""bench_bake.py -- the ambient occlusion bake (rtHipSceneBakeAmbientOcclusionDevice) of the headline 1M-triangle soup over a grid atlas
(scene.grid_atlas_uv) at 4096x4096, R = 16, G = 2.

Two radii: +inf and a short one (0.05 scene units; the soup lies 2 to 4 units deep).  Per radius:
  bake:      the device entry point into device W x H maps on a stream of its own: HIP events around each call, the median of --reps
             calls.  One call rasterises the atlas, makes the surface points, traces every AO ray, finishes and dilates.
  setup:     the same call with R = 1 and radius 1e-30 (each AO ray's walk ends at once): an upper bound on the rasterise, points, finish
             and dilation share; ao_phase = bake - setup.
  baseline:  the same AO rays (generated on the host by tests/bake_oracle.py, rays already on the device) through
             rtHipSceneIntersectDevice, timed the same way; the map they give, counted with torch on the device, is checked against
             the bake's values before dilation (a G = 0 call).
rays_per_s counts the AO rays that are traced (R per covered texel with a normal).  Prints one JSON line.  One process; at most 16 CPU
threads."""
import argparse
import ctypes as C
import dataclasses
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
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rays", type=int, default=16)
    ap.add_argument("--short", type=float, default=0.05)
    args = ap.parse_args()
    import torch
    import bake_oracle as B
    from opencl_render_amd import raytrace as R, scene as S

    sc = S.make_soup(1920, 1080, args.triangles, 0.004, seed=12345, name="lambert_1m")
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    N, Rr = args.size, args.rays
    sc = dataclasses.replace(sc, tri_uv=S.grid_atlas_uv(sc.triangle_count, N))
    rs = R.ResidentScene(sc)
    dev = torch.device("cuda", 0)
    L = R.lib()
    run = torch.cuda.Stream(dev)  # a stream of its own: the library takes a NULL stream for the scene's stream
    ao = torch.empty((N, N), dtype=torch.float32, device=dev)
    tri = torch.empty((N, N), dtype=torch.int32, device=dev)

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

    def bake_call(p):
        def fn():
            if L.rtHipSceneBakeAmbientOcclusionDevice(rs.handle, C.byref(p), C.c_void_p(ao.data_ptr()), C.c_void_p(tri.data_ptr()),
                                                      C.c_void_p(run.cuda_stream)):
                raise RuntimeError(R.last_error())
        return fn

    # the AO rays of every covered texel, generated once (the walk answers them with misses: only the rays are wanted)
    t0 = time.perf_counter()
    gen = B.bake(sc, N, N, rays=Rr, dilate_passes=0, rects=True, with_rays=True,
                 walk=lambda r: dict(triangle=np.full(len(r["o"]), B.NONE, np.uint32)))
    gen_s = time.perf_counter() - t0
    covered = int((gen["triangle"] != B.NONE).sum())
    rays = gen["rays"]
    n = len(rays["o"])
    packed = np.empty((n, 8), np.float32)
    packed[:, 0:3], packed[:, 4:7], packed[:, 3] = rays["o"], rays["d"], 0.0
    rays_dev = torch.from_numpy(packed).to(dev)
    excl_dev = torch.from_numpy(rays["excluded"].view(np.int32).copy()).to(dev)
    texel_dev = torch.from_numpy(gen["texel"].astype(np.int64)).to(dev)
    cov_dev = torch.from_numpy((gen["triangle"] != B.NONE).ravel()).to(dev)
    hits = torch.empty((n, 4), dtype=torch.float32, device=dev)
    del packed, gen, rays

    setup_ms = median_ms(bake_call(R.bake_params(N, N, rays=1, radius=1e-30)))
    res = {}
    for name, radius in (("inf", float("inf")), ("short", args.short)):
        bake_ms = median_ms(bake_call(R.bake_params(N, N, rays=Rr, radius=radius)))
        rays_dev[:, 7] = radius
        torch.cuda.synchronize()

        def query():
            if L.rtHipSceneIntersectDevice(rs.handle, C.c_void_p(rays_dev.data_ptr()), C.c_void_p(excl_dev.data_ptr()), n,
                                           C.c_void_p(hits.data_ptr()), C.c_void_p(run.cuda_stream)):
                raise RuntimeError(R.last_error())

        q_ms = median_ms(query)
        with torch.cuda.stream(run):
            bake_call(R.bake_params(N, N, rays=Rr, radius=radius, dilate=0))()
        torch.cuda.synchronize()
        occluded = (hits[:, 1].view(torch.int32) != -1).to(torch.int64)
        closed = torch.zeros(N * N, dtype=torch.int64, device=dev).index_add_(0, texel_dev, occluded)
        want = torch.where(cov_dev, (Rr - closed).to(torch.float32) / float(Rr), torch.zeros((), device=dev))
        same = bool(torch.equal(want, ao.view(-1)))
        ao_phase = max(bake_ms - setup_ms, 1e-9)
        res[name] = dict(radius=radius, mean_ao=round(float(ao.mean()), 4),
                         bake=dict(ms=round(bake_ms, 4), texels_per_s=round(N * N / (bake_ms * 1e-3), 1), rays_per_s=round(n / (bake_ms * 1e-3), 1)),
                         ao_phase=dict(ms=round(ao_phase, 4), rays_per_s=round(n / (ao_phase * 1e-3), 1)),
                         baseline_query=dict(ms=round(q_ms, 4), rays_per_s=round(n / (q_ms * 1e-3), 1)),
                         setup_share=round(setup_ms / bake_ms, 4), speedup=round(q_ms / bake_ms, 3), baseline_map_equal=same)
    rs.close()
    print(json.dumps(dict(bench="ambient_occlusion_bake", scene="lambert_1m", triangles=args.triangles, size=N, rays_per_texel=Rr, dilate=2,
                          covered_texels=covered, traced_ao_rays=n, reps=args.reps, ray_generation_s=round(gen_s, 1),
                          setup=dict(ms=round(setup_ms, 4), note="R = 1, radius 1e-30: rasterise + points + finish + dilate, an upper bound"),
                          time=time.strftime("%Y-%m-%d %H:%M:%S"), **res)))


if __name__ == "__main__":
    main()
