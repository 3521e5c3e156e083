"""Device time of the denoiser (include/raytrace_hip.h, "DENOISER") at 1080p and 4K: prints one JSON line.

Per size, with HIP events on torch's stream around rtHipDenoiseDevice (seeded random inputs, median of --reps calls after --warmup):
  call_ms       the whole K-iteration call (guides, K iterations, output)
  k0_ms         a K = 0 call: the guide prologue and the output kernel alone
  iter_us       (call_ms - k0_ms) / K
  iter_us_by_h  (1080p) what the iteration of dilation h adds: the difference of the medians of the K = i + 1 and K = i calls
                (medians of separate runs, so these do not add up exactly to call_ms - k0_ms)
and per size from rtHipSceneDenoise on a rendered demo room, medians of the events the library records around its stages
(rtHipSceneDenoiseTimes):
  gather_ms     the gather kernel (tile and surface buffers -> row-major inputs)
  prologue_ms   the guide prologue on its own
  scene_filter_ms  the K iterations and the output kernel
  scene_wall_ms the host wall time of the whole call (it synchronises and copies the result to the host)
Kernel-level statistics come from a separate `rocprofv3 --kernel-trace --stats` run, never from this timed one."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(run, reps, warmup):
    import torch
    for _ in range(warmup):
        run()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def scene_times(R, demo, W, H, args) -> dict:
    """rtHipSceneDenoise on a W x H demo room at S = 1: medians of its stage events and of its wall time."""
    sc = demo.room_scene(W, H, samples=1)
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    rs = R.ResidentScene(sc, 0)
    try:
        rs.set_passes(normal=True, albedo=True)
        rs.render()
        for _ in range(args.warmup):
            rs.denoise(iterations=args.iterations)
        stages, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rs.denoise(iterations=args.iterations)
            wall.append(1e3 * (time.perf_counter() - t0))
            stages.append(rs.denoise_times_ms())
    finally:
        rs.close()
    med = lambda k: round(float(np.median([t[k] for t in stages])), 4)  # noqa: E731
    return {"gather_ms": med("gather"), "prologue_ms": med("prologue"), "scene_filter_ms": med("filter"),
            "scene_wall_ms": round(float(np.median(wall)), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    from opencl_render_amd import demo, raytrace as R

    L = R.lib()
    result = {"iterations": args.iterations}
    for name, (W, H) in (("1080p", (1920, 1080)), ("4k", (3840, 2160))):
        rng = np.random.default_rng(1)
        ins = [torch.from_numpy(rng.random((H, W, 3), dtype=np.float32)).cuda() for _ in range(3)]
        out = torch.empty_like(ins[0])
        nbytes = L.rtHipDenoiseScratchBytes(W, H)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream or None

        def call(k):
            p = R.denoise_params(iterations=k)
            ptrs = [C.c_void_p(t.data_ptr()) for t in ins]
            rc = L.rtHipDenoiseDevice(0, W, H, *ptrs, C.c_void_p(out.data_ptr()), C.c_void_p(scratch.data_ptr()), nbytes, C.byref(p),
                                      stream and C.c_void_p(stream))
            if rc != 0:
                raise RuntimeError(R.last_error())

        full = event_ms(lambda: call(args.iterations), args.reps, args.warmup)
        k0 = event_ms(lambda: call(0), args.reps, args.warmup)
        result[name] = {"call_ms": round(full, 4), "k0_ms": round(k0, 4),
                        "iter_us": round(1e3 * (full - k0) / max(args.iterations, 1), 2)}
        if name == "1080p":  # what each iteration adds: h = 1, 2, 4, ...
            ks = [k0] + [event_ms(lambda k=k: call(k), args.reps, args.warmup) for k in range(1, args.iterations + 1)]
            result[name]["iter_us_by_h"] = {str(1 << i): round(1e3 * (ks[i + 1] - ks[i]), 1) for i in range(args.iterations)}
        del ins, out, scratch
        result[name].update(scene_times(R, demo, W, H, args))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
