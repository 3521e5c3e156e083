"""bench_geometry.py -- changing a resident scene's shape (rtHipSceneSetGeometry) on the headline 1M-triangle soup at 1920x1080, S = 1.

Every step displaces every vertex by a sine wave along x whose amplitude is 3 % of the scene's extent and whose phase advances per step,
so the split planes and most cells change.  Medians of `--reps` interleaved repetitions of
  (a) set_vertices from host arrays,
  (b) set_vertices from torch tensors that are already on the device,
  (c) the other route in the same process: build_scene_grid_device + build_camera_list_device on the host arrays, a new ResidentScene,
      destroy of the old one;
the first update's cost and what the scene grows by; the per-stage stream times of (a) and (b); update + frame + readback per second
over a 32-step animation for (b) and (c); and the planned frame after an update against that of a scene created fresh from the same
arrays, A/B interleaved, kernel_time_ms(), the fresh scene's own spread being the yardstick.
Prints one JSON line.  One process; at most 16 CPU threads."""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library loads its HIP runtime: the order bench.py uses)


def med(v):
    return round(float(np.median(v)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--triangles", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--baseline-steps", type=int, default=8)
    args = ap.parse_args()
    from opencl_render_amd import raytrace as R, scene as S

    sc = S.make_soup(1920, 1080, args.triangles, 0.004, seed=12345, name="lambert_1m")
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    lo, hi = sc.vertex[:, :3].min(0), sc.vertex[:, :3].max(0)
    extent = float(np.linalg.norm(hi - lo))
    amp, wave = 0.03 * extent, 2 * np.pi / (0.25 * extent)

    def displaced(step):
        v = sc.vertex.copy()
        ph = 2 * np.pi * step / args.steps
        v[:, 1] += (amp * np.sin(wave * sc.vertex[:, 0].astype(np.float64) + ph)).astype(np.float32)
        v[:, 2] += (amp * np.cos(wave * sc.vertex[:, 1].astype(np.float64) + ph)).astype(np.float32)
        return v

    dev = torch.device("cuda", 0)
    host = [displaced(i) for i in range(args.steps)]
    tens = [torch.from_numpy(v).to(dev) for v in host]
    torch.cuda.synchronize()

    def timed_update(rs, v):
        t = time.perf_counter()
        rs.set_vertices(v)
        return (1e3 * (time.perf_counter() - t),) + tuple(rs.geometry_times_ms()[k] for k in ("records", "grid", "dense", "camera"))

    def rebuilt(old, v):
        """route (c): both device builders on the host arrays, a new scene, the old one destroyed"""
        t = time.perf_counter()
        s = copy.copy(sc)
        s.vertex = v
        grid_ms = R.build_scene_grid_device(s, 0)
        cam_ms = R.build_camera_list_device(s, 0)
        new = R.ResidentScene(s, 0)
        old.close()
        return new, 1e3 * (time.perf_counter() - t), grid_ms, cam_ms

    # ---- the update ----
    a = R.ResidentScene(sc, 0)
    a.render(); a.readback()
    bytes_created = a.bytes()
    t = time.perf_counter()
    a.set_vertices(host[1], sc.tri_index)
    first_wall = 1e3 * (time.perf_counter() - t)
    first_ms, first_log, bytes_first = a.geometry_times_ms(), a.geometry_log(), a.bytes()
    b = R.ResidentScene(sc, 0)
    b.set_vertices(tens[1], torch.from_numpy(sc.tri_index).to(dev))
    c = R.ResidentScene(sc, 0)
    ta, tb, tc = [], [], []
    for i in range(args.reps):
        k = 2 + i % 2  # back and forth between two shapes
        ta.append(timed_update(a, host[k]))
        tb.append(timed_update(b, tens[k]))
        c, wall, grid_ms, cam_ms = rebuilt(c, host[k])
        tc.append((wall, grid_ms, cam_ms))
    ta, tb, tc = np.array(ta), np.array(tb), np.array(tc)
    stages = ("wall_ms", "records_ms", "grid_ms", "dense_ms", "camera_ms")
    update = dict(first=dict(wall_ms=round(first_wall, 3), stages_ms={k: round(v, 4) for k, v in first_ms.items()}, log=first_log),
                  host_arrays={k: med(ta[:, i]) for i, k in enumerate(stages)}, device_tensors={k: med(tb[:, i]) for i, k in enumerate(stages)},
                  rebuilt=dict(wall_ms=med(tc[:, 0]), grid_device_ms=med(tc[:, 1]), camera_device_ms=med(tc[:, 2])),
                  wall_ratio_host=round(float(np.median(tc[:, 0]) / np.median(ta[:, 0])), 2),
                  wall_ratio_device=round(float(np.median(tc[:, 0]) / np.median(tb[:, 0])), 2),
                  allocated_in_steady_state=a.geometry_log()["allocated"], pairs=a.geometry_log()["pairs"], entries=a.geometry_log()["entries"],
                  bytes_created=bytes_created, bytes_after_first_update=bytes_first, bytes_after_updates=a.bytes())
    a.close()

    # ---- the frame after an update ----
    fresh_sc = copy.copy(sc)
    fresh_sc.vertex = host[3]
    R.build_scene_grid_device(fresh_sc, 0)
    R.build_camera_list_device(fresh_sc, 0)
    fresh = R.ResidentScene(fresh_sc, 0)
    b.set_vertices(tens[3])
    times = {"updated": [], "fresh": []}
    for rs in (b, fresh):  # the watched frame, then one planned frame as a warm-up
        for _ in range(2):
            rs.render(); rs.sync(); rs.finish()
        rs.kernel_time_ms()
    same = all(np.array_equal(x, y) for x, y in zip(b.readback(), fresh.readback()))
    for _ in range(max(args.reps, 10)):
        for key, rs in (("updated", b), ("fresh", fresh)):
            rs.render(); rs.sync(); rs.finish()
            times[key].append(rs.kernel_time_ms()[0])
    f = np.array(times["fresh"])
    frame = dict(updated_ms=med(times["updated"]), fresh_ms=med(f), fresh_min_ms=round(float(f.min()), 4), fresh_max_ms=round(float(f.max()), 4),
                 fresh_iqr_ms=round(float(np.percentile(f, 75) - np.percentile(f, 25)), 4), planes_equal=bool(same))
    fresh.close()

    # ---- animation ----
    planes = [np.zeros(sc.pixels, np.uint16) for _ in range(3)]
    t = time.perf_counter()
    for i in range(args.steps):
        b.set_vertices(tens[i])
        b.render()
        for p in planes:
            p[:] = 0
        b.readback(planes)
    anim = time.perf_counter() - t
    b.close()
    n = min(args.baseline_steps, args.steps)
    t = time.perf_counter()
    for i in range(n):
        c, _, _, _ = rebuilt(c, host[i])
        c.render()
        for p in planes:
            p[:] = 0
        c.readback(planes)
    base = time.perf_counter() - t
    c.close()
    animation = dict(steps=args.steps, fps=round(args.steps / anim, 2), rebuilt_steps=n, rebuilt_fps=round(n / base, 2))
    print(json.dumps(dict(bench="geometry_update", scene="lambert_1m", triangles=args.triangles, width=sc.width, height=sc.height, reps=args.reps,
                          amplitude=round(amp, 5), time=time.strftime("%Y-%m-%d %H:%M:%S"), update=update, frame=frame, animation=animation)))


if __name__ == "__main__":
    main()
