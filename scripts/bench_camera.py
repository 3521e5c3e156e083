"""bench_camera.py -- moving a resident scene's camera (rtHipSceneSetCamera) on the headline 1M-triangle soup at 1920x1080, S = 1.

  move:       a 5-degree orbit step about the vertical axis through the soup's middle: host wall time of the call and the device time of
              its two stages (HIP events on the scene's stream), the first move (which makes the build storage) apart.  Interleaved with
              the route without it: build_camera_list_device on the host arrays + ResidentScene(like=old) + destroy of the old one.
  frame:      the planned frame of the moved scene against that of a scene created at the same pose from host-built, de-duplicated
              lists, A/B interleaved, kernel_time_ms(); the fresh scene's own spread is the margin.
  turntable:  72 poses of move + frame + readback end to end, next to at most 8 poses of the other route.
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

CENTRE = np.array([0.0, 0.0, 3.0])


def orbit(sc, degrees):
    """A copy of the scene with its camera turned about the vertical axis through CENTRE (no lists)."""
    a = np.deg2rad(degrees)
    m = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    out = copy.copy(sc)

    def f4(v):
        r = np.zeros(4, np.float32)
        r[:3] = v
        return r
    out.eye = f4(CENTRE + m @ (np.float64(sc.eye[:3]) - CENTRE))
    out.eye_to_top_left, out.left_to_right, out.top_to_bottom = (f4(m @ np.float64(v[:3])) for v in (sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom))
    out.cam_start = out.cam_end = out.cam_list = None
    return out


def med(v):
    return round(float(np.median(v)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--triangles", type=int, default=1_000_000)
    ap.add_argument("--poses", type=int, default=72)
    ap.add_argument("--baseline-poses", type=int, default=8)
    args = ap.parse_args()
    from opencl_render_amd import raytrace as R, scene as S

    sc = S.make_soup(1920, 1080, args.triangles, 0.004, seed=12345, name="lambert_1m")
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)

    def cam(s):
        return s.eye, s.eye_to_top_left, s.left_to_right, s.top_to_bottom, s.pixel_size_inv

    def timed_move(rs, s):
        t = time.perf_counter()
        rs.set_camera(*cam(s))
        wall = 1e3 * (time.perf_counter() - t)
        ms = rs.camera_times_ms()
        return wall, ms["count"], ms["fill"]

    def rebuilt(old, s):
        """the route without the move: lists built on the device from the host arrays, a new instance beside the old one, the old one destroyed"""
        t = time.perf_counter()
        dev_ms = R.build_camera_list_device(s, 0)
        new = R.ResidentScene(s, 0, like=old)
        old.close()
        return new, 1e3 * (time.perf_counter() - t), dev_ms

    # ---- the move ----
    moved = R.ResidentScene(sc, 0)
    moved.render(); moved.readback()
    bytes_created = moved.bytes()
    first = timed_move(moved, orbit(sc, 5.0))
    bytes_moved = moved.bytes()
    other = R.ResidentScene(sc, 0)
    steps = [orbit(sc, 5.0 * (i % 2)) for i in range(args.reps)]  # back and forth by one step
    mv, rb = [], []
    for s in steps:
        mv.append(timed_move(moved, s))
        other, wall, dev_ms = rebuilt(other, s)
        rb.append((wall, dev_ms))
    other.close()
    mv, rb = np.array(mv), np.array(rb)
    move = dict(first=dict(wall_ms=round(first[0], 3), device_count_ms=round(first[1], 4), device_fill_ms=round(first[2], 4)),
                wall_ms=med(mv[:, 0]), device_ms=med(mv[:, 1] + mv[:, 2]), device_count_ms=med(mv[:, 1]), device_fill_ms=med(mv[:, 2]),
                rebuilt_wall_ms=med(rb[:, 0]), rebuilt_list_device_ms=med(rb[:, 1]), wall_ratio=round(float(np.median(rb[:, 0]) / np.median(mv[:, 0])), 2),
                bytes_created=bytes_created, bytes_after_first_move=bytes_moved, bytes_after_moves=moved.bytes())

    # ---- the frame after a move ----
    pose = orbit(sc, 5.0)
    moved.set_camera(*cam(pose))
    fresh_sc = copy.copy(pose)
    R.build_camera_list_device(fresh_sc, 0)
    fresh = R.ResidentScene(fresh_sc, 0)
    times = {"moved": [], "fresh": []}
    for rs in (moved, fresh):  # the watched frame, then one planned frame as a warm-up
        for _ in range(2):
            rs.render(); rs.sync(); rs.finish()
        rs.kernel_time_ms()
    same = all(np.array_equal(a, b) for a, b in zip(moved.readback(), fresh.readback()))
    for _ in range(max(args.reps, 10)):
        for key, rs in (("moved", moved), ("fresh", fresh)):
            rs.render(); rs.sync(); rs.finish()
            times[key].append(rs.kernel_time_ms()[0])
    f = np.array(times["fresh"])
    frame = dict(moved_ms=med(times["moved"]), fresh_ms=med(f), fresh_min_ms=round(float(f.min()), 4), fresh_max_ms=round(float(f.max()), 4),
                 fresh_iqr_ms=round(float(np.percentile(f, 75) - np.percentile(f, 25)), 4), moved_entries=moved.camera_log()["entries"],
                 fresh_entries=int(len(fresh_sc.cam_list)), planes_equal=bool(same))
    fresh.close()

    # ---- turntable ----
    planes = [np.zeros(sc.pixels, np.uint16) for _ in range(3)]
    t = time.perf_counter()
    for i in range(args.poses):
        moved.set_camera(*cam(orbit(sc, 360.0 * i / args.poses)))
        moved.render()
        for p in planes:
            p[:] = 0
        moved.readback(planes)
    turn = time.perf_counter() - t
    moved.close()
    n = min(args.baseline_poses, args.poses)
    other = R.ResidentScene(sc, 0)
    t = time.perf_counter()
    for i in range(n):
        other, _, _ = rebuilt(other, orbit(sc, 360.0 * i / args.poses))
        other.render()
        for p in planes:
            p[:] = 0
        other.readback(planes)
    base = time.perf_counter() - t
    other.close()
    turntable = dict(poses=args.poses, fps=round(args.poses / turn, 2), rebuilt_poses=n, rebuilt_fps=round(n / base, 2))
    print(json.dumps(dict(bench="camera_move", scene="lambert_1m", triangles=args.triangles, width=sc.width, height=sc.height, reps=args.reps,
                          time=time.strftime("%Y-%m-%d %H:%M:%S"), move=move, frame=frame, turntable=turntable)))


if __name__ == "__main__":
    main()
