"""bench_window.py -- what rendering in sample windows costs on the headline 1M-triangle soup at 1920x1080 (include/raytrace_hip.h,
"SAMPLE WINDOWS").

  whole:        one frame of a scene created with S = 16 (the default window), planned, kernel_time_ms().
  progressive:  the same image as 16 frames of a scene created with S = 1 under the progressive window {16, 0, 16, 1, 1}: the first frame
                starts from zero and may be planned, the fifteen that continue from the tile buffer are watched (they cannot be redone),
                and every frame after the first goes through sampleOut and the accumulate kernel.  Sum of the frames' kernel times, and
                the wall time of the 16 frames with one synchronisation at the end.
  sequence:     16 planned frames of the S = 1 scene under the sequence window {16, 0, 1, 0, 1} next to 16 under the default window: what
                a fresh set of samples per frame costs (nothing but other sample ids).
The planes of `progressive` are compared with those of `whole`.  Reported, not gated.  Prints one JSON line.  One process."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def med(v):
    return round(float(np.median(v)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--triangles", type=int, default=1_000_000)
    ap.add_argument("--total", type=int, default=16)
    args = ap.parse_args()
    import dataclasses

    from opencl_render_amd import raytrace as R, scene as S

    N = args.total
    one = S.make_soup(1920, 1080, args.triangles, 0.004, seed=12345, samples=1, name="lambert_1m")
    R.build_camera_list_device(one, 0)
    R.build_scene_grid_device(one, 0)
    many = dataclasses.replace(one, sample_count=N)

    def frame_ms(rs):
        rs.render(); rs.sync(); rs.finish()
        return rs.kernel_time_ms()[0]

    whole = R.ResidentScene(many, 0)
    for _ in range(2):  # the watched frame, then one planned frame as a warm-up
        frame_ms(whole)
    whole_ms = [frame_ms(whole) for _ in range(args.reps)]
    want = whole.readback()
    whole.close()

    rs = R.ResidentScene(one, 0)
    for _ in range(2):
        frame_ms(rs)
    default_ms = [sum(frame_ms(rs) for _ in range(N)) for _ in range(args.reps)]
    rs.set_sample_window(N, 0, 1, advance=True)
    sequence_ms = [sum(frame_ms(rs) for _ in range(N)) for _ in range(args.reps)]
    progressive_ms, progressive_wall = [], []
    for _ in range(args.reps):
        rs.set_sample_window(N, 0, N, accumulate=True, advance=True)
        progressive_ms.append(sum(frame_ms(rs) for _ in range(N)))
        rs.set_sample_window(N, 0, N, accumulate=True, advance=True)
        t = time.perf_counter()
        for _ in range(N):
            rs.render()
        rs.sync()
        progressive_wall.append(1e3 * (time.perf_counter() - t))
    same = all(np.array_equal(a, b) for a, b in zip(rs.readback(), want))
    rs.close()
    print(json.dumps(dict(bench="sample_window", scene="lambert_1m", triangles=args.triangles, width=one.width, height=one.height, total=N,
                          reps=args.reps, time=time.strftime("%Y-%m-%d %H:%M:%S"), whole_frame_ms=med(whole_ms),
                          progressive_kernels_ms=med(progressive_ms), progressive_wall_ms=med(progressive_wall),
                          progressive_over_whole=round(float(np.median(progressive_ms) / np.median(whole_ms)), 3),
                          sequence_frames_ms=med(sequence_ms), default_frames_ms=med(default_ms), planes_equal=bool(same))))


if __name__ == "__main__":
    main()
