"""bench_query.py -- ray queries (ResidentScene.intersect, device entry point) on the headline 1M-triangle soup at 1920x1080.

Three ray sets, each traced from device tensors; per set the device entry point alone on rays already packed on the device ("query": the
kernel's cost) and ResidentScene.intersect end to end ("call": packing, query, derived outputs):
  (a) primary:  the eye through every pixel centre;
  (b) random:   origins uniform in the grid's box, directions uniform on the sphere;
  (c) shadow:   segments from (a)'s hits to a point light above the scene, tmax = 1, the source triangle excluded.
Next to them: the trace stage's rays/s of a rendered frame of the same scene (stage_times_ms, round_rays).
Prints one JSON line.  One process; at most 16 CPU threads (list builders)."""
import argparse
import ctypes as C
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
    ap.add_argument("--random-rays", type=int, default=2_000_000)
    args = ap.parse_args()
    import torch
    from opencl_render_amd import raytrace as R, scene as S

    sc = S.make_soup(1920, 1080, args.triangles, 0.004, seed=12345, name="lambert_1m")
    R.build_lists(sc, threads=16)
    rs = R.ResidentScene(sc)
    dev = torch.device("cuda", 0)
    f32 = np.float32

    W, H = sc.width, sc.height
    p = np.arange(W * H)
    x, y = (p % W).astype(f32) + f32(0.5), (p // W).astype(f32) + f32(0.5)
    tl, lr, tb = (np.asarray(v, f32)[:3] for v in (sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom))
    d = tl[None, :] + lr[None, :] * x[:, None]
    d = d + tb[None, :] * y[:, None]
    o = np.broadcast_to(np.asarray(sc.eye, f32)[:3], d.shape).copy()
    box = np.asarray(sc.box_min, f32)
    lo, hi = box[0, :3], box[256, :3]
    rng = np.random.default_rng(1)
    ro = (lo + rng.random((args.random_rays, 3)) * (hi - lo)).astype(f32)
    rd = rng.normal(size=(args.random_rays, 3)).astype(f32)
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)

    run = torch.cuda.Stream(dev)  # a stream of its own: the library takes a NULL stream for the scene's stream

    def timed(oo, dd, tmax=np.inf, exclude=None):
        """Two figures per set: `query` = the device entry point alone on rays already packed on the device (what the kernel costs), and
        `call` = ResidentScene.intersect end to end (packing, the query, the derived outputs)."""
        to, td = torch.from_numpy(oo).to(dev), torch.from_numpy(dd).to(dev)
        tt = tmax if np.isscalar(tmax) else torch.from_numpy(tmax).to(dev)
        te = None if exclude is None else torch.from_numpy(exclude.view(np.int32)).to(dev)
        n = len(oo)
        rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        rays[:, 0:3] = to
        rays[:, 3] = 0.0
        rays[:, 4:7] = td
        rays[:, 7] = tt
        hits = torch.empty((n, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        L = R.lib()
        excl = None if te is None else C.c_void_p(te.data_ptr())

        def query():
            if L.rtHipSceneIntersectDevice(rs.handle, C.c_void_p(rays.data_ptr()), excl, n, C.c_void_p(hits.data_ptr()), C.c_void_p(run.cuda_stream)):
                raise RuntimeError(R.last_error())

        def call():
            return rs.intersect(to, td, 0.0, tt, te)

        figures = {}
        with torch.cuda.stream(run):
            out = call()  # warm-up (and the answer)
            query()
            for key, fn in (("query", query), ("call", call)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.reps):
                    fn()
                b.record()
                torch.cuda.synchronize()
                ms = a.elapsed_time(b) / args.reps
                figures[key] = dict(ms=round(ms, 4), rays_per_s=round(n / (ms * 1e-3), 1))
        return out, dict(rays=n, hit_rate=round(float(out["hit"].float().mean()), 4), **figures)

    res = {}
    prim, res["primary"] = timed(o, d)
    res["random"] = timed(ro, rd)[1]
    hit = prim["hit"].cpu().numpy()
    pos = prim["position"].cpu().numpy()[hit]
    light = np.array([0.0, 3.0, 1.0], f32)
    tri = prim["triangle"].view(torch.int32).cpu().numpy().view(np.uint32)[hit]
    res["shadow"] = timed(pos, (light[None, :] - pos).astype(f32), np.ones(len(pos), f32), tri)[1]

    # the trace stage of a frame of the same scene
    rs.render()
    rs.sync()
    rs.stage_timing(True)
    rs.render()
    rs.sync()
    stage, rounds = rs.stage_times_ms()
    rays = sum(rs.round_rays(64)[1:])
    res["frame_trace_stage"] = dict(ms=round(stage["trace"], 4), rays=int(rays), rounds=int(rounds),
                                    rays_per_s=round(rays / (stage["trace"] * 1e-3), 1) if stage["trace"] > 0 else None)
    rs.close()
    print(json.dumps(dict(bench="ray_queries", scene="lambert_1m", triangles=args.triangles, width=W, height=H, reps=args.reps,
                          time=time.strftime("%Y-%m-%d %H:%M:%S"), **res)))


if __name__ == "__main__":
    main()
