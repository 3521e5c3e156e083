"""bench_edit.py -- editing a resident scene's lights, materials and material ids (rtHipSceneSetLights / rtHipSceneSetMaterials) on the
headline 1M-triangle soup at 1920x1080, S = 1, against creating the scene again in the same process.

Medians (and the spread) of `--reps` interleaved repetitions of
  (a) set_lights: the one distant light, turned a little every time,
  (b) set_materials with the headline's tables and atlas (one Lambert material),
  (c) set_materials(tri_material=...): all T ids reassigned, from a host array and from a torch tensor that is already on the device,
  (d) ResidentScene(sc) -- the only route before these calls -- and the old scene's destruction,
wall time around each call (a call is synchronous on the scene's stream) and edit_times_ms(), the device time of the edit's own stages.
A planned frame is rendered between the repetitions, so that every edit meets a scene with a launch plan and frames behind it.  At the
end the edited scene's frame is compared with a fresh scene's of the same description.
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


def spread(v):
    v = np.asarray(v, np.float64)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4),
                iqr=round(float(np.percentile(v, 75) - np.percentile(v, 25)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--triangles", type=int, default=1_000_000)
    args = ap.parse_args()
    from opencl_render_amd import raytrace as R, scene as S

    sc = S.make_soup(1920, 1080, args.triangles, 0.004, seed=12345, name="lambert_1m")
    R.build_camera_list_device(sc, 0)
    R.build_scene_grid_device(sc, 0)
    T = sc.triangle_count
    lights = R.scene_lights(sc)
    tables = dict(mat_size=sc.mat_size, mat_start=sc.mat_start, textures=sc.textures)
    dev = torch.device("cuda", 0)
    ids_host = [np.where(np.arange(T) % (3 + k) == 0, -1, 0).astype(np.int32) for k in range(2)]  # (one material: ids 0 or -1)
    ids_dev = [torch.from_numpy(a).to(dev) for a in ids_host]
    torch.cuda.synchronize()

    def timed(call, key=None):
        t = time.perf_counter()
        call()
        wall = 1e3 * (time.perf_counter() - t)
        return (wall, rs.edit_times_ms()[key]) if key else (wall,)

    def settle():  # a planned frame behind every edit
        rs.render(); rs.sync(); rs.finish()

    rs = R.ResidentScene(sc, 0)
    for _ in range(2):  # the watched frame, then a planned one
        settle()
    bytes_created = rs.bytes()
    first = dict(lights_ms=round(timed(lambda: rs.set_lights(R.relight(lights, 1, 360)))[0], 4),
                 materials_ms=round(timed(lambda: rs.set_materials(tables))[0], 4),
                 ids_host_ms=round(timed(lambda: rs.set_materials(tri_material=ids_host[0]))[0], 4))
    bytes_first = rs.bytes()
    out = {k: [] for k in ("lights", "materials", "ids_host", "ids_device", "create")}
    other = None
    for i in range(args.reps):
        settle()
        out["lights"].append(timed(lambda: rs.set_lights(R.relight(lights, 2 + i, 360)), "lights"))
        settle()
        out["materials"].append(timed(lambda: rs.set_materials(tables), "materials"))
        settle()
        out["ids_host"].append(timed(lambda: rs.set_materials(tri_material=ids_host[i % 2]), "ids"))
        settle()
        out["ids_device"].append(timed(lambda: rs.set_materials(tri_material=ids_dev[(i + 1) % 2]), "ids"))
        t = time.perf_counter()
        new = R.ResidentScene(sc, 0)
        if other is not None:
            other.close()
        out["create"].append((1e3 * (time.perf_counter() - t),))
        other = new
    if other is not None:
        other.close()
    bytes_steady = rs.bytes()
    # the edited scene against a fresh one of the same description
    final_lights, final_ids = R.relight(lights, 1 + args.reps, 360), ids_host[args.reps % 2]
    rs.set_lights(final_lights)
    rs.set_materials(tri_material=final_ids)
    rs.render()
    got = rs.readback()
    rs.close()
    twin = copy.copy(sc)
    for k, v in final_lights.items():
        setattr(twin, k, v)
    twin.tri_material = final_ids
    fr = R.ResidentScene(twin, 0)
    fr.render()
    want = fr.readback()
    fr.close()
    same = all(np.array_equal(x, y) for x, y in zip(got, want))

    res = {k: dict(wall_ms=spread([r[0] for r in v]), **({"device_ms": spread([r[1] for r in v])} if len(v[0]) > 1 else {})) for k, v in out.items()}
    create = res["create"]["wall_ms"]["median"]
    for k in ("lights", "materials", "ids_host", "ids_device"):
        res[k]["create_over_edit"] = round(create / res[k]["wall_ms"]["median"], 1)
    print(json.dumps(dict(bench="scene_edit", scene="lambert_1m", triangles=T, width=sc.width, height=sc.height, reps=args.reps,
                          time=time.strftime("%Y-%m-%d %H:%M:%S"), first_edit=first, bytes_created=bytes_created, bytes_after_first_edits=bytes_first,
                          bytes_after_edits=bytes_steady, planes_equal=bool(same), **res)))


if __name__ == "__main__":
    main()
