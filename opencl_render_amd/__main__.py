"""Headless harness: ``python -m opencl_render_amd --scene room --width 640 --height 480 --samples 16 --out room.bmp``.

The counterpart of the plugin's dialog fields (image size, samples per pixel, device: reference ``source/render.cpp:174-186``)
and of the tail of ``parseAndRender`` (``render.cpp:1311-1397``): build a scene through the front-end, build both lists on the
GPU, render through the drop-in ``RaytraceAll`` and write the image the way the reference does (BMP in ``writebmp3s``'s layout,
or PPM).  Needs an MI355X: there is no CPU fallback.

``--passes PREFIX`` renders through the resident layer instead (one instance per GPU over a tile deal for the all-GPUs device) and
also writes the render passes: PREFIX_alpha.pgm (coverage), PREFIX_depth.pfm (eye-to-hit distance of sample 1) and PREFIX_ids.npz
(triangle, material and mesh ids of sample 1's hit; -1 -- 0xffffffff for the triangle -- where it missed).  With
``--surface-passes`` it also writes PREFIX_normal.pfm and PREFIX_albedo.pfm (colour PFMs of the shading normal and the albedo at the
primary hit, means over the pixel's samples: a denoiser's auxiliary images).

``--denoise PATH`` renders through the resident layer with the normal and albedo passes on and writes the frame denoised by the
built-in edge-aware filter (include/raytrace_hip.h, "DENOISER", default parameters) to PATH: .bmp / .ppm (u16 planes) or .pfm (the
f32 colour).  ``--out`` is still the noisy beauty.  For the all-GPUs device the instances' read-backs are composed on the host and
denoised with rtHipDenoise on device 0.

``--ao PATH`` also writes the scene's ambient occlusion (include/raytrace_hip.h, "AMBIENT OCCLUSION"), traced on the device from the
scene's camera, to PATH: .pfm (f32) or .pgm (u16 quantised like the denoiser's output, written as 8 bits).  ``--ao-rays``,
``--ao-radius``, ``--ao-samples`` and ``--ao-seed`` set its parameters.  For the all-GPUs device it runs on device 0.

``--motion PREFIX`` (with ``--orbit N`` or ``--spin N``) also writes every frame's motion vectors (include/raytrace_hip.h, "MOTION
VECTORS") against the frame before it to PREFIX_000.npz .. PREFIX_{N-1}.npz.

``--temporal PATH`` (with ``--orbit N``, ``--spin N`` or ``--relight N``) also writes every frame accumulated over the frames before it (include/raytrace_hip.h,
"TEMPORAL ACCUMULATION"; ResidentScene.temporal) to PATH_000 .. PATH_{N-1}: .bmp, .ppm or .pfm.  With ``--denoise`` the denoiser runs on
the accumulation before it is written.  ``--variance-guided`` (beside ``--temporal PATH``) carries the luminance moments along and
runs the variance-guided filter (include/raytrace_hip.h, "VARIANCE-GUIDED FILTER"; ResidentScene.temporal_variance) on the accumulation
in the denoiser's place; ``--variance PATH`` also writes each frame's variance (V^K with the filter) as .pfm, numbered the same way.
``--temporal-clamp [GAMMA]`` (beside ``--temporal PATH``) turns the scene's temporal clamp on (include/raytrace_hip.h, "TEMPORAL CLAMP";
ResidentScene.set_temporal_clamp): the reprojected history is pulled into the frame's 3x3 colour box before the blend, GAMMA (default 1)
standard deviations wide; ``--temporal-clamp-mode minmax|variance|both`` (default both) chooses the box.  ``--relight N --temporal PATH``
shows what it is for: without the clamp the old lighting fades out over the history's length, with it the accumulation follows the
light at once.

``--motion-blur PATH`` (with ``--orbit N`` or ``--spin N``) also writes every frame blurred along its motion vectors to the frame before
it (include/raytrace_hip.h, "MOTION BLUR"; ResidentScene.motion_blur) to PATH_000 .. PATH_{N-1}: .bmp, .ppm or .pfm; frame 0 is written
unblurred.  ``--shutter S``, ``--max-blur PX`` and ``--blur-taps N`` set its parameters.  Beside ``--temporal`` the blur runs first:
the accumulation marks the scene again.

``--dof PATH`` also writes the frame blurred by its depth pass's circle of confusion (include/raytrace_hip.h, "DEPTH OF FIELD";
ResidentScene.depth_of_field) to PATH: .bmp, .ppm or .pfm, numbered like --out under ``--orbit`` / ``--spin`` / ``--relight``.  ``--aperture A``
is the lens radius in scene units; the distance in focus is ``--focus D`` (along the ray) or the depth of pixel ``--focus-pixel X Y`` of
every frame; ``--dof-rings N`` and ``--max-coc PX`` set the tap rings and the cap of the blur radius.  The depth pass is turned on by itself.

``--relight N`` renders N frames of the one resident scene with its first light turned about the vertical axis between them
(include/raytrace_hip.h, "SCENE EDITS: LIGHTS AND MATERIALS"; ResidentScene.set_lights): img_000 .. img_{N-1}, with ``--passes`` /
``--denoise`` / ``--ao`` numbered alike.

``--bake-ao PATH`` also bakes ambient occlusion into a texture over the scene's UVs (include/raytrace_hip.h, "AMBIENT OCCLUSION
BAKE") and writes it to PATH like ``--ao``: .pfm (f32) or .pgm (8 bits).  ``--bake-size W H`` (default 512 512), ``--bake-rays``,
``--bake-radius``, ``--bake-seed`` and ``--bake-dilate`` set its parameters; ``--bake-material M`` or ``--bake-triangles FIRST COUNT``
selects what is baked; ``--bake-atlas`` bakes over a grid atlas (scene.grid_atlas_uv) instead of the scene's own UVs.  For the
all-GPUs device it runs on device 0.

``--progressive N`` renders N samples per pixel in N / S frames of S (S = ``--samples``) on the one resident scene (include/raytrace_hip.h,
"SAMPLE WINDOWS"; ResidentScene.progressive): ``--out img.bmp`` is the finished image, equal to the ``--samples N`` image, and after each
frame but the last a preview img_000.bmp, img_001.bmp .. is written, the tile buffer scaled by N / done on the host.  ``--sequence N``
(with ``--orbit N``, ``--spin N`` or ``--temporal PATH``) gives the frames the sequence window: frame i draws S fresh samples per pixel of
a sequence of N, so that the temporal chain has something to average under a still or slowly moving camera.

``--mattes PREFIX`` also writes anti-aliased id mattes over the frame's own samples (include/raytrace_hip.h, "MATTES";
ResidentScene.mattes): one PREFIX_matte_<id>.pgm per ``--matte-select`` id (u16 = trunc(coverage * 65535)) and PREFIX_layers.npz with the
``--matte-layers K`` ranked layers.  ``--matte-kind`` says what the ids are: mesh (the default; a scene not made of front-end meshes
counts as mesh 0), material or triangle.  Single views only; for the all-GPUs device it runs on device 0.
"""
import argparse
import sys
import time

import numpy as np


def matte_ids(text: str) -> tuple:
    """--matte-select: ID[,ID..] -> a tuple of u32 ids."""
    try:
        ids = tuple(int(v, 0) for v in text.split(",") if v.strip())
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not a comma-separated list of ids")
    if len(ids) > 16 or any(not 0 <= v < 0xFFFFFFFF for v in ids):
        raise argparse.ArgumentTypeError("at most 16 ids, each in 0 .. 2^32 - 2")
    return ids


def parser():
    ap = argparse.ArgumentParser(prog="python -m opencl_render_amd", description=__doc__.splitlines()[0])
    ap.add_argument("--scene", choices=["room", "soup"], default="room", help="demo room (meshes through the front-end) or a seeded triangle soup")
    ap.add_argument("--obj", help="render this Wavefront OBJ (its MTL libraries and PPM / BMP textures are read too) instead of a demo scene")
    ap.add_argument("--eye", type=float, nargs=3, default=None, help="--obj: camera position (default: in front of the model's bounding box)")
    ap.add_argument("--look-at", type=float, nargs=3, default=None, help="--obj: point the camera looks at (default: the bounding box's centre)")
    ap.add_argument("--fov", type=float, default=50.0, help="--obj: horizontal field of view in degrees")
    ap.add_argument("--light-dir", type=float, nargs=3, default=(0.3, -0.8, 0.5), help="--obj: direction of the one distant light")
    ap.add_argument("--width", type=int, default=1024)   # the dialog's defaults (render.cpp:176-182)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--triangles", type=int, default=100_000, help="soup only")
    ap.add_argument("--device", type=int, default=1, help="computationType: 1..N = HIP device, N+1 = all GPUs (tiled)")
    ap.add_argument("--out", default="img.bmp", help=".bmp or .ppm")
    ap.add_argument("--low-byte-compat", action="store_true", help="BMP only: keep the low byte of every u16 like the reference's writebmp3s")
    ap.add_argument("--passes", metavar="PREFIX", help="also write PREFIX_alpha.pgm, PREFIX_depth.pfm and PREFIX_ids.npz (render passes)")
    ap.add_argument("--surface-passes", action="store_true", help="with --passes: also write PREFIX_normal.pfm and PREFIX_albedo.pfm")
    ap.add_argument("--denoise", metavar="PATH", help="also write the denoised frame to PATH (.bmp, .ppm or .pfm)")
    ap.add_argument("--ao", metavar="PATH", help="also write the ambient occlusion image to PATH (.pfm or .pgm)")
    ap.add_argument("--ao-rays", type=int, default=16, help="--ao: hemisphere rays per pixel sample (1..256)")
    ap.add_argument("--ao-radius", type=float, default=float("inf"), help="--ao: how far an occluder counts (scene units; default: any distance)")
    ap.add_argument("--ao-samples", type=int, default=1, help="--ao: jittered primary samples per pixel (1..64)")
    ap.add_argument("--ao-seed", type=int, default=0, help="--ao: seed of the ray directions (u32)")
    ap.add_argument("--mattes", metavar="PREFIX",
                    help="also write anti-aliased id mattes over the frame's samples (include/raytrace_hip.h, \"MATTES\"): "
                         "PREFIX_matte_<id>.pgm per --matte-select id (u16 = trunc(coverage * 65535)) and PREFIX_layers.npz with layer_id, "
                         "layer_coverage [K, H, W] and rest [H, W].  Single views only")
    ap.add_argument("--matte-kind", choices=("mesh", "material", "triangle"), default="mesh", help="--mattes: what the ids are")
    ap.add_argument("--matte-select", type=matte_ids, default=(), metavar="ID[,ID..]", help="--mattes: up to 16 ids, one matte each")
    ap.add_argument("--matte-layers", type=int, default=4, metavar="K", help="--mattes: ranked layers per pixel (0..8)")
    ap.add_argument("--bake-ao", metavar="PATH", help="also bake ambient occlusion over the UVs into PATH (.pfm or .pgm)")
    ap.add_argument("--bake-size", type=int, nargs=2, metavar=("W", "H"), default=(512, 512), help="--bake-ao: texture size")
    ap.add_argument("--bake-rays", type=int, default=16, help="--bake-ao: hemisphere rays per texel (1..256)")
    ap.add_argument("--bake-radius", type=float, default=float("inf"), help="--bake-ao: how far an occluder counts (default: any distance)")
    ap.add_argument("--bake-seed", type=int, default=0, help="--bake-ao: seed of the ray directions (u32)")
    ap.add_argument("--bake-dilate", type=int, default=2, help="--bake-ao: gutter-fill passes (0..64)")
    sel = ap.add_mutually_exclusive_group()
    sel.add_argument("--bake-material", type=int, metavar="M", help="--bake-ao: bake only the triangles of material M")
    sel.add_argument("--bake-triangles", type=int, nargs=2, metavar=("FIRST", "COUNT"), help="--bake-ao: bake only these triangles")
    ap.add_argument("--bake-atlas", action="store_true", help="--bake-ao: bake over a grid atlas, one cell per triangle, not the scene's UVs")
    ap.add_argument("--motion", metavar="PREFIX",
                    help="with --orbit N or --spin N: also write every frame's motion vectors (include/raytrace_hip.h, \"MOTION VECTORS\") to "
                         "PREFIX_000.npz .. PREFIX_{N-1}.npz with the arrays motion [H, W, 2], t, prev_t and triangle [H, W].  Each frame is "
                         "measured against the state of the frame before it (frame 0 against itself): the scene is marked after each frame's outputs")
    ap.add_argument("--temporal", metavar="PATH",
                    help="with --orbit N or --spin N: also write every frame accumulated over the frames before it (ResidentScene.temporal: "
                         "the history reprojected along the motion vectors, default parameters) to PATH numbered like --out: .bmp, .ppm or "
                         ".pfm.  With --denoise the denoiser runs on the accumulation before it is written (the history stays unfiltered)")
    ap.add_argument("--motion-blur", metavar="PATH",
                    help="with --orbit N or --spin N: also write every frame blurred along its motion vectors to the frame before it "
                         "(ResidentScene.motion_blur) to PATH numbered like --out: .bmp, .ppm or .pfm.  Frame 0 has no frame before it and is "
                         "written unblurred")
    ap.add_argument("--shutter", type=float, default=None, metavar="S",
                    help="with --motion-blur: the share of the frame interval the exposure covers, 0..4 (default 0.5)")
    ap.add_argument("--max-blur", type=float, default=None, metavar="PX",
                    help="with --motion-blur: the longest half-extent of a streak in pixels, 1..32 (default 16)")
    ap.add_argument("--blur-taps", type=int, default=None, metavar="N", help="with --motion-blur: samples along a streak, 1..64 (default 15)")
    ap.add_argument("--dof", metavar="PATH",
                    help="also write the frame blurred by its depth pass's circle of confusion (ResidentScene.depth_of_field) to PATH: .bmp, "
                         ".ppm or .pfm, numbered like --out under --orbit / --spin / --relight.  Needs --aperture and --focus or --focus-pixel")
    ap.add_argument("--aperture", type=float, default=None, metavar="A", help="with --dof: the lens radius in scene units, >= 0")
    ap.add_argument("--focus", type=float, default=None, metavar="D", help="with --dof: the distance in focus, along the ray, > 0")
    ap.add_argument("--focus-pixel", type=int, nargs=2, default=None, metavar=("X", "Y"),
                    help="with --dof: focus on what pixel (X, Y) shows (its value in the depth pass); an error where its ray hits nothing")
    ap.add_argument("--dof-rings", type=int, default=None, metavar="N", help="with --dof: octagonal rings of taps, 1..6 (default 3)")
    ap.add_argument("--max-coc", type=float, default=None, metavar="PX", help="with --dof: the cap of the blur radius in pixels, 1..32 (default 16)")
    ap.add_argument("--temporal-clamp", type=float, nargs="?", const=1.0, default=None, metavar="GAMMA",
                    help="with --temporal PATH: clamp the reprojected history to the colour box of the frame's 3x3 neighbourhood before the "
                         "blend (ResidentScene.set_temporal_clamp); GAMMA (default 1) is the variance box's half-width in standard deviations")
    ap.add_argument("--temporal-clamp-mode", choices=("minmax", "variance", "both"), default=None,
                    help="with --temporal-clamp: the box is the neighbourhood's min / max, its mean +- GAMMA sigma, or (the default) the "
                         "intersection of both")
    ap.add_argument("--variance-guided", action="store_true",
                    help="with --temporal PATH: accumulate the luminance moments too and run the variance-guided filter (default parameters) "
                         "on the accumulation before it is written (ResidentScene.temporal_variance); not together with --denoise")
    ap.add_argument("--variance", metavar="PATH",
                    help="with --temporal PATH: also write every frame's variance as .pfm, numbered like --out: V^K of the variance-guided "
                         "filter with --variance-guided, the temporal variance of the luminance without")
    ap.add_argument("--progressive", type=int, default=0, metavar="N",
                    help="render N samples per pixel in N / --samples frames of the one resident scene (sample windows): --out is the finished "
                         "image, the --samples N image bit for bit; the previews after the earlier frames are numbered like --orbit's outputs "
                         "and scaled by N / done on the host.  One GPU only; not together with --orbit, --spin or the other outputs")
    ap.add_argument("--sequence", type=int, default=0, metavar="N",
                    help="with --orbit, --spin or --temporal: frame i renders samples i * S + 1 .. (i + 1) * S (mod N) of a sequence of N per "
                         "pixel (S = --samples; N a multiple of S) instead of the same S samples every frame")
    ap.add_argument("--orbit", type=int, default=1, metavar="N",
                    help="N views of the one resident scene on a circle about the vertical axis through the look-at point, same height and "
                         "distance, each after the first through ResidentScene.look_at (the camera lists are rebuilt on the device, nothing is "
                         "uploaded again); --out img.bmp becomes img_000.bmp .. img_{N-1}.bmp, and --passes, --denoise and --ao are numbered "
                         "the same way.  One GPU only.  Face normals the front-end made for a mesh WITHOUT normals were oriented toward the "
                         "first eye and are not re-oriented by a move; a scene whose normals come from the file is unaffected.  For the "
                         "built-in scenes every view, the first included, is set through --eye / --look-at / --fov (defaults: the origin and "
                         "(0, 0, 3))")
    ap.add_argument("--spin", type=int, default=1, metavar="N",
                    help="N frames of the one resident scene with the meshes turned by i * 360 / N degrees about the vertical axis through the "
                         "look-at point (vertices and corner normals turned, lights and camera fixed), each after the first through "
                         "ResidentScene.set_vertices (grid and camera lists are rebuilt on the device); outputs are numbered like --orbit's.  "
                         "For the built-in scenes the camera is set through --eye / --look-at / --fov as for --orbit (defaults: the origin "
                         "and (0, 0, 3)).  One GPU only; not together with --orbit or --bake-ao")
    ap.add_argument("--relight", type=int, default=1, metavar="N",
                    help="N frames of the one resident scene with the first light's position and direction turned by i * 360 / N degrees "
                         "about the vertical axis (raytrace.relight), each after the first through ResidentScene.set_lights (six small arrays "
                         "are uploaded, nothing is rebuilt); outputs are numbered like --orbit's.  One GPU only; not together with --orbit "
                         "or --spin")
    return ap


def parse_args(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    if args.relight < 1:
        ap.error("--relight N needs N >= 1")
    if args.relight > 1 and (args.orbit > 1 or args.spin > 1 or args.progressive or args.bake_ao):
        ap.error("--relight does not go with --orbit, --spin, --progressive or --bake-ao")
    if args.orbit < 1:
        ap.error("--orbit N needs N >= 1")
    if args.orbit > 1 and args.bake_ao:
        ap.error("--orbit does not go with --bake-ao (a bake does not read the camera)")
    if args.spin < 1:
        ap.error("--spin N needs N >= 1")
    if args.spin > 1 and (args.orbit > 1 or args.bake_ao):
        ap.error("--spin does not go with --orbit or --bake-ao")
    if args.motion and args.orbit < 2 and args.spin < 2:
        ap.error("--motion PREFIX needs --orbit N or --spin N with N >= 2 (the frames it is measured between)")
    if args.temporal and args.orbit < 2 and args.spin < 2 and args.relight < 2:
        ap.error("--temporal PATH needs --orbit N, --spin N or --relight N with N >= 2 (the frames it accumulates)")
    if args.motion_blur and args.orbit < 2 and args.spin < 2:
        ap.error("--motion-blur PATH needs --orbit N or --spin N with N >= 2 (the frames whose flow it blurs along)")
    if args.motion_blur and not args.motion_blur.lower().endswith((".bmp", ".ppm", ".pfm")):
        ap.error("--motion-blur PATH must end in .bmp, .ppm or .pfm")
    if (args.shutter is not None or args.max_blur is not None or args.blur_taps is not None) and not args.motion_blur:
        ap.error("--shutter, --max-blur and --blur-taps need --motion-blur PATH")
    if args.shutter is not None and not 0 <= args.shutter <= 4:
        ap.error("--shutter S needs S in 0..4")
    if args.max_blur is not None and not 1 <= args.max_blur <= 32:
        ap.error("--max-blur PX needs PX in 1..32")
    if args.blur_taps is not None and not 1 <= args.blur_taps <= 64:
        ap.error("--blur-taps N needs N in 1..64")
    if args.dof:
        if not args.dof.lower().endswith((".bmp", ".ppm", ".pfm")):
            ap.error("--dof PATH must end in .bmp, .ppm or .pfm")
        if args.aperture is None or not (np.isfinite(args.aperture) and args.aperture >= 0):
            ap.error("--dof PATH needs --aperture A with a finite A >= 0")
        if (args.focus is None) == (args.focus_pixel is None):
            ap.error("--dof PATH needs --focus D or --focus-pixel X Y (one of them)")
        if args.focus is not None and not (np.isfinite(args.focus) and args.focus > 0):
            ap.error("--focus D needs a finite D > 0")
        if args.focus_pixel is not None and not (0 <= args.focus_pixel[0] < args.width and 0 <= args.focus_pixel[1] < args.height):
            ap.error("--focus-pixel X Y needs a pixel of the image")
        if args.dof_rings is not None and not 1 <= args.dof_rings <= 6:
            ap.error("--dof-rings N needs N in 1..6")
        if args.max_coc is not None and not 1 <= args.max_coc <= 32:
            ap.error("--max-coc PX needs PX in 1..32")
        if args.progressive:
            ap.error("--dof does not go with --progressive")
    elif any(v is not None for v in (args.aperture, args.focus, args.focus_pixel, args.dof_rings, args.max_coc)):
        ap.error("--aperture, --focus, --focus-pixel, --dof-rings and --max-coc need --dof PATH")
    if args.temporal_clamp is not None and not args.temporal:
        ap.error("--temporal-clamp needs --temporal PATH")
    if args.temporal_clamp is not None and not (np.isfinite(args.temporal_clamp) and args.temporal_clamp >= 0):
        ap.error("--temporal-clamp GAMMA needs a finite GAMMA >= 0")
    if args.temporal_clamp_mode and args.temporal_clamp is None:
        ap.error("--temporal-clamp-mode needs --temporal-clamp")
    if args.temporal and not args.temporal.lower().endswith((".bmp", ".ppm", ".pfm")):
        ap.error("--temporal PATH must end in .bmp, .ppm or .pfm")
    if (args.variance_guided or args.variance) and not args.temporal:
        ap.error("--variance-guided and --variance PATH need --temporal PATH")
    if args.variance_guided and args.denoise:
        ap.error("--variance-guided does not go with --denoise (one filter runs on the accumulation)")
    if args.variance and not args.variance.lower().endswith(".pfm"):
        ap.error("--variance PATH must end in .pfm")
    if args.progressive:
        if args.progressive < args.samples or args.progressive % args.samples:
            ap.error("--progressive N needs N to be a multiple of --samples (the samples of one frame)")
        if args.orbit > 1 or args.spin > 1 or args.passes or args.denoise or args.ao or args.bake_ao or args.sequence:
            ap.error("--progressive does not go with --orbit, --spin, --sequence, --passes, --denoise, --ao or --bake-ao")
    if args.sequence:
        if args.orbit < 2 and args.spin < 2:
            ap.error("--sequence N needs --orbit N or --spin N with N >= 2 (the frames of the sequence)")
        if args.sequence < args.samples or args.sequence % args.samples:
            ap.error("--sequence N needs N to be a multiple of --samples (the samples of one frame)")
    if args.surface_passes and not args.passes:
        ap.error("--surface-passes needs --passes PREFIX")
    if args.denoise and not args.denoise.lower().endswith((".bmp", ".ppm", ".pfm")):
        ap.error("--denoise PATH must end in .bmp, .ppm or .pfm")
    if args.ao and not args.ao.lower().endswith((".pfm", ".pgm")):
        ap.error("--ao PATH must end in .pfm or .pgm")
    if args.bake_ao and not args.bake_ao.lower().endswith((".pfm", ".pgm")):
        ap.error("--bake-ao PATH must end in .pfm or .pgm")
    if args.mattes:
        if args.orbit > 1 or args.spin > 1 or args.relight > 1 or args.progressive:
            ap.error("--mattes PREFIX writes a single view: it does not go with --orbit, --spin, --relight or --progressive")
        if not 0 <= args.matte_layers <= 8:
            ap.error("--matte-layers K needs K in 0..8")
        if not args.matte_select and args.matte_layers == 0:
            ap.error("--mattes PREFIX needs --matte-select ids or --matte-layers K >= 1")
    elif args.matte_select or args.matte_kind != "mesh" or args.matte_layers != 4:
        ap.error("--matte-kind, --matte-select and --matte-layers need --mattes PREFIX")
    return args


def write_mattes(sc, prefix: str, device: int, kind: str, select, layers: int) -> dict:
    """ResidentScene.mattes over the frame's own samples on HIP device `device` -> PREFIX_matte_<id>.pgm per selected id and
    PREFIX_layers.npz.  Returns what mattes() returned."""
    from . import frontend, raytrace
    rs = raytrace.ResidentScene(sc, device)
    try:
        if kind == "mesh" and getattr(sc, "tri_mesh", None) is None:  # a scene not made of front-end meshes: all of it counts as mesh 0
            rs.set_matte_groups(np.zeros(sc.triangle_count, np.uint32))
            kind = "group"
        res = rs.mattes(kind=kind, select=select, layers=layers)
    finally:
        rs.close()
    for m, i in enumerate(select):
        frontend.write_pgm(f"{prefix}_matte_{i}.pgm", (res["select"][m] * np.float32(65535.0)).astype(np.uint16))
    if layers:
        np.savez(prefix + "_layers.npz", layer_id=res["layer_id"], layer_coverage=res["layer_coverage"], rest=res["rest"])
    return res


def write_ao(sc, path: str, device: int, rays: int, radius: float, samples: int, seed: int) -> np.ndarray:
    """ResidentScene.ambient_occlusion on HIP device `device` -> PATH (.pfm: f32; .pgm: u16 quantised like raytrace.quantise).  Returns
    the [H, W] f32 image."""
    from . import frontend, raytrace
    rs = raytrace.ResidentScene(sc, device)
    try:
        ao = rs.ambient_occlusion(rays=rays, radius=radius, pixel_samples=samples, seed=seed)
    finally:
        rs.close()
    if path.lower().endswith(".pfm"):
        frontend.write_pfm(path, ao)
    else:
        frontend.write_pgm(path, raytrace.quantise(ao[..., None].repeat(3, -1))[0])
    return ao


def write_bake_ao(sc, path: str, device: int, size, rays: int, radius: float, seed: int, dilate: int, triangles=None, material=None,
                  atlas: bool = False) -> dict:
    """ResidentScene.bake_ambient_occlusion on HIP device `device` -> PATH (.pfm: f32; .pgm: u16 quantised like raytrace.quantise, 8
    bits written); atlas: over scene.grid_atlas_uv instead of the scene's UVs.  Returns the bake's {"ao", "triangle"}."""
    import dataclasses

    from . import frontend, raytrace, scene
    W, H = (int(v) for v in size)
    if atlas:
        sc = dataclasses.replace(sc, tri_uv=scene.grid_atlas_uv(sc.triangle_count, max(W, H)))
    rs = raytrace.ResidentScene(sc, device)
    try:
        res = rs.bake_ambient_occlusion(W, H, rays=rays, radius=radius, seed=seed, dilate=dilate, triangles=triangles, material=material)
    finally:
        rs.close()
    if path.lower().endswith(".pfm"):
        frontend.write_pfm(path, res["ao"])
    else:
        frontend.write_pgm(path, raytrace.quantise(res["ao"][..., None].repeat(3, -1))[0])
    return res


def dof_keywords(args) -> dict:
    """--dof's options as the keywords of ResidentScene.depth_of_field."""
    kw = dict(aperture=args.aperture, focus=args.focus, focus_pixel=tuple(args.focus_pixel) if args.focus_pixel else None,
              rings=args.dof_rings, max_coc=args.max_coc)
    return {k: v for k, v in kw.items() if v is not None}


def write_dof_image(args, path: str, res: dict) -> None:
    from . import frontend
    if path.lower().endswith(".pfm"):
        frontend.write_pfm_rgb(path, res["rgb"])
    elif path.lower().endswith(".ppm"):
        frontend.write_ppm(path, *res["planes"])
    else:
        frontend.write_bmp(path, *res["planes"], low_byte_compat=args.low_byte_compat)


def write_dof(rs, args, index: int) -> None:
    """--dof under --orbit / --spin / --relight: frame `index` blurred by its depth pass -> PATH numbered like --out."""
    if args.dof:
        from . import raytrace
        write_dof_image(args, raytrace.orbit_path(args.dof, index), rs.depth_of_field(**dof_keywords(args)))


def render_passes(sc, device: int, gpus: int, surface: bool = False, basic: bool = True, denoise: bool = False, dof=None):
    """The frame through ResidentScene with the alpha, depth and triangle passes on (with `basic`) and normal and albedo (with `surface`
    or `denoise`): computation type `device` (1..gpus = one GPU, gpus + 1 = all of them, one instance per GPU over
    raytrace.tiles_of_rank).  Returns the R, G, B planes and readback_passes' dict; with `denoise` the dict also holds "denoised", what
    ResidentScene.denoise returns (default parameters) -- for several instances their read-backs composed and run through
    raytrace.denoise on device 0.  `dof`: the keywords of ResidentScene.depth_of_field; the dict then holds "dof", what it returns --
    for several instances their read-backs composed and run through raytrace.dof_lens and raytrace.depth_of_field on device 0."""
    from . import raytrace
    world = gpus if device == gpus + 1 else 1
    instances = []
    try:
        for rank in range(world):
            tiles = raytrace.tiles_of_rank(sc.width, sc.height, rank, world) if world > 1 else None
            rs = raytrace.ResidentScene(sc, rank if world > 1 else device - 1, tiles, like=instances[0] if instances else None)
            instances.append(rs)
            rs.set_passes(alpha=basic, depth=basic or dof is not None, triangle=basic, normal=surface or denoise, albedo=surface or denoise)
        for rs in instances:
            rs.render()
        planes = [np.zeros(sc.pixels, np.uint16) for _ in range(3)]
        passes = None
        for rs in instances:  # disjoint tiles: the planes add up, the passes are stored tile by tile
            rs.readback(planes)
            passes = rs.readback_passes(passes)
        if denoise and world == 1:
            passes["denoised"] = instances[0].denoise()
        if dof is not None and world == 1:
            passes["dof"] = instances[0].depth_of_field(**dof)
        camera = instances[0].camera()
    finally:
        for rs in instances:
            rs.close()
    if denoise and world > 1:
        colour = np.stack(planes, -1).reshape(sc.height, sc.width, 3).astype(np.float32) / np.float32(65535.0)
        out = raytrace.denoise(colour, passes["normal"], passes["albedo"], device=0)
        passes["denoised"] = {"colour": out, "planes": raytrace.quantise(out)}
    if dof is not None and world > 1:
        kw = dict(dof)
        aperture, focus, pixel = kw.pop("aperture"), kw.pop("focus", None), kw.pop("focus_pixel", None)
        if pixel is not None:
            focus = float(passes["depth"][pixel[1], pixel[0]])
            if not (np.isfinite(focus) and focus > 0):
                raise ValueError(f"--focus-pixel {pixel}: the ray of that pixel hit nothing")
        p = raytrace.dof_lens(camera, aperture, focus, **kw)
        colour = np.stack(planes, -1).reshape(sc.height, sc.width, 3).astype(np.float32) / np.float32(65535.0)
        out = raytrace.depth_of_field(colour, passes["depth"], focus=p.focus, coc_scale=p.cocScale, max_coc=p.maxCoc, rings=p.rings,
                                      depth_softness=p.depthSoftness, device=0)
        passes["dof"] = {"rgb": out, "planes": raytrace.quantise(out)}
    if "triangle" in passes and "mesh" not in passes:  # a scene not made of front-end meshes: all of it counts as mesh 0
        passes["mesh"] = np.where(passes["triangle"] != 0xFFFFFFFF, 0, -1).astype(np.int32)
    return [p.reshape(sc.height, sc.width) for p in planes], passes


def orbit_outputs(args, index: int) -> dict:
    """The files view `index` of an orbit writes: every given path numbered like --out (img.bmp -> img_007.bmp)."""
    from . import raytrace
    return dict(out=raytrace.orbit_path(args.out, index), passes=f"{args.passes}_{index:03d}" if args.passes else None,
                denoise=raytrace.orbit_path(args.denoise, index) if args.denoise else None,
                ao=raytrace.orbit_path(args.ao, index) if args.ao else None)


def write_view(args, paths: dict, planes, passes, denoised, ao) -> None:
    from . import frontend, raytrace
    r, g, b = planes
    if paths["passes"]:
        frontend.write_pgm(paths["passes"] + "_alpha.pgm", passes["alpha"])
        frontend.write_pfm(paths["passes"] + "_depth.pfm", passes["depth"])
        np.savez(paths["passes"] + "_ids.npz", triangle=passes["triangle"], material=passes["material"], mesh=passes["mesh"])
        if args.surface_passes:
            frontend.write_pfm_rgb(paths["passes"] + "_normal.pfm", passes["normal"])
            frontend.write_pfm_rgb(paths["passes"] + "_albedo.pfm", passes["albedo"])
    if paths["denoise"]:
        if paths["denoise"].lower().endswith(".pfm"):
            frontend.write_pfm_rgb(paths["denoise"], denoised["colour"])
        elif paths["denoise"].lower().endswith(".ppm"):
            frontend.write_ppm(paths["denoise"], *denoised["planes"])
        else:
            frontend.write_bmp(paths["denoise"], *denoised["planes"], low_byte_compat=args.low_byte_compat)
    if paths["ao"]:
        if paths["ao"].lower().endswith(".pfm"):
            frontend.write_pfm(paths["ao"], ao)
        else:
            frontend.write_pgm(paths["ao"], raytrace.quantise(ao[..., None].repeat(3, -1))[0])
    if paths["out"].lower().endswith(".ppm"):
        frontend.write_ppm(paths["out"], r, g, b)
    else:
        frontend.write_bmp(paths["out"], r, g, b, low_byte_compat=args.low_byte_compat)


def write_motion(rs, args, index: int) -> None:
    """--motion: frame `index`'s motion vectors against the marked state (frame 0: against itself) -> PREFIX_index.npz; then the scene is
    marked for the next frame (with --temporal by write_temporal, which follows: ResidentScene.temporal owns the mark)."""
    if not args.motion:
        return
    if index == 0:
        rs.mark_motion()
    np.savez(f"{args.motion}_{index:03d}.npz", **rs.motion())
    if not args.temporal:
        rs.mark_motion()


def write_motion_blur(rs, args, index: int, planes) -> None:
    """--motion-blur: frame `index` blurred along its flow to the marked state (the frame before it) -> PATH numbered like --out.  Frame
    0 has no frame before it: it is written as it is (`planes`, the read-back).  Called before write_motion and write_temporal, which
    mark the scene for the next frame; without them the mark is made here (ResidentScene.motion_blur does not mark)."""
    if not args.motion_blur:
        return
    from . import frontend, raytrace
    if index == 0:
        rs.mark_motion()
        res = dict(rgb=np.stack(planes, -1).astype(np.float32) / np.float32(65535.0), planes=planes)
    else:
        params = dict(shutter=args.shutter, max_blur=args.max_blur, taps=args.blur_taps)
        res = rs.motion_blur(**{k: v for k, v in params.items() if v is not None})
    if index and not (args.motion or args.temporal):
        rs.mark_motion()
    path = raytrace.orbit_path(args.motion_blur, index)
    if path.lower().endswith(".pfm"):
        frontend.write_pfm_rgb(path, res["rgb"])
    elif path.lower().endswith(".ppm"):
        frontend.write_ppm(path, *res["planes"])
    else:
        frontend.write_bmp(path, *res["planes"], low_byte_compat=args.low_byte_compat)


def write_temporal(rs, args, index: int) -> None:
    """--temporal: frame `index` accumulated over the frames before it -> PATH numbered like --out; with --denoise or --variance-guided,
    filtered; --variance: its variance too.  --temporal-clamp: under the scene's clamp, set before frame 0."""
    if not args.temporal:
        return
    from . import frontend, raytrace
    if index == 0 and args.temporal_clamp is not None:
        rs.set_temporal_clamp(args.temporal_clamp_mode or "both", args.temporal_clamp)
    if args.variance_guided or args.variance:
        res = rs.temporal_variance(filter={} if args.variance_guided else None)
        if args.variance:
            frontend.write_pfm(raytrace.orbit_path(args.variance, index), res["variance"])
    else:
        res = rs.temporal(denoise={} if args.denoise else None)
    path = raytrace.orbit_path(args.temporal, index)
    if path.lower().endswith(".pfm"):
        frontend.write_pfm_rgb(path, res["colour"])
    elif path.lower().endswith(".ppm"):
        frontend.write_ppm(path, *res["planes"])
    else:
        frontend.write_bmp(path, *res["planes"], low_byte_compat=args.low_byte_compat)


def render_progressive(sc, args, device: int):
    """--progressive: args.progressive samples per pixel in frames of sc.sample_count on one ResidentScene of HIP device `device`.  Writes
    a preview after every frame but the last (the planes scaled by N / done, saturating) and returns the finished R, G, B planes."""
    from . import frontend, raytrace
    rs = raytrace.ResidentScene(sc, device)
    try:
        total = args.progressive
        for done, planes in rs.progressive(total):
            planes = [p.reshape(sc.height, sc.width) for p in planes]
            if done < total:
                preview = [np.minimum(p.astype(np.uint64) * total // done, 65535).astype(np.uint16) for p in planes]
                path = raytrace.orbit_path(args.out, done // sc.sample_count - 1)
                if path.lower().endswith(".ppm"):
                    frontend.write_ppm(path, *preview)
                else:
                    frontend.write_bmp(path, *preview, low_byte_compat=args.low_byte_compat)
        return planes
    finally:
        rs.close()


def render_orbit(sc, args, device: int, eye, centre, move_first: bool) -> float:
    """--orbit: args.orbit views of one ResidentScene on HIP device `device`, the camera moved on the device between them.  Returns
    the seconds the moves, frames and read-backs took."""
    from . import raytrace
    rs = raytrace.ResidentScene(sc, device)
    try:
        basic, surface = bool(args.passes), bool(args.surface_passes or args.denoise or args.variance_guided)
        if basic or surface or args.dof:
            rs.set_passes(alpha=basic, depth=basic or bool(args.dof), triangle=basic, normal=surface, albedo=surface)
        if args.sequence:
            rs.set_sample_window(args.sequence, 0, sc.sample_count, advance=True)
        spent = 0.0
        for i, position in enumerate(raytrace.orbit_positions(eye, centre, args.orbit)):
            t = time.perf_counter()
            if i or move_first:
                rs.look_at(position, centre, (0, 1, 0), np.radians(args.fov))
            rs.render()
            planes = [p.reshape(sc.height, sc.width) for p in rs.readback()]
            spent += time.perf_counter() - t
            passes = rs.readback_passes() if basic or surface else None
            if passes is not None and "triangle" in passes and "mesh" not in passes:
                passes["mesh"] = np.where(passes["triangle"] != 0xFFFFFFFF, 0, -1).astype(np.int32)
            denoised = rs.denoise() if args.denoise else None
            ao = rs.ambient_occlusion(rays=args.ao_rays, radius=args.ao_radius, pixel_samples=args.ao_samples, seed=args.ao_seed) if args.ao else None
            write_view(args, orbit_outputs(args, i), planes, passes, denoised, ao)
            write_dof(rs, args, i)
            write_motion_blur(rs, args, i, planes)
            write_motion(rs, args, i)
            write_temporal(rs, args, i)
    finally:
        rs.close()
    return spent


def render_spin(sc, args, device: int, centre, eye=None) -> float:
    """--spin: args.spin frames of one ResidentScene on HIP device `device`, the meshes turned on the device between them.  `eye`: the
    camera is set through look_at first (the built-in scenes, as --orbit does).  Returns the seconds the updates, frames and read-backs
    took."""
    from . import raytrace
    rs = raytrace.ResidentScene(sc, device)
    try:
        if eye is not None:
            rs.look_at(eye, centre, (0, 1, 0), np.radians(args.fov))
        basic, surface = bool(args.passes), bool(args.surface_passes or args.denoise or args.variance_guided)
        if basic or surface or args.dof:
            rs.set_passes(alpha=basic, depth=basic or bool(args.dof), triangle=basic, normal=surface, albedo=surface)
        if args.sequence:
            rs.set_sample_window(args.sequence, 0, sc.sample_count, advance=True)
        vertex, index, normal = sc.vertex, sc.tri_index, sc.tri_normal
        spent = 0.0
        for i in range(args.spin):
            t = time.perf_counter()
            if i:
                rs.set_vertices(raytrace.spin_vertices(vertex, centre, i, args.spin), index if i == 1 else None,
                                raytrace.spin_directions(normal, i, args.spin))
            rs.render()
            planes = [p.reshape(sc.height, sc.width) for p in rs.readback()]
            spent += time.perf_counter() - t
            passes = rs.readback_passes() if basic or surface else None
            if passes is not None and "triangle" in passes and "mesh" not in passes:
                passes["mesh"] = np.where(passes["triangle"] != 0xFFFFFFFF, 0, -1).astype(np.int32)
            denoised = rs.denoise() if args.denoise else None
            ao = rs.ambient_occlusion(rays=args.ao_rays, radius=args.ao_radius, pixel_samples=args.ao_samples, seed=args.ao_seed) if args.ao else None
            write_view(args, orbit_outputs(args, i), planes, passes, denoised, ao)
            write_dof(rs, args, i)
            write_motion_blur(rs, args, i, planes)
            write_motion(rs, args, i)
            write_temporal(rs, args, i)
    finally:
        rs.close()
    return spent


def render_relight(sc, args, device: int) -> float:
    """--relight: args.relight frames of one ResidentScene on HIP device `device`, its first light turned through set_lights between
    them.  Returns the seconds the edits, frames and read-backs took."""
    from . import raytrace
    rs = raytrace.ResidentScene(sc, device)
    try:
        basic, surface = bool(args.passes), bool(args.surface_passes or args.denoise or args.variance_guided)
        if basic or surface or args.dof:
            rs.set_passes(alpha=basic, depth=basic or bool(args.dof), triangle=basic, normal=surface, albedo=surface)
        lights = raytrace.scene_lights(sc)
        spent = 0.0
        for i in range(args.relight):
            t = time.perf_counter()
            if i:
                rs.set_lights(raytrace.relight(lights, i, args.relight))
            rs.render()
            planes = [p.reshape(sc.height, sc.width) for p in rs.readback()]
            spent += time.perf_counter() - t
            passes = rs.readback_passes() if basic or surface else None
            if passes is not None and "triangle" in passes and "mesh" not in passes:
                passes["mesh"] = np.where(passes["triangle"] != 0xFFFFFFFF, 0, -1).astype(np.int32)
            denoised = rs.denoise() if args.denoise else None
            ao = rs.ambient_occlusion(rays=args.ao_rays, radius=args.ao_radius, pixel_samples=args.ao_samples, seed=args.ao_seed) if args.ao else None
            write_view(args, orbit_outputs(args, i), planes, passes, denoised, ao)
            write_dof(rs, args, i)
            write_temporal(rs, args, i)
    finally:
        rs.close()
    return spent


def main(argv=None):
    args = parse_args(argv)

    from . import demo, frontend, raytrace, scene
    if raytrace.lib().rtHipDeviceCount() < 1:
        sys.exit("no HIP device visible: this library has no CPU fallback")
    names = raytrace.computation_type_names()
    if not (1 <= args.device < len(names)):
        sys.exit(f"--device {args.device}: choose 1..{len(names) - 1} ({names[1:]})")
    t0 = time.perf_counter()
    if args.obj:
        try:
            mesh, materials = frontend.read_obj(args.obj)
        except OSError as e:  # (malformed or unreadable: the OBJ, one of its libraries or one of their images)
            sys.exit(f"--obj {args.obj}: {e}")
        if not len(mesh.polygons):
            sys.exit(f"--obj {args.obj}: the file holds no faces")
        lo, hi = mesh.points.min(axis=0), mesh.points.max(axis=0)
        centre, size = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) or 1.0
        look_at = np.asarray(args.look_at, np.float32) if args.look_at else centre
        eye = np.asarray(args.eye, np.float32) if args.eye else centre + np.float32([0.35, 0.25, -1.0]) * size
        sc = frontend.scene_from_meshes([mesh], materials, [dict(type=scene.LIGHT_DISTANT, dir=tuple(args.light_dir))], eye, look_at, (0, 1, 0),
                                        np.radians(args.fov), args.width, args.height, samples=args.samples, name=args.obj)
    elif args.scene == "room":
        sc = demo.room_scene(args.width, args.height, samples=args.samples)
    else:
        sc = scene.make_soup(args.width, args.height, args.triangles, 0.02, samples=args.samples)
    t1 = time.perf_counter()
    cam_ms = raytrace.build_camera_list_device(sc, 0)
    grid_ms = raytrace.build_scene_grid_device(sc, 0)
    t2 = time.perf_counter()
    if args.relight > 1:
        if args.device == raytrace.lib().rtHipDeviceCount() + 1:
            sys.exit("--relight renders on one GPU: choose --device 1..%d" % raytrace.lib().rtHipDeviceCount())
        spent = render_relight(sc, args, args.device - 1)
        print(f"{names[args.device]}: {sc.name}, {sc.triangle_count} triangles, {args.width}x{args.height}, {args.samples} samples/pixel, "
              f"{args.relight} lightings -> {raytrace.orbit_path(args.out, 0)} ..\n  edits + frames + read-backs {1e3 * spent:.0f} ms = {args.relight / spent:.1f} frames/s")
        return 0
    if args.spin > 1:
        if args.device == raytrace.lib().rtHipDeviceCount() + 1:
            sys.exit("--spin renders on one GPU: choose --device 1..%d" % raytrace.lib().rtHipDeviceCount())
        centre = look_at if args.obj else (np.asarray(args.look_at, np.float32) if args.look_at else np.float32([0, 0, 3]))
        first_eye = None if args.obj else (np.asarray(args.eye, np.float32) if args.eye else np.zeros(3, np.float32))
        spent = render_spin(sc, args, args.device - 1, centre, first_eye)
        print(f"{names[args.device]}: {sc.name}, {sc.triangle_count} triangles, {args.width}x{args.height}, {args.samples} samples/pixel, "
              f"{args.spin} poses -> {raytrace.orbit_path(args.out, 0)} ..\n  updates + frames + read-backs {1e3 * spent:.0f} ms = {args.spin / spent:.1f} frames/s")
        return 0
    if args.orbit > 1:
        if args.device == raytrace.lib().rtHipDeviceCount() + 1:
            sys.exit("--orbit renders on one GPU: choose --device 1..%d" % raytrace.lib().rtHipDeviceCount())
        if not args.obj:
            eye = np.asarray(args.eye, np.float32) if args.eye else np.zeros(3, np.float32)
            look_at = np.asarray(args.look_at, np.float32) if args.look_at else np.float32([0, 0, 3])
        spent = render_orbit(sc, args, args.device - 1, eye, look_at, move_first=not args.obj)
        print(f"{names[args.device]}: {sc.name}, {sc.triangle_count} triangles, {args.width}x{args.height}, {args.samples} samples/pixel, "
              f"{args.orbit} views -> {raytrace.orbit_path(args.out, 0)} ..\n  moves + frames + read-backs {1e3 * spent:.0f} ms = {args.orbit / spent:.1f} views/s")
        return 0
    if args.progressive:
        if args.device == raytrace.lib().rtHipDeviceCount() + 1:
            sys.exit("--progressive renders on one GPU: choose --device 1..%d" % raytrace.lib().rtHipDeviceCount())
        r, g, b = render_progressive(sc, args, args.device - 1)
        ok = True
    elif args.passes or args.denoise or args.dof:
        (r, g, b), passes = render_passes(sc, args.device, raytrace.lib().rtHipDeviceCount(), surface=args.surface_passes,
                                          basic=bool(args.passes), denoise=bool(args.denoise), dof=dof_keywords(args) if args.dof else None)
        ok = True
    else:
        ok, r, g, b = raytrace.raytrace_all(args.device, sc)
    t3 = time.perf_counter()
    if not ok:
        sys.exit("RaytraceAll failed: " + raytrace.last_error())
    if args.passes:
        frontend.write_pgm(args.passes + "_alpha.pgm", passes["alpha"])
        frontend.write_pfm(args.passes + "_depth.pfm", passes["depth"])
        np.savez(args.passes + "_ids.npz", triangle=passes["triangle"], material=passes["material"], mesh=passes["mesh"])
        if args.surface_passes:
            frontend.write_pfm_rgb(args.passes + "_normal.pfm", passes["normal"])
            frontend.write_pfm_rgb(args.passes + "_albedo.pfm", passes["albedo"])
    if args.denoise:
        den = passes["denoised"]
        if args.denoise.lower().endswith(".pfm"):
            frontend.write_pfm_rgb(args.denoise, den["colour"])
        elif args.denoise.lower().endswith(".ppm"):
            frontend.write_ppm(args.denoise, *den["planes"])
        else:
            frontend.write_bmp(args.denoise, *den["planes"], low_byte_compat=args.low_byte_compat)
    if args.dof:
        write_dof_image(args, args.dof, passes["dof"])
    if args.ao:
        gpus = raytrace.lib().rtHipDeviceCount()
        write_ao(sc, args.ao, 0 if args.device == gpus + 1 else args.device - 1, args.ao_rays, args.ao_radius, args.ao_samples, args.ao_seed)
    if args.mattes:
        gpus = raytrace.lib().rtHipDeviceCount()
        write_mattes(sc, args.mattes, 0 if args.device == gpus + 1 else args.device - 1, args.matte_kind, args.matte_select, args.matte_layers)
    if args.bake_ao:
        gpus = raytrace.lib().rtHipDeviceCount()
        write_bake_ao(sc, args.bake_ao, 0 if args.device == gpus + 1 else args.device - 1, args.bake_size, args.bake_rays, args.bake_radius,
                      args.bake_seed, args.bake_dilate, triangles=args.bake_triangles, material=args.bake_material, atlas=args.bake_atlas)
    if args.out.lower().endswith(".ppm"):
        frontend.write_ppm(args.out, r, g, b)
    else:
        frontend.write_bmp(args.out, r, g, b, low_byte_compat=args.low_byte_compat)
    rays = args.width * args.height * (args.progressive or args.samples)
    print(f"{names[args.device]}: {sc.name}, {sc.triangle_count} triangles, {args.width}x{args.height}, {args.samples} samples/pixel -> {args.out}\n"
          f"  scene {1e3 * (t1 - t0):.0f} ms, lists on the device {1e3 * (t2 - t1):.0f} ms (kernels {cam_ms:.1f} + {grid_ms:.1f} ms), "
          f"{'progressive frames + previews' if args.progressive else 'resident render + passes' if args.passes or args.denoise or args.dof else 'RaytraceAll'} {1e3 * (t3 - t2):.0f} ms = {rays / (t3 - t2) / 1e6:.0f} M primary rays/s, lit pixels {float((np.asarray(r) > 0).mean()):.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
