"""What lightmap finishing costs and what it buys (DESIGN.md "Lightmap finishing"), one MI355X, one process.

Cost, on the 10 M-triangle stand-in scene with a 2048 x 2048 atlas (the points of mipt_bake_texels_device, a 1-sample gather as the
radiance): mipt_bake_surface_device (both outputs, unit normals; the call blocks, so the time is a host clock around it and includes
its index check), mipt_lightmap_filter_device (5 iterations, both guides) and mipt_lightmap_dilate_device (radius 8), HIP events
around each stream-ordered call.  Each stands beside a device copy of as many bytes as it must read plus write at least (surface 16 +
24 B per texel, filter 52 + 12, dilation 28 + 12), timed in the same repetitions.  The filter's mean pass is (t(5 iterations) -
t(1 iteration)) / 4 -- the pack pass and the pass to the planar output cancel -- and stands beside the same difference of
mipt_denoise_device (normal and depth guides) on one view of as many pixels, alternating in every repetition.  Per cell: median,
min, max, spread (max - min) / median.

Quality, on the charted room of tests/tools/charted_room.py at 256 x 192: the atlas baked with 4 samples raw, filtered, and filtered +
dilated, against 1024 samples: the RMSE over covered texels, and the RMSE of a bilinear lookup at 4096 surface points near chart
borders against a 1024-sample gather AT those points, with and without dilation.

    python tools/lightmap_time.py [--tris 10000000] [--reps 7] [--json profiles/lightmap_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))


def cell(ms, **more):
    ms = np.asarray(ms, dtype=np.float64)
    med = float(np.median(ms))
    return dict(ms_median=round(med, 3), ms_min=round(float(ms.min()), 3), ms_max=round(float(ms.max()), 3),
                spread=round(float((ms.max() - ms.min()) / med), 4), reps=len(ms), **more)


def rmse(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float(np.sqrt(np.mean(d * d)))


def cost(args, torch, rrt, L, lib, dev):
    from rust_ray_tracing_amd import synth
    tris, mats, texs, cam = synth.atrium_scene(n_target=args.tris, tex_size=args.tex_size)
    scene = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    n_tris = len(tris)
    del tris
    scene.upload_from_triangles(0)
    a = args.atlas
    n = a * a
    points, info = scene.bake_texels(a, a, device=True)
    radiance, _ = scene.bake_gather(points, samples=1, max_ray_depth=4, traversal=L.TRAVERSAL_CULLED)
    position, normal = scene.bake_surface(points, unit_normals=True)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out = torch.empty_like(radiance)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(run):
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    so = L.MiptBakeSurfaceOptions()
    so.flags = L.BAKE_SURFACE_UNIT_NORMALS

    def surface():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        L.check(lib.mipt_bake_surface_device(scene._handle, points.data_ptr(), n, C.byref(so), position.data_ptr(), normal.data_ptr(), sp), "mipt_bake_surface_device")
        return (time.perf_counter() - t0) * 1e3                 # the entry has synchronised

    f_ws = torch.empty(lib.mipt_lightmap_filter_workspace_bytes(a, a) // 4, dtype=torch.float32, device=dev)
    fb = L.MiptLightmapFilterBuffers()
    fb.radiance, fb.points, fb.position, fb.normal, fb.out = radiance.data_ptr(), points.data_ptr(), position.data_ptr(), normal.data_ptr(), out.data_ptr()

    def filt(iterations):
        fo = L.MiptLightmapFilterOptions()
        fo.width, fo.height, fo.iterations = a, a, iterations
        fo.sigma_color, fo.sigma_normal, fo.sigma_plane, fo.sigma_distance = 4.0, 0.5, 0.05, 0.5
        return timed(lambda: L.check(lib.mipt_lightmap_filter_device(C.byref(fo), C.byref(fb), f_ws.data_ptr(), f_ws.numel() * 4, sp), "mipt_lightmap_filter_device"))

    d_ws = torch.empty(lib.mipt_lightmap_dilate_workspace_bytes(a, a) // 4, dtype=torch.float32, device=dev)
    db = L.MiptLightmapDilateBuffers()
    db.radiance, db.points, db.out = radiance.data_ptr(), points.data_ptr(), out.data_ptr()
    do = L.MiptLightmapDilateOptions()
    do.width, do.height, do.radius = a, a, args.radius

    def dilate():
        return timed(lambda: L.check(lib.mipt_lightmap_dilate_device(C.byref(do), C.byref(db), d_ws.data_ptr(), d_ws.numel() * 4, sp), "mipt_lightmap_dilate_device"))

    # the denoiser on one view of as many pixels: the atlas's own planes as its frame, |position| as a depth
    depth = position.norm(dim=1).contiguous()
    n_ws = torch.empty(lib.mipt_denoise_workspace_bytes(a, a, 1) // 4, dtype=torch.float32, device=dev)
    nb = L.MiptDenoiseBuffers()
    nb.hdr, nb.normal, nb.depth, nb.out = radiance.data_ptr(), normal.data_ptr(), depth.data_ptr(), out.data_ptr()

    def denoise(iterations):
        no = L.MiptDenoiseOptions()
        no.width, no.height, no.n_views, no.iterations = a, a, 1, iterations
        no.sigma_color, no.sigma_normal, no.sigma_depth = 4.0, 0.5, 0.5
        return timed(lambda: L.check(lib.mipt_denoise_device(C.byref(no), C.byref(nb), n_ws.data_ptr(), n_ws.numel() * 4, sp), "mipt_denoise_device"))

    copies = {}
    for name, per_texel in (("surface", 40), ("filter", 64), ("dilate", 40)):
        src, dst = torch.empty(per_texel * n, dtype=torch.uint8, device=dev), torch.empty(per_texel * n, dtype=torch.uint8, device=dev)
        copies[name] = (lambda s=src, d=dst: timed(lambda: d.copy_(s)), per_texel * n)

    runs = [("surface", surface), ("surface_copy", copies["surface"][0]), ("filter_5", lambda: filt(5)), ("filter_copy", copies["filter"][0]),
            ("filter_1", lambda: filt(1)), ("denoise_5", lambda: denoise(5)), ("denoise_1", lambda: denoise(1)),
            ("dilate", dilate), ("dilate_copy", copies["dilate"][0])]
    for _ in range(args.warmup):
        for _, run in runs:
            run()
    ms = {name: [] for name, _ in runs}
    for _ in range(args.reps):                                   # everything alternates inside every repetition
        for name, run in runs:
            ms[name].append(run())
    res = {"scene": dict(n_tris=n_tris), "atlas": dict(size=f"{a}x{a}", texels=n, covered_texels=int(info["covered_texels"]))}
    for name, _ in runs:
        res[name] = cell(ms[name], **({"bytes": copies[name[:-5]][1]} if name.endswith("_copy") else {}))
    for name in ("surface", "dilate"):
        res[f"{name}_over_copy"] = round(res[name]["ms_median"] / res[f"{name}_copy"]["ms_median"], 2)
    res["filter_over_copy"] = round(res["filter_5"]["ms_median"] / res["filter_copy"]["ms_median"], 2)
    f_pass = (np.asarray(ms["filter_5"]) - np.asarray(ms["filter_1"])) / 4.0
    n_pass = (np.asarray(ms["denoise_5"]) - np.asarray(ms["denoise_1"])) / 4.0
    res["filter_mean_pass"], res["denoise_mean_pass"] = cell(f_pass), cell(n_pass)
    res["filter_pass_over_denoise_pass"] = round(res["filter_mean_pass"]["ms_median"] / res["denoise_mean_pass"]["ms_median"], 3)
    res["filter_pass_over_copy"] = round(res["filter_mean_pass"]["ms_median"] / res["filter_copy"]["ms_median"], 2)
    res["dilate"]["radius"] = args.radius
    scene.release()
    return res


def quality(args, torch, rrt, L):
    import charted_room as room
    tris, mats = room.build(rrt)
    scene = rrt.Scene.from_arrays(tris, mats, (), build_bvh=False)
    scene.upload_from_triangles(0)
    w, h = args.room_width, args.room_height
    kw = dict(device=False, max_ray_depth=args.depth)
    fopt = dict(iterations=args.room_iterations, sigma_color=args.sigma_color, sigma_normal=0.5, sigma_plane=0.05, sigma_distance=args.sigma_distance)
    ref, covered, _ = scene.bake_lightmap(w, h, args.ref_samples, **kw)
    raw, _, _ = scene.bake_lightmap(w, h, args.samples, **kw)
    filtered, _, _ = scene.bake_lightmap(w, h, args.samples, filter=fopt, **kw)
    finished, _, _ = scene.bake_lightmap(w, h, args.samples, filter=fopt, dilate=args.room_dilate, **kw)
    raw_dilated, _, _ = scene.bake_lightmap(w, h, args.samples, dilate=args.room_dilate, **kw)
    ref_dilated = rrt.lightmap_dilate(ref, scene.bake_texels(w, h)[0], radius=args.room_dilate)
    pts, uv = room.border_points(args.border_points, seed=5)
    at_points, _ = scene.bake_gather(pts, samples=args.ref_samples, max_ray_depth=args.depth)
    res = {"room": dict(atlas=f"{w}x{h}", covered_texels=int(covered.sum()), samples=args.samples, reference_samples=args.ref_samples,
                        max_ray_depth=args.depth, filter=fopt, dilate=args.room_dilate, border_points=args.border_points),
           "rmse_covered": {k: round(rmse(v[covered], ref[covered]), 5) for k, v in (("raw", raw), ("filtered", filtered), ("filtered_dilated", finished))},
           "rmse_bilinear_near_borders": {k: round(rmse(room.bilinear(v, uv), at_points), 5)
                                          for k, v in (("raw", raw), ("raw_dilated", raw_dilated), ("filtered", filtered), ("filtered_dilated", finished),
                                                       ("reference", ref), ("reference_dilated", ref_dilated))},
           "mean_reference_radiance": round(float(ref[covered].mean()), 5)}
    scene.release()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--tex-size", type=int, default=1024)
    ap.add_argument("--atlas", type=int, default=2048)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--room-width", type=int, default=256)
    ap.add_argument("--room-height", type=int, default=192)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--ref-samples", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--room-iterations", type=int, default=4)
    ap.add_argument("--room-dilate", type=int, default=4)
    ap.add_argument("--sigma-color", type=float, default=1.0)
    ap.add_argument("--sigma-distance", type=float, default=0.25)
    ap.add_argument("--border-points", type=int, default=4096)
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "lightmap_time.json"))
    args = ap.parse_args()

    import torch

    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L

    if not torch.cuda.is_available():
        raise SystemExit("lightmap_time.py measures on an MI355X: no HIP device visible")
    lib = rrt.load()
    dev = torch.device("cuda:0")
    out = {"config": dict(warmup=args.warmup, reps=args.reps, device=torch.cuda.get_device_name(0),
                          compute_units=torch.cuda.get_device_properties(0).multi_processor_count)}
    out["quality"] = quality(args, torch, rrt, L)
    if not args.skip_cost:
        out["cost"] = cost(args, torch, rrt, L, lib, dev)
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
