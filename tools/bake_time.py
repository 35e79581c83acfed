"""What baking costs on the 10 M-triangle stand-in scene (DESIGN.md "Baking"), one MI355X, one process.

(a) mipt_bake_texels_device at 2048 x 2048: the HIP-event time of the memsets and kernels (MiptBakeTexelInfo.kernel_ms) and the covered
    count, beside a device copy of the bytes the pass must read (64 B x triangles) plus the bytes it must write (16 B x texels), timed
    with HIP events in the same repetitions.  The split between the coverage and the resolve pass comes from a kernel trace taken in
    a run of its own:  rocprofv3 --kernel-trace --stats -- python tools/bake_time.py --texels-only
(b) mipt_bake_gather_device on the first hits of the 1920 x 1080 view tools/radiance_time.py uses (one point per pixel that sees a
    surface, from mipt_query_closest_device along the camera's rays), 8 samples, depth 8, culled with MIPT_CULL_MARGIN_SAFE -- beside
    mipt_query_radiance_device on pre-generated rays of the same number of paths (points x 8 rays leaving along
    normalized(N + a random unit vector), samples = 1) and beside the 8-samples-per-ray call of DESIGN section 23 (one ray per point
    along its normal).  The three alternate inside every repetition.  Times: MiptStats.kernel_ms -- for the gather the span from its
    first kernel to its last, chunks and staging kernels included.  Reported per cell: median, min, max, spread (max - min) / median.

    python tools/bake_time.py [--tris 10000000] [--reps 7] [--json profiles/bake_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cell(ms, **more):
    ms = np.asarray(ms, dtype=np.float64)
    med = float(np.median(ms))
    return dict(ms_median=round(med, 3), ms_min=round(float(ms.min()), 3), ms_max=round(float(ms.max()), 3),
                spread=round(float((ms.max() - ms.min()) / med), 4), reps=len(ms), **more)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--tex-size", type=int, default=1024)
    ap.add_argument("--atlas", type=int, default=2048)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--texels-only", action="store_true", help="part (a) alone, three calls, nothing written: the run a kernel trace is taken of")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "bake_time.json"))
    args = ap.parse_args()

    import torch

    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("bake_time.py measures on an MI355X: no HIP device visible")
    lib = rrt.load()
    dev = torch.device("cuda:0")
    tris, mats, texs, cam = synth.atrium_scene(n_target=args.tris, tex_size=args.tex_size)
    scene = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    n_tris = len(tris)
    del tris
    scene.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    handle = scene.upload_from_triangles(0)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    # ---- (a) texels ----
    a = args.atlas
    d_points = torch.empty((a * a, 4), dtype=torch.int32, device=dev)
    info = L.MiptBakeTexelInfo()

    def texels():
        L.check(lib.mipt_bake_texels_device(handle, a, a, None, d_points.data_ptr(), sp, C.byref(info)), "mipt_bake_texels_device")
        return info.kernel_ms

    if args.texels_only:
        for _ in range(3):
            texels()
        print(json.dumps(dict(covered_texels=int(info.covered_texels), degenerate_tris=int(info.degenerate_tris), kernel_ms=round(info.kernel_ms, 3))))
        scene.release()
        return
    copy_bytes = 64 * n_tris + 16 * a * a
    src, dst = torch.empty(copy_bytes, dtype=torch.uint8, device=dev), torch.empty(copy_bytes, dtype=torch.uint8, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def copy():
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        texels(); copy()
    t_ms, c_ms = [], []
    for _ in range(args.reps):
        t_ms.append(texels()); c_ms.append(copy())
    out = {"scene": dict(n_tris=n_tris),
           "config": dict(atlas=f"{a}x{a}", traversal="culled", cull_margin=L.CULL_MARGIN_SAFE, view=f"{args.width}x{args.height}", samples=args.spp,
                          max_ray_depth=args.depth, warmup=args.warmup, reps=args.reps, device=torch.cuda.get_device_name(0),
                          compute_units=torch.cuda.get_device_properties(0).multi_processor_count),
           "texels": dict(cell(t_ms), covered_texels=int(info.covered_texels), degenerate_tris=int(info.degenerate_tris)),
           "texels_copy_floor": cell(c_ms, bytes=copy_bytes)}
    out["texels_over_copy"] = round(out["texels"]["ms_median"] / out["texels_copy_floor"]["ms_median"], 2)
    del src, dst

    # ---- (b) gather ----
    w, h = args.width, args.height
    first = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=args.depth, output_image_dimensions=(w, h), output_image_path="/dev/null",
                                                 traversal=L.TRAVERSAL_CULLED, cull_margin=L.CULL_MARGIN_SAFE))
    planes, _ = first.render_features(scene, features=("position", "normal"), device=True)
    p, nrm = planes["position"].reshape(-1, 3), planes["normal"].reshape(-1, 3)
    n = p.shape[0]
    eye = torch.tensor(np.asarray(cam[0], dtype=np.float32), device=dev)
    seen = ~(nrm == 0).all(dim=1)
    prim_rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    prim_rays[:, 0:3] = eye
    prim_rays[:, 3] = 1e30
    prim_rays[:, 4:7] = torch.where(seen[:, None], p - eye, torch.zeros_like(p))          # a pixel that saw nothing: a zero direction, which misses
    hits, _ = scene._query(False, prim_rays, None, L.TRAVERSAL_CULLED, L.CULL_MARGIN_SAFE, False, None, None)
    points = hits.clone()
    points[:, 0] = torch.arange(n, dtype=torch.int32, device=dev)                          # the seed word
    n_points = int((points[:, 3] != -1).sum().item())
    radiance = torch.empty((n, 3), dtype=torch.float32, device=dev)
    # the same number of paths as pre-generated rays: along normalized(N + a random unit vector), 1e-4 off the surface
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rnd = torch.randn((n, args.spp, 3), generator=g, device=dev)
    d = nrm[:, None, :] + rnd / rnd.norm(dim=2, keepdim=True)
    d = torch.where(seen[:, None, None], d / d.norm(dim=2, keepdim=True).clamp_min(1e-20), torch.zeros_like(d))
    pre = torch.zeros((n, args.spp, 8), dtype=torch.float32, device=dev)
    pre[:, :, 0:3] = p[:, None, :] + d * 1e-4
    pre[:, :, 4:7] = d
    pre[:, :, 7] = torch.from_numpy(rrt.Scene.radiance_default_seeds(n * args.spp).view(np.int32)).to(dev).view(torch.float32).reshape(n, args.spp)
    pre = pre.reshape(-1, 8).contiguous()
    pre_out = torch.empty((n * args.spp, 3), dtype=torch.float32, device=dev)
    along = torch.zeros((n, 8), dtype=torch.float32, device=dev)                           # DESIGN section 23's rays
    along[:, 0:3] = p + nrm * 1e-4
    along[:, 4:7] = nrm
    along[:, 7] = torch.from_numpy(rrt.Scene.radiance_default_seeds(n).view(np.int32)).to(dev).view(torch.float32)
    del planes, p, nrm, rnd, d, hits, prim_rays
    st = L.MiptStats()

    def bake(flags=0):
        bo = L.MiptBakeOptions()
        bo.samples, bo.max_ray_depth, bo.traversal, bo.cull_margin, bo.flags, bo.sample_stride = args.spp, args.depth, L.TRAVERSAL_CULLED, L.CULL_MARGIN_SAFE, flags, n
        L.check(lib.mipt_bake_gather_device(handle, points.data_ptr(), n, C.byref(bo), radiance.data_ptr(), sp, C.byref(st)), "mipt_bake_gather_device")
        return st.kernel_ms

    def query(rays, out_t, samples, flags=0):
        ro = L.MiptRadianceOptions()
        ro.samples, ro.max_ray_depth, ro.traversal, ro.cull_margin, ro.flags = samples, args.depth, L.TRAVERSAL_CULLED, L.CULL_MARGIN_SAFE, flags
        L.check(lib.mipt_query_radiance_device(handle, rays.data_ptr(), rays.shape[0], C.byref(ro), out_t.data_ptr(), sp, C.byref(st)), "mipt_query_radiance_device")
        return st.kernel_ms

    runs = (("gather", lambda f=0: bake(f)), ("pregenerated_rays", lambda f=0: query(pre, pre_out, 1, f)), ("rays_along_normal_8_samples", lambda f=0: query(along, radiance, args.spp, f)))
    counted = {}
    for name, run in runs:                                                                 # the counting launches, outside the timed ones
        run(L.FLAG_COUNT)
        counted[name] = {k: int(getattr(st, k)) for k in ("rays", "inner_steps", "tri_tests", "hits", "pixels")}
    for _ in range(args.warmup):
        for _, run in runs:
            run()
    ms = {name: [] for name, _ in runs}
    for _ in range(args.reps):                                                             # the three alternate inside every repetition
        for name, run in runs:
            ms[name].append(run())
    for name, _ in runs:
        out[name] = dict(cell(ms[name]), mray_s=round(counted[name]["rays"] / float(np.median(ms[name])) / 1e3, 1), counting_launch=counted[name])
    out["gather"].update(n_points=n_points, n_records=n, paths=n * args.spp)
    out["gather_over_pregenerated_rays"] = round(out["gather"]["ms_median"] / out["pregenerated_rays"]["ms_median"], 3)
    out["gather_over_rays_along_normal"] = round(out["gather"]["ms_median"] / out["rays_along_normal_8_samples"]["ms_median"], 3)
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    scene.release()


if __name__ == "__main__":
    main()
