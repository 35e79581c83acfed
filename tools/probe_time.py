"""What irradiance probes cost on the 10 M-triangle stand-in scene (DESIGN.md "Irradiance probes"), one MI355X, one process.

(a) mipt_probe_bake_device on a 32 x 32 x 16 grid over the scene's bounds, 256 samples a probe, depth 8, culled with
    MIPT_CULL_MARGIN_SAFE -- 2^22 paths, one chunk -- beside mipt_query_radiance_device on pre-generated rays of the same number of
    paths: the same origins, directions drawn uniformly on the sphere by torch (the same distribution, not the same draws),
    samples = 1.  The two alternate inside every repetition.  Times: MiptStats.kernel_ms -- for the bake the span from its first
    kernel to its last, the ray generation and the projection included.  The split of the surplus between those two comes from a
    kernel trace taken in a run of its own:
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/probe_time.py --bake-only
    and is merged into the JSON afterwards with --merge-trace DIR/.../..._kernel_stats.csv.
(b) mipt_probe_irradiance_device for the first-hit points of the 1920 x 1080 view (position and normal planes of
    mipt_render_features_device) against the grid (a) baked, timed with HIP events beside a device copy of the bytes it must move:
    36 B a point (position, normal, irradiance) plus 108 B a probe.
Reported per cell: median, min, max, spread (max - min) / median.

    python tools/probe_time.py [--tris 10000000] [--reps 7] [--json profiles/probe_time.json]
"""
import argparse
import csv
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


def merge_trace(json_path, csv_path):
    """the per-kernel totals of a `rocprofv3 --kernel-trace --stats` run of --bake-only, beside the measured numbers"""
    rows = {}
    with open(csv_path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            short = "probe_rays_kernel" if "probe_rays_kernel" in name else "probe_project_kernel" if "probe_project_kernel" in name else \
                    "trace" if "pt_trace" in name else None
            if short is None:
                continue
            calls, total = int(r["Calls"]), float(r["TotalDurationNs"])
            c = rows.setdefault(short, dict(calls=0, total_ms=0.0, kernels=[]))
            c["calls"] += calls
            c["total_ms"] += total / 1e6
            c["kernels"].append(name[:96])
    for c in rows.values():
        c["ms_per_call"] = round(c["total_ms"] / max(c["calls"], 1), 3)
        c["total_ms"] = round(c["total_ms"], 3)
    with open(json_path) as f:
        out = json.load(f)
    out["bake_kernel_trace"] = rows
    with open(json_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(rows, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--tex-size", type=int, default=1024)
    ap.add_argument("--grid", type=int, nargs=3, default=(32, 32, 16))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bake-only", action="store_true", help="part (a)'s bake alone, three calls, nothing written: the run a kernel trace is taken of")
    ap.add_argument("--merge-trace", default=None, help="a kernel_stats.csv of such a run: its per-kernel totals are added to the JSON, nothing is run")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "probe_time.json"))
    args = ap.parse_args()
    if args.merge_trace:
        merge_trace(args.json, args.merge_trace)
        return

    import torch

    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("probe_time.py measures on an MI355X: no HIP device visible")
    lib = rrt.load()
    dev = torch.device("cuda:0")
    tris, mats, texs, cam = synth.atrium_scene(n_target=args.tris, tex_size=args.tex_size)
    P = tris["vertices"]["position"].reshape(-1, 3)
    lo, hi = P.min(0).astype(np.float64), P.max(0).astype(np.float64)
    scene = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    n_tris = len(tris)
    del tris, P
    scene.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    handle = scene.upload_from_triangles(0)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    # ---- (a) bake ----
    dims = tuple(int(d) for d in args.grid)
    spacing = tuple(float(np.float32((hi[a] - lo[a]) / max(dims[a] - 1, 1))) for a in range(3))
    grid = (tuple(float(np.float32(x)) for x in lo), spacing, dims)
    pos = rrt.probe_grid(*grid)
    n_probes = len(pos)
    paths = n_probes * args.spp
    probes = np.zeros(n_probes, dtype=L.PROBE)
    probes["position"], probes["seed"] = pos, np.arange(n_probes, dtype=np.uint32)
    d_probes = torch.from_numpy(probes.view(np.int32).reshape(-1, 4).copy()).to(dev)
    d_sh = torch.empty((n_probes, 9, 3), dtype=torch.float32, device=dev)
    st = L.MiptStats()

    def bake(flags=0):
        bo = L.MiptProbeBakeOptions()
        bo.samples, bo.max_ray_depth, bo.traversal, bo.cull_margin, bo.flags, bo.sample_stride = args.spp, args.depth, L.TRAVERSAL_CULLED, L.CULL_MARGIN_SAFE, flags, n_probes
        L.check(lib.mipt_probe_bake_device(handle, d_probes.data_ptr(), n_probes, C.byref(bo), d_sh.data_ptr(), sp, C.byref(st)), "mipt_probe_bake_device")
        return st.kernel_ms

    if args.bake_only:
        for _ in range(3):
            bake()
        print(json.dumps(dict(probes=n_probes, paths=paths, kernel_ms=round(st.kernel_ms, 3))))
        scene.release()
        return
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    rnd = torch.randn((n_probes, args.spp, 3), generator=g, device=dev)
    pre = torch.zeros((n_probes, args.spp, 8), dtype=torch.float32, device=dev)
    pre[:, :, 0:3] = torch.from_numpy(pos).to(dev)[:, None, :]
    pre[:, :, 4:7] = rnd / rnd.norm(dim=2, keepdim=True)
    pre[:, :, 7] = torch.from_numpy(rrt.Scene.radiance_default_seeds(paths).view(np.int32)).to(dev).view(torch.float32).reshape(n_probes, args.spp)
    pre = pre.reshape(-1, 8).contiguous()
    pre_out = torch.empty((paths, 3), dtype=torch.float32, device=dev)
    del rnd

    def query(flags=0):
        ro = L.MiptRadianceOptions()
        ro.samples, ro.max_ray_depth, ro.traversal, ro.cull_margin, ro.flags = 1, args.depth, L.TRAVERSAL_CULLED, L.CULL_MARGIN_SAFE, flags
        L.check(lib.mipt_query_radiance_device(handle, pre.data_ptr(), paths, C.byref(ro), pre_out.data_ptr(), sp, C.byref(st)), "mipt_query_radiance_device")
        return st.kernel_ms

    runs = (("bake", bake), ("pregenerated_rays", query))
    counted = {}
    for name, run in runs:                                                                 # the counting launches, outside the timed ones
        run(L.FLAG_COUNT)
        counted[name] = {k: int(getattr(st, k)) for k in ("rays", "inner_steps", "tri_tests", "hits", "pixels")}
    for _ in range(args.warmup):
        for _, run in runs:
            run()
    ms = {name: [] for name, _ in runs}
    for _ in range(args.reps):                                                             # the two alternate inside every repetition
        for name, run in runs:
            ms[name].append(run())
    out = {"scene": dict(n_tris=n_tris, bounds=[lo.tolist(), hi.tolist()]),
           "config": dict(grid="x".join(map(str, dims)), probes=n_probes, samples=args.spp, paths=paths, traversal="culled", cull_margin=L.CULL_MARGIN_SAFE,
                          max_ray_depth=args.depth, view=f"{args.width}x{args.height}", warmup=args.warmup, reps=args.reps,
                          device=torch.cuda.get_device_name(0), compute_units=torch.cuda.get_device_properties(0).multi_processor_count)}
    for name, _ in runs:
        out[name] = dict(cell(ms[name]), mray_s=round(counted[name]["rays"] / float(np.median(ms[name])) / 1e3, 1), counting_launch=counted[name])
    out["bake_over_pregenerated_rays"] = round(out["bake"]["ms_median"] / out["pregenerated_rays"]["ms_median"], 3)
    sh_finite = bool(torch.isfinite(d_sh).all().item())
    out["bake"].update(all_coefficients_finite=sh_finite)
    del pre, pre_out

    # ---- (b) lookup ----
    w, h = args.width, args.height
    first = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=args.depth, output_image_dimensions=(w, h), output_image_path="/dev/null",
                                                 traversal=L.TRAVERSAL_CULLED, cull_margin=L.CULL_MARGIN_SAFE))
    planes, _ = first.render_features(scene, features=("position", "normal"), device=True)
    p, nrm = planes["position"].reshape(-1, 3).contiguous(), planes["normal"].reshape(-1, 3).contiguous()
    n = p.shape[0]
    e_out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    gr = L.MiptProbeGrid()
    gr.origin[:], gr.spacing[:], gr.dims[:], gr.flags = grid[0], grid[1], grid[2], L.PROBE_CLAMP
    bufs = L.MiptProbeIrradianceBuffers()
    bufs.sh, bufs.position, bufs.normal, bufs.irradiance = d_sh.data_ptr(), p.data_ptr(), nrm.data_ptr(), e_out.data_ptr()
    copy_bytes = 36 * n + 108 * n_probes
    src, dst = torch.empty(copy_bytes, dtype=torch.uint8, device=dev), torch.empty(copy_bytes, dtype=torch.uint8, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(f):
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def lookup():
        L.check(lib.mipt_probe_irradiance_device(C.byref(gr), n, C.byref(bufs), sp), "mipt_probe_irradiance_device")

    for _ in range(args.warmup):
        timed(lookup); timed(lambda: dst.copy_(src))
    l_ms, c_ms = [], []
    for _ in range(args.reps):
        l_ms.append(timed(lookup)); c_ms.append(timed(lambda: dst.copy_(src)))
    out["irradiance"] = cell(l_ms, points=n, gb_s=round(copy_bytes / float(np.median(l_ms)) / 1e6, 1))
    out["irradiance_copy_floor"] = cell(c_ms, bytes=copy_bytes)
    out["irradiance_over_copy"] = round(out["irradiance"]["ms_median"] / out["irradiance_copy_floor"]["ms_median"], 2)
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    scene.release()


if __name__ == "__main__":
    main()
