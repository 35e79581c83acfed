"""Radiance-query rate on a bake-shaped workload, beside the frame's (DESIGN.md "Radiance queries").

One MI355X, the 10 M-triangle stand-in scene bench.py builds, culled traversal with MIPT_CULL_MARGIN_SAFE (bench.py's).  The rays:
the `position` and `normal` planes of mipt_render_features_device at 1920x1080 as origins and directions, every origin moved
1e-4 x its direction off the surface -- one ray per visible surface point, leaving along the normal, as a lightmap or vertex baker
sends them (2.07 M rays; a pixel that saw nothing gives a ray with a zero direction, which misses).  Timed: the HIP-event kernel time
(MiptStats.kernel_ms) of mipt_query_radiance_device at 8 samples, depth 8, and beside it mipt_render_device of the same scene at the
same size, samples and depth, the two alternating inside every repetition of one process.  Rays (traverse_bvh invocations) come from
one MIPT_FLAG_COUNT launch of each, outside the timed ones; its wave diagnostics give the lanes per traversal step.  Reported per
cell: median, min and max of the repetitions and the spread (max - min) / median.

    python tools/radiance_time.py [--tris 10000000] [--reps 7] [--json profiles/radiance_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cell(ms, rays):
    ms = np.asarray(ms, dtype=np.float64)
    med = float(np.median(ms))
    return dict(rays=int(rays), kernel_ms_median=round(med, 3), kernel_ms_min=round(float(ms.min()), 3), kernel_ms_max=round(float(ms.max()), 3),
                spread=round(float((ms.max() - ms.min()) / med), 4), mray_s=round(rays / med / 1e3, 1), reps=len(ms))


def lanes(st):
    """from the counting launch's wave diagnostics (MiptStats.diag): lanes at work per traversal iteration of a wave, out of 64"""
    d = [int(x) for x in st.diag]
    return dict(iterations=d[0], lanes_per_iteration=round((d[1] + d[2]) / max(d[0], 1), 2), inner_lanes_per_inner_iteration=round(d[1] / max(d[3], 1), 2),
                leaf_lanes_per_leaf_iteration=round(d[2] / max(d[4], 1), 2), lanes_per_service_pass=round(d[6] / max(d[5], 1), 2),
                service_cycle_share=round(d[7] / max(d[8], 1), 4), tail_cycle_share=round(d[10] / max(d[8], 1), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--tex-size", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "radiance_time.json"))
    args = ap.parse_args()

    import torch

    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("radiance_time.py measures on an MI355X: no HIP device visible")
    lib = rrt.load()
    dev = torch.device("cuda:0")
    tris, mats, texs, cam = synth.atrium_scene(n_target=args.tris, tex_size=args.tex_size)
    scene = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    n_tris = len(tris)
    del tris
    scene.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    handle = scene.upload_from_triangles(0)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    w, h = args.width, args.height

    # the bake rays: one per pixel's first hit, along its shading normal
    first = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=args.depth, output_image_dimensions=(w, h), output_image_path="/dev/null",
                                                 traversal=L.TRAVERSAL_CULLED, cull_margin=L.CULL_MARGIN_SAFE))
    planes, _ = first.render_features(scene, features=("position", "normal"), device=True)
    p, nrm = planes["position"].reshape(-1, 3), planes["normal"].reshape(-1, 3)
    n = p.shape[0]
    rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    rays[:, 0:3] = p + nrm * 1e-4
    rays[:, 4:7] = nrm
    rays[:, 7] = torch.from_numpy(rrt.Scene.radiance_default_seeds(n).view(np.int32)).to(dev).view(torch.float32)
    no_surface = int((nrm == 0).all(dim=1).sum().item())
    del planes, p, nrm
    radiance = torch.empty((n, 3), dtype=torch.float32, device=dev)
    frame = torch.empty(w * h * 3, dtype=torch.float32, device=dev)

    def options(flags):
        ro = L.MiptRadianceOptions()
        ro.samples, ro.max_ray_depth, ro.traversal, ro.cull_margin, ro.flags = args.spp, args.depth, L.TRAVERSAL_CULLED, L.CULL_MARGIN_SAFE, flags
        return ro, rrt.make_options(w, h, args.spp, args.depth, traversal=L.TRAVERSAL_CULLED, cull_margin=L.CULL_MARGIN_SAFE, flags=flags)

    st = L.MiptStats()

    def query(ro):
        L.check(lib.mipt_query_radiance_device(handle, rays.data_ptr(), n, C.byref(ro), radiance.data_ptr(), sp, C.byref(st)), "mipt_query_radiance_device")
        return st.kernel_ms

    def render(o):
        L.check(lib.mipt_render_device(handle, L.ptr(scene.camera.uniform), C.byref(o), C.c_void_p(frame.data_ptr()), None, sp, C.byref(st)), "mipt_render_device")
        return st.kernel_ms

    ro_c, o_c = options(L.FLAG_COUNT)
    ro, o = options(0)
    counted = {}
    for name, run, opt in (("query", query, ro_c), ("frame", render, o_c)):          # the counting launches, outside the timed ones
        run(opt)
        counted[name] = dict({k: int(getattr(st, k)) for k in ("rays", "inner_steps", "tri_tests", "hits", "texel_fetches", "max_stack")}, **lanes(st))
    for _ in range(args.warmup):
        query(ro); render(o)
    q_ms, f_ms = [], []
    for _ in range(args.reps):                                                         # the two kernels alternate inside every repetition
        q_ms.append(query(ro)); f_ms.append(render(o))
    out = {"scene": dict(n_tris=n_tris),
           "config": dict(traversal="culled", cull_margin=L.CULL_MARGIN_SAFE, size=f"{w}x{h}", samples=args.spp, max_ray_depth=args.depth, origin_offset=1e-4,
                          warmup=args.warmup, reps=args.reps, device=torch.cuda.get_device_name(0), compute_units=torch.cuda.get_device_properties(0).multi_processor_count),
           "query": dict(cell(q_ms, counted["query"]["rays"]), n_rays=n, rays_without_a_surface=no_surface, counting_launch=counted["query"]),
           "frame": dict(cell(f_ms, counted["frame"]["rays"]), counting_launch=counted["frame"])}
    out["query_over_frame_mray_s"] = round(out["query"]["mray_s"] / out["frame"]["mray_s"], 3)
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    scene.release()


if __name__ == "__main__":
    main()
