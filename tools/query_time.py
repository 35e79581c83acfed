"""Ray-query rates against the trace kernel's on the bench scene.

One MI355X, the 10 M-triangle stand-in scene bench.py builds, culled traversal with MIPT_CULL_MARGIN_SAFE (bench.py's).  Mray/s from
HIP-event kernel time (MiptStats.kernel_ms) of mipt_query_closest_device and mipt_query_occluded_device on two sets of >= 16 M rays:
  (a) camera: the camera rays of a 1920x1080 frame as cpu.rs:31-45 makes them, without the jitter, the frame repeated 8 times;
  (b) incoherent: origins uniform in the scene's bounds, directions uniform on the sphere;
all with t_max = 1e30 (occlusion: "does the ray hit anything").  In the same process, as the yardstick: the trace kernel on the
bench frame (1920x1080, 8 spp, depth 64), rays from one MIPT_FLAG_COUNT launch.  The three kernels of a set alternate inside every
repetition; reported per cell: median, min and max of the repetitions and the spread (max - min) / median.

    python tools/query_time.py [--tris 10000000] [--reps 7] [--json profiles/query_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def camera_rays(torch, cam, w, h, frames, dev):
    """cpu.rs:31-45 without jitter: pixel index -> (screen x, y) -> look_at * (-x, y, 1), normalised; origin = the camera position"""
    idx = torch.arange(w * h, device=dev, dtype=torch.int64)
    x = (idx % w).to(torch.float32)
    y = (h - idx // w).to(torch.float32)
    sx = ((x / w) * 2.0 - 1.0) * (np.float32(w) / np.float32(h))
    sy = (y / h) * 2.0 - 1.0
    m = torch.tensor(np.asarray(cam["look_at"], dtype=np.float32), device=dev)            # data[col][row]
    d = (-sx)[:, None] * m[0, :3] + sy[:, None] * m[1, :3] + m[2, :3]
    d = d / d.norm(dim=1, keepdim=True)
    rays = torch.zeros((w * h, 8), dtype=torch.float32, device=dev)
    rays[:, 0:3] = torch.tensor(np.asarray(cam["position"], dtype=np.float32), device=dev)
    rays[:, 3] = 1e30
    rays[:, 4:7] = d
    return rays.repeat(frames, 1).contiguous()


def incoherent_rays(torch, lo, hi, n, dev, seed=2026):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lo, hi = torch.tensor(lo, device=dev), torch.tensor(hi, device=dev)
    rays = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    rays[:, 0:3] = lo + (hi - lo) * torch.rand((n, 3), generator=g, device=dev)
    d = torch.randn((n, 3), generator=g, device=dev)
    rays[:, 4:7] = d / d.norm(dim=1, keepdim=True)
    rays[:, 3] = 1e30
    return rays


def cell(ms, rays):
    ms = np.asarray(ms, dtype=np.float64)
    med = float(np.median(ms))
    return dict(rays=int(rays), kernel_ms_median=round(med, 3), kernel_ms_min=round(float(ms.min()), 3), kernel_ms_max=round(float(ms.max()), 3),
                spread=round(float((ms.max() - ms.min()) / med), 4), mray_s=round(rays / med / 1e3, 1), reps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--tex-size", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--rays", type=int, default=1 << 24, help="rays of the incoherent set; the camera set repeats the frame up to at least this many")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "query_time.json"))
    args = ap.parse_args()

    import torch

    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("query_time.py measures on an MI355X: no HIP device visible")
    lib = rrt.load()
    dev = torch.device("cuda:0")
    tris, mats, texs, cam = synth.atrium_scene(n_target=args.tris, tex_size=args.tex_size)
    pos = tris["vertices"]["position"].reshape(-1, 3)
    lo, hi = pos.min(axis=0).astype(np.float32), pos.max(axis=0).astype(np.float32)
    scene = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    n_tris = len(tris)
    del tris, pos
    scene.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    handle = scene.upload_from_triangles(0)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    w, h = args.width, args.height

    frames = -(-args.rays // (w * h))
    sets = {"camera": camera_rays(torch, scene.camera.uniform, w, h, frames, dev), "incoherent": incoherent_rays(torch, lo, hi, args.rays, dev)}
    qo = L.MiptQueryOptions()
    qo.traversal, qo.cull_margin = L.TRAVERSAL_CULLED, L.CULL_MARGIN_SAFE
    qc = L.MiptQueryOptions()
    qc.traversal, qc.cull_margin, qc.flags = L.TRAVERSAL_CULLED, L.CULL_MARGIN_SAFE, L.FLAG_COUNT
    st = L.MiptStats()
    o = rrt.make_options(w, h, args.spp, args.depth, traversal=L.TRAVERSAL_CULLED, cull_margin=L.CULL_MARGIN_SAFE)
    oc = rrt.make_options(w, h, args.spp, args.depth, traversal=L.TRAVERSAL_CULLED, cull_margin=L.CULL_MARGIN_SAFE, flags=L.FLAG_COUNT)
    frame = torch.empty(w * h * 3, dtype=torch.float32, device=dev)

    def trace(opt=o):
        L.check(lib.mipt_render_device(handle, L.ptr(scene.camera.uniform), C.byref(opt), C.c_void_p(frame.data_ptr()), None, sp, C.byref(st)), "mipt_render_device")
        return st.kernel_ms

    trace(oc)
    trace_rays = int(st.rays)
    out = {"scene": dict(n_tris=n_tris, bounds_min=[float(x) for x in lo], bounds_max=[float(x) for x in hi]),
           "config": dict(traversal="culled", cull_margin=L.CULL_MARGIN_SAFE, t_max=1e30, warmup=args.warmup, reps=args.reps,
                          trace_frame=f"{w}x{h}, {args.spp} spp, depth {args.depth}", device=torch.cuda.get_device_name(0)),
           "sets": {}}
    trace_ms = []
    for name, rays in sets.items():
        n = rays.shape[0]
        hits = torch.empty((n, 4), dtype=torch.int32, device=dev)
        occ = torch.empty((n,), dtype=torch.uint8, device=dev)

        def closest(opt=qo):
            L.check(lib.mipt_query_closest_device(handle, rays.data_ptr(), n, C.byref(opt), hits.data_ptr(), sp, C.byref(st)), "mipt_query_closest_device")
            return st.kernel_ms

        def occluded(opt=qo):
            L.check(lib.mipt_query_occluded_device(handle, rays.data_ptr(), n, C.byref(opt), occ.data_ptr(), sp, C.byref(st)), "mipt_query_occluded_device")
            return st.kernel_ms

        closest(qc)
        counters = {k: int(getattr(st, k)) for k in ("rays", "inner_steps", "tri_tests", "hits", "max_stack")}
        occluded(qc)
        occ_counters = {k: int(getattr(st, k)) for k in ("rays", "inner_steps", "tri_tests", "hits", "max_stack")}
        for _ in range(args.warmup):
            closest(); occluded(); trace()
        c_ms, o_ms, t_ms = [], [], []
        for _ in range(args.reps):                                   # the three kernels alternate inside every repetition
            c_ms.append(closest()); o_ms.append(occluded()); t_ms.append(trace())
        trace_ms += t_ms
        out["sets"][name] = dict(closest=dict(cell(c_ms, n), counters=counters), occluded=dict(cell(o_ms, n), counters=occ_counters),
                                 trace_alongside=cell(t_ms, trace_rays))
        print(name, json.dumps(out["sets"][name]), flush=True)
        del hits, occ
    out["trace"] = cell(trace_ms, trace_rays)
    b, t = out["sets"]["incoherent"]["closest"], out["trace"]
    spread = max(b["spread"], t["spread"])
    out["closest_incoherent_over_trace"] = round(b["mray_s"] / t["mray_s"], 3)
    out["not_below_trace_by_more_than_spread"] = bool(b["mray_s"] >= t["mray_s"] * (1.0 - spread))
    print("trace", json.dumps(out["trace"]))
    print(f"closest-hit on the incoherent set: {b['mray_s']} Mray/s = {out['closest_incoherent_over_trace']} x the trace kernel's {t['mray_s']} Mray/s "
          f"(spread {spread:.1%}): {'ok' if out['not_below_trace_by_more_than_spread'] else 'BELOW the yardstick'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    scene.release()


if __name__ == "__main__":
    main()
