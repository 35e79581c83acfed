"""The first-hit feature pass against a depth-1 render of the same frame.

One MI355X, the 10 M-triangle stand-in scene bench.py builds, 1920x1080, culled traversal with MIPT_CULL_MARGIN_SAFE (bench.py's), one
sample, MIPT_SEED_PIXEL_STREAM.  HIP-event kernel time (MiptStats.kernel_ms) of
  (a) mipt_render_features_device with all eight buffers wanted (76 B of stores per pixel),
  (b) mipt_render_features_device with depth + normal + albedo (28 B per pixel),
  (c) mipt_render_device with samples = 1, max_ray_depth = 1: the same primary rays and the same traversal, 12 B per pixel.
The three kernels alternate inside every repetition; reported per cell: median, min and max of the repetitions and the spread
(max - min) / median, then the ratios (a) / (c) and (b) / (c).

    python tools/features_time.py [--tris 10000000] [--reps 7] [--json profiles/features_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cell(ms, pixels):
    ms = np.asarray(ms, dtype=np.float64)
    med = float(np.median(ms))
    return dict(kernel_ms_median=round(med, 4), kernel_ms_min=round(float(ms.min()), 4), kernel_ms_max=round(float(ms.max()), 4),
                spread=round(float((ms.max() - ms.min()) / med), 4), mpixel_s=round(pixels / med / 1e3, 1), reps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--tex-size", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "features_time.json"))
    args = ap.parse_args()

    import torch

    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("features_time.py measures on an MI355X: no HIP device visible")
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
    n = w * h
    st = L.MiptStats()
    o = rrt.make_options(w, h, 1, 1, traversal=L.TRAVERSAL_CULLED, cull_margin=L.CULL_MARGIN_SAFE)
    oc = rrt.make_options(w, h, 1, 1, traversal=L.TRAVERSAL_CULLED, cull_margin=L.CULL_MARGIN_SAFE, flags=L.FLAG_COUNT)
    table = np.ascontiguousarray(np.asarray(scene.camera.uniform, dtype=L.CAMERA).reshape(1))
    frame = torch.empty(n * 3, dtype=torch.float32, device=dev)
    planes = {name: torch.empty(n * k, dtype=torch.int32, device=dev) for name, k, _ in L.FEATURES}

    def buffers(names):
        b = L.MiptFeatureBuffers()
        for name in names:
            setattr(b, name, planes[name].data_ptr())
        return b

    every, guides = buffers(planes), buffers(("depth", "normal", "albedo"))

    def features(b, opt=o):
        L.check(lib.mipt_render_features_device(handle, L.ptr(table), 1, C.byref(opt), C.byref(b), sp, C.byref(st)), "mipt_render_features_device")
        return st.kernel_ms

    def render(opt=o):
        L.check(lib.mipt_render_device(handle, L.ptr(scene.camera.uniform), C.byref(opt), C.c_void_p(frame.data_ptr()), None, sp, C.byref(st)), "mipt_render_device")
        return st.kernel_ms

    names = ("rays", "inner_steps", "tri_tests", "hits", "texel_fetches", "max_stack")
    features(every, oc)
    f_counters = {k: int(getattr(st, k)) for k in names}
    features(guides, oc)
    g_counters = {k: int(getattr(st, k)) for k in names}
    render(oc)
    r_counters = {k: int(getattr(st, k)) for k in names}
    # the comparison is fair only if the two sides do the same traversal work, and the pass must reproduce the render it is timed against
    same_work = all(f_counters[k] == r_counters[k] for k in ("rays", "inner_steps", "tri_tests", "hits", "max_stack"))
    features(every)
    render()
    torch.cuda.synchronize()
    a, e = planes["albedo"].view(torch.float32), planes["emission"].view(torch.float32)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    same_frame = bool(torch.equal(((zero + a * e) + zero).view(torch.int32), frame.view(torch.int32)))
    for _ in range(args.warmup):
        features(every); features(guides); render()
    a_ms, b_ms, c_ms = [], [], []
    for _ in range(args.reps):                                       # the three kernels alternate inside every repetition
        a_ms.append(features(every)); b_ms.append(features(guides)); c_ms.append(render())
    out = {"scene": dict(n_tris=n_tris),
           "config": dict(frame=f"{w}x{h}", samples=1, seed_mode="pixel_stream", traversal="culled", cull_margin=L.CULL_MARGIN_SAFE, warmup=args.warmup,
                          reps=args.reps, device=torch.cuda.get_device_name(0)),
           "features_all_eight": dict(cell(a_ms, n), store_bytes_per_pixel=76, counters=f_counters),
           "features_depth_normal_albedo": dict(cell(b_ms, n), store_bytes_per_pixel=28, counters=g_counters),
           "render_depth_one": dict(cell(c_ms, n), store_bytes_per_pixel=12, counters=r_counters),
           "same_traversal_counters": bool(same_work), "albedo_times_emission_is_the_render": same_frame}
    base = out["render_depth_one"]
    for key in ("features_all_eight", "features_depth_normal_albedo"):
        out[key]["over_render_depth_one"] = round(out[key]["kernel_ms_median"] / base["kernel_ms_median"], 3)
        out[key]["slower_by_more_than_spread"] = bool(out[key]["kernel_ms_median"] > base["kernel_ms_median"] * (1.0 + max(out[key]["spread"], base["spread"])))
    for key in ("features_all_eight", "features_depth_normal_albedo", "render_depth_one"):
        print(key, json.dumps(out[key]), flush=True)
    print(f"same traversal counters: {same_work}; albedo * emission is the depth-1 render: {same_frame}")
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    scene.release()


if __name__ == "__main__":
    main()
