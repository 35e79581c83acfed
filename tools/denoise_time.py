"""The a-trous denoiser at 1080p against the least traffic one of its iterations could have.

One MI355X, the 10 M-triangle stand-in scene bench.py builds, 1920x1080, one view.  The inputs are real: the 1 spp frame of
mipt_render_batch_device and the depth, normal and albedo planes of mipt_render_features_device, all left in HBM.  Timed with HIP
events on the launch stream, around whole calls (the C ABI has no event between the passes of one call):
  (a) mipt_denoise_device with all three guides and iterations = 1 ... 5.  The call with k iterations runs the pack pass and the
      passes of step 1 ... 2^(k-1); T(k) - T(k-1) is what the pass of step 2^(k-1) adds, T(1) is the pack pass plus one pass;
  (b) a device-to-device copy of 24 B per pixel: 24 B read + 24 B written, the 48 B per pixel (32 B read + 16 B written) an iteration
      must move at least -- the centre's colour and guide records in, one colour record out;
  (c) mipt_render_features_device for depth + normal + albedo (MiptStats.kernel_ms), the pass that makes the guides.
All cells alternate inside every repetition; reported per cell: median, min and max of the repetitions and the spread
(max - min) / median; then the per-pass figures and their ratio to the copy.

    python tools/denoise_time.py [--tris 10000000] [--reps 7] [--json profiles/denoise_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERATIONS = 5


def cell(ms):
    ms = np.asarray(ms, dtype=np.float64)
    med = float(np.median(ms))
    return dict(ms_median=round(med, 4), ms_min=round(float(ms.min()), 4), ms_max=round(float(ms.max()), 4),
                spread=round(float((ms.max() - ms.min()) / med), 4), reps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--tex-size", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "denoise_time.json"))
    args = ap.parse_args()

    import torch

    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("denoise_time.py measures on an MI355X: no HIP device visible")
    lib = rrt.load()
    dev = torch.device("cuda:0")
    tris, mats, texs, cam = synth.atrium_scene(n_target=args.tris, tex_size=args.tex_size)
    scene = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    n_tris = len(tris)
    del tris
    scene.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    handle = scene.upload_from_triangles(0)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    w, h = args.width, args.height
    n = w * h
    st = L.MiptStats()
    o = rrt.make_options(w, h, 1, 8, traversal=L.TRAVERSAL_CULLED, cull_margin=L.CULL_MARGIN_SAFE)
    table = np.ascontiguousarray(np.asarray(scene.camera.uniform, dtype=L.CAMERA).reshape(1))
    hdr = torch.empty((1, h, w, 3), dtype=torch.float32, device=dev)
    out = torch.empty_like(hdr)
    planes = dict(depth=torch.empty((1, h, w), dtype=torch.float32, device=dev), normal=torch.empty((1, h, w, 3), dtype=torch.float32, device=dev),
                  albedo=torch.empty((1, h, w, 3), dtype=torch.float32, device=dev))
    L.check(lib.mipt_render_batch_device(handle, L.ptr(table), 1, C.byref(o), C.c_void_p(hdr.data_ptr()), None, sp, C.byref(st)), "mipt_render_batch_device")
    fb = L.MiptFeatureBuffers()
    for k, t in planes.items():
        setattr(fb, k, t.data_ptr())

    def features():
        L.check(lib.mipt_render_features_device(handle, L.ptr(table), 1, C.byref(o), C.byref(fb), sp, C.byref(st)), "mipt_render_features_device")
        return st.kernel_ms

    features()
    need = int(lib.mipt_denoise_workspace_bytes(w, h, 1))
    workspace = torch.empty((need // 16, 4), dtype=torch.float32, device=dev)
    db = L.MiptDenoiseBuffers()
    db.hdr, db.out = hdr.data_ptr(), out.data_ptr()
    for k, t in planes.items():
        setattr(db, k, t.data_ptr())
    do = L.MiptDenoiseOptions()
    do.width, do.height, do.n_views = w, h, 1
    do.sigma_color, do.sigma_normal, do.sigma_depth = 4.0, 0.5, 0.5

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        f()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def denoise(k):
        do.iterations = k
        L.check(lib.mipt_denoise_device(C.byref(do), C.byref(db), C.c_void_p(workspace.data_ptr()), need, sp), "mipt_denoise_device")

    copy_src = torch.empty((n * 6,), dtype=torch.float32, device=dev)       # 24 B per pixel
    copy_dst = torch.empty_like(copy_src)
    copy_src.normal_()

    def rounds(k):
        cells = {f"iterations_{i}": [] for i in range(1, ITERATIONS + 1)}
        cells.update(copy=[], features=[])
        for _ in range(k):                                                    # every cell once per repetition
            for i in range(1, ITERATIONS + 1):
                cells[f"iterations_{i}"].append(timed(lambda: denoise(i)))
            cells["copy"].append(timed(lambda: copy_dst.copy_(copy_src)))
            cells["features"].append(features())
        return cells

    rounds(args.warmup)
    cells = rounds(args.reps)
    res = {"scene": dict(n_tris=n_tris),
           "config": dict(frame=f"{w}x{h}", views=1, samples=1, max_ray_depth=8, guides=["normal", "depth", "albedo"], sigma_color=4.0, sigma_normal=0.5,
                          sigma_depth=0.5, warmup=args.warmup, reps=args.reps, device=torch.cuda.get_device_name(0),
                          timing="HIP events on the launch stream around whole calls"),
           "workspace_bytes": need}
    for i in range(1, ITERATIONS + 1):
        res[f"denoise_iterations_{i}"] = cell(cells[f"iterations_{i}"])
    res["denoise_total"] = dict(res[f"denoise_iterations_{ITERATIONS}"], mpixel_s=round(n / res[f"denoise_iterations_{ITERATIONS}"]["ms_median"] / 1e3, 1))
    res["copy_24B_per_pixel"] = dict(cell(cells["copy"]), bytes_moved=48 * n,
                                     gbyte_s=round(48 * n / float(np.median(cells["copy"])) / 1e6, 1))
    res["features_depth_normal_albedo"] = cell(cells["features"])
    med = [0.0] + [res[f"denoise_iterations_{i}"]["ms_median"] for i in range(1, ITERATIONS + 1)]
    copy = res["copy_24B_per_pixel"]["ms_median"]
    res["pack_plus_first_pass_ms"] = round(med[1], 4)
    res["added_by_pass"] = [dict(step=1 << (i - 1), ms=round(med[i] - med[i - 1], 4), over_copy=round((med[i] - med[i - 1]) / copy, 2)) for i in range(2, ITERATIONS + 1)]
    res["mean_pass_over_copy"] = round(med[ITERATIONS] / ITERATIONS / copy, 2)   # the pack pass charged to the iterations
    res["total_over_features"] = round(med[ITERATIONS] / res["features_depth_normal_albedo"]["ms_median"], 2)
    for k, v in res.items():
        if k not in ("scene", "config"):
            print(k, json.dumps(v), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    scene.release()


if __name__ == "__main__":
    main()
