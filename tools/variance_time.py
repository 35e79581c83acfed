"""The variance-guided a-trous filter at 1080p against the fixed-bandwidth one and a copy.

One MI355X, the 10 M-triangle stand-in scene bench.py builds, 1920x1080, one view.  The inputs are real: a few 1 spp frames of
mipt_render_batch_device along a slowly moving camera, the planes of mipt_render_features_device and the accumulated frame, variance
and history length of mipt_temporal_device for the last of them, all left in HBM.  Timed with HIP events on the launch stream, around
whole calls (the C ABI has no event between the passes of one call):
  (a) mipt_denoise_variance_device with all three guides, variance_out and iterations = 1 ... 5.  The call with k iterations runs the
      pack pass, the spatial-estimate pass and the passes of step 1 ... 2^(k-1); T(k) - T(k-1) is what the pass of step 2^(k-1) adds;
  (b) the same with short_history = 0, which skips the estimate pass: (a) - (b) is that pass;
  (c) mipt_denoise_device with 4 and 5 iterations, the comparator: their difference is one pass of the fixed filter;
  (d) a device-to-device copy of 24 B per pixel, the comparator of tools/denoise_time.py.
All cells alternate inside every repetition; reported per cell: median, min and max of the repetitions and the spread
(max - min) / median; then the per-pass figures and their ratios to the fixed filter's pass and to the copy.

    python tools/variance_time.py [--tris 10000000] [--reps 7] [--json profiles/variance_time.json]
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
SHORT_HISTORY = 4.0


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
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "variance_time.json"))
    args = ap.parse_args()

    import torch

    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("variance_time.py measures on an MI355X: no HIP device visible")
    lib = rrt.load()
    dev = torch.device("cuda:0")
    tris, mats, texs, cam = synth.atrium_scene(n_target=args.tris, tex_size=args.tex_size)
    scene = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    n_tris = len(tris)
    del tris
    scene.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    scene.upload_from_triangles(0)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    w, h = args.width, args.height
    n = w * h
    # the inputs: the last frame of a short moving sequence, so that histories of every length up to `frames` occur
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=8, output_image_dimensions=(w, h), output_image_path="/dev/null",
                                             seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED, cull_margin=L.CULL_MARGIN_SAFE))
    path = []
    for f in range(args.frames):
        c = rrt.Camera(position=(float(cam[0][0]) + 0.02 * f, float(cam[0][1]), float(cam[0][2]) + 0.01 * f), pitch=cam[1], yaw=cam[2] + 0.4 * f)
        c.update_view()
        path.append(c)
    for fr in r.render_sequence(scene, path, denoise=False):
        last = fr
    torch.cuda.synchronize()
    hdr, variance, length = last["accumulated"], last["variance"], last["length"]
    planes = {k: last["features"][k] for k in ("normal", "depth", "albedo")}
    short = float((length < SHORT_HISTORY).float().mean().item())
    out = torch.empty_like(hdr)
    var_out = torch.empty_like(variance)

    need = int(lib.mipt_denoise_variance_workspace_bytes(w, h, 1))
    assert need == int(lib.mipt_denoise_workspace_bytes(w, h, 1))
    workspace = torch.empty((need // 16, 4), dtype=torch.float32, device=dev)
    vb = L.MiptVarianceBuffers()
    vb.hdr, vb.out, vb.variance, vb.length, vb.variance_out = hdr.data_ptr(), out.data_ptr(), variance.data_ptr(), length.data_ptr(), var_out.data_ptr()
    db = L.MiptDenoiseBuffers()
    db.hdr, db.out = hdr.data_ptr(), out.data_ptr()
    for k, t in planes.items():
        setattr(vb, k, t.data_ptr())
        setattr(db, k, t.data_ptr())
    vo = L.MiptVarianceOptions()
    vo.width, vo.height, vo.n_views = w, h, 1
    vo.sigma_luminance, vo.sigma_normal, vo.sigma_depth = 16.0, 0.5, 0.5
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

    def guided(k, short_history):
        vo.iterations, vo.short_history = k, short_history
        L.check(lib.mipt_denoise_variance_device(C.byref(vo), C.byref(vb), C.c_void_p(workspace.data_ptr()), need, sp), "mipt_denoise_variance_device")

    def fixed(k):
        do.iterations = k
        L.check(lib.mipt_denoise_device(C.byref(do), C.byref(db), C.c_void_p(workspace.data_ptr()), need, sp), "mipt_denoise_device")

    copy_src = torch.empty((n * 6,), dtype=torch.float32, device=dev)       # 24 B per pixel
    copy_dst = torch.empty_like(copy_src)
    copy_src.normal_()

    def rounds(k):
        cells = {f"{name}_{i}": [] for name in ("iterations", "no_estimate") for i in range(1, ITERATIONS + 1)}
        cells.update(fixed_4=[], fixed_5=[], copy=[])
        for _ in range(k):                                                    # every cell once per repetition
            for i in range(1, ITERATIONS + 1):
                cells[f"iterations_{i}"].append(timed(lambda: guided(i, SHORT_HISTORY)))
                cells[f"no_estimate_{i}"].append(timed(lambda: guided(i, 0.0)))
            cells["fixed_4"].append(timed(lambda: fixed(4)))
            cells["fixed_5"].append(timed(lambda: fixed(5)))
            cells["copy"].append(timed(lambda: copy_dst.copy_(copy_src)))
        return cells

    rounds(args.warmup)
    cells = rounds(args.reps)
    res = {"scene": dict(n_tris=n_tris),
           "config": dict(frame=f"{w}x{h}", views=1, samples=1, max_ray_depth=8, frames_accumulated=args.frames, guides=["normal", "depth", "albedo"],
                          sigma_luminance=16.0, sigma_normal=0.5, sigma_depth=0.5, short_history=SHORT_HISTORY,
                          pixels_below_short_history=round(short, 4), warmup=args.warmup, reps=args.reps, device=torch.cuda.get_device_name(0),
                          timing="HIP events on the launch stream around whole calls"),
           "workspace_bytes": need}
    for i in range(1, ITERATIONS + 1):
        res[f"variance_iterations_{i}"] = cell(cells[f"iterations_{i}"])
    for i in range(1, ITERATIONS + 1):
        res[f"variance_no_estimate_iterations_{i}"] = cell(cells[f"no_estimate_{i}"])
    res["denoise_iterations_4"], res["denoise_iterations_5"] = cell(cells["fixed_4"]), cell(cells["fixed_5"])
    res["copy_24B_per_pixel"] = dict(cell(cells["copy"]), bytes_moved=48 * n, gbyte_s=round(48 * n / float(np.median(cells["copy"])) / 1e6, 1))
    med = [0.0] + [res[f"variance_iterations_{i}"]["ms_median"] for i in range(1, ITERATIONS + 1)]
    bare = [0.0] + [res[f"variance_no_estimate_iterations_{i}"]["ms_median"] for i in range(1, ITERATIONS + 1)]
    copy = res["copy_24B_per_pixel"]["ms_median"]
    fixed_pass = res["denoise_iterations_5"]["ms_median"] - res["denoise_iterations_4"]["ms_median"]
    res["fixed_pass_ms"] = round(fixed_pass, 4)
    res["estimate_pass_ms"] = round(float(np.median([med[i] - bare[i] for i in range(1, ITERATIONS + 1)])), 4)
    res["pack_plus_first_pass_ms"] = round(bare[1], 4)
    res["added_by_pass"] = [dict(step=1 << (i - 1), ms=round(bare[i] - bare[i - 1], 4), over_fixed_pass=round((bare[i] - bare[i - 1]) / fixed_pass, 2),
                                 over_copy=round((bare[i] - bare[i - 1]) / copy, 2)) for i in range(2, ITERATIONS + 1)]
    res["total_over_fixed_total"] = round(med[ITERATIONS] / res["denoise_iterations_5"]["ms_median"], 2)
    res["total_mpixel_s"] = round(n / med[ITERATIONS] / 1e3, 1)
    for k, v in res.items():
        if k not in ("scene", "config"):
            print(k, json.dumps(v), flush=True)
    print("config", json.dumps(res["config"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    scene.release()


if __name__ == "__main__":
    main()
