"""The temporal accumulation at 1080p against the least traffic it could have.

One MI355X, the 10 M-triangle stand-in scene bench.py builds, 1920x1080, one view.  The inputs are real: the 1 spp frame of
mipt_render_batch_device and the position, normal, depth, material and albedo planes of mipt_render_features_device, all left in
HBM; the history is the one mipt_temporal_device itself wrote for the frame before.  Timed with HIP events on the launch stream,
around whole calls:
  (a) mipt_temporal_device with albedo and without length / variance: the first frame (no history), a frame whose history comes
      from the same camera, and a frame whose history comes from a camera 0.02 / 0.01 to the side and 0.4 degrees of yaw away;
      the moved frame again with length and variance written;
  (b) a device-to-device copy of 82 B per pixel: 82 B read + 82 B written, the 164 B per pixel the call must move at least --
      56 B of planes and 48 B of history in, 48 B of history and 12 B of output out;
  (c) quoted, not measured here: what one a-trous pass adds, from profiles/denoise_time.json.
All cells alternate inside every repetition; reported per cell: median, min and max of the repetitions and the spread
(max - min) / median; then the ratios.  Not measured: more than one view, other frame sizes, the host entry.

    python tools/temporal_time.py [--tris 10000000] [--reps 7] [--json profiles/temporal_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COMPULSORY_BYTES = dict(read_planes=56, read_history=48, write_history=48, write_out=12)


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
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "temporal_time.json"))
    args = ap.parse_args()

    import torch

    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("temporal_time.py measures on an MI355X: no HIP device visible")
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
    before = rrt.Camera(position=(cam[0][0] - 0.02, cam[0][1], cam[0][2] - 0.01), pitch=cam[1], yaw=cam[2] - 0.4)
    before.update_view()
    tables = {name: np.ascontiguousarray(np.asarray(c.uniform, dtype=L.CAMERA).reshape(1)) for name, c in (("now", scene.camera), ("before", before))}

    def frame(name, sample):
        """the 1 spp frame and the feature planes of one camera, left in HBM"""
        o = rrt.make_options(w, h, 1, 8, seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED, cull_margin=L.CULL_MARGIN_SAFE, sample_begin=sample)
        hdr = torch.empty((1, h, w, 3), dtype=torch.float32, device=dev)
        L.check(lib.mipt_render_batch_device(handle, L.ptr(tables[name]), 1, C.byref(o), C.c_void_p(hdr.data_ptr()), None, sp, C.byref(st)), "mipt_render_batch_device")
        planes = dict(hdr=hdr, depth=torch.empty((1, h, w), dtype=torch.float32, device=dev), material=torch.empty((1, h, w), dtype=torch.int32, device=dev))
        for k in ("position", "normal", "albedo"):
            planes[k] = torch.empty((1, h, w, 3), dtype=torch.float32, device=dev)
        fb = L.MiptFeatureBuffers()
        for k, t in planes.items():
            if k != "hdr":
                setattr(fb, k, t.data_ptr())
        o.sample_begin = 0
        L.check(lib.mipt_render_features_device(handle, L.ptr(tables[name]), 1, C.byref(o), C.byref(fb), sp, C.byref(st)), "mipt_render_features_device")
        return planes

    words = int(lib.mipt_temporal_history_bytes(w, h, 1)) // 4
    to = L.MiptTemporalOptions()
    to.width, to.height, to.n_views = w, h, 1
    to.alpha_min, to.max_history, to.normal_tol, to.depth_tol = 0.0, 32.0, 0.1, 0.1
    out = torch.empty((1, h, w, 3), dtype=torch.float32, device=dev)
    length, variance = torch.empty((1, h, w), dtype=torch.float32, device=dev), torch.empty((1, h, w), dtype=torch.float32, device=dev)
    hist = {name: torch.empty((words,), dtype=torch.int32, device=dev) for name in ("now", "before", "out")}

    def temporal(planes, table, history_in, history_out, extras=False):
        b = L.MiptTemporalBuffers()
        for k, t in planes.items():
            setattr(b, k, t.data_ptr())
        b.out, b.history_out = out.data_ptr(), history_out.data_ptr()
        b.history_in = history_in.data_ptr() if history_in is not None else None
        if extras:
            b.length, b.variance = length.data_ptr(), variance.data_ptr()
        L.check(lib.mipt_temporal_device(C.byref(to), L.ptr(table), C.byref(b), sp), "mipt_temporal_device")

    now, earlier = frame("now", 2), frame("before", 1)
    temporal(earlier, tables["before"], None, hist["before"])                 # the histories the timed frames read
    temporal(now, tables["now"], None, hist["now"])
    temporal(now, tables["now"], hist["before"], hist["out"], extras=True)
    torch.cuda.synchronize()
    reused = int((length > 1.0).sum().item())

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        f()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    moved = sum(COMPULSORY_BYTES.values())
    copy_src = torch.empty((n * moved // 2,), dtype=torch.uint8, device=dev)  # 82 B per pixel
    copy_dst = torch.empty_like(copy_src)
    copy_src.random_(0, 255)

    def rounds(k):
        cells = dict(first_frame=[], same_camera=[], moved_camera=[], moved_camera_length_variance=[], copy=[])
        for _ in range(k):                                                    # every cell once per repetition
            cells["first_frame"].append(timed(lambda: temporal(now, tables["now"], None, hist["out"])))
            cells["same_camera"].append(timed(lambda: temporal(now, tables["now"], hist["now"], hist["out"])))
            cells["moved_camera"].append(timed(lambda: temporal(now, tables["now"], hist["before"], hist["out"])))
            cells["moved_camera_length_variance"].append(timed(lambda: temporal(now, tables["now"], hist["before"], hist["out"], extras=True)))
            cells["copy"].append(timed(lambda: copy_dst.copy_(copy_src)))
        return cells

    rounds(args.warmup)
    cells = rounds(args.reps)
    res = {"scene": dict(n_tris=n_tris),
           "config": dict(frame=f"{w}x{h}", views=1, samples=1, max_ray_depth=8, albedo=True, alpha_min=0.0, max_history=32.0, normal_tol=0.1, depth_tol=0.1,
                          warmup=args.warmup, reps=args.reps, device=torch.cuda.get_device_name(0),
                          timing="HIP events on the launch stream around whole calls"),
           "history_bytes": words * 4, "compulsory_bytes_per_pixel": COMPULSORY_BYTES, "pixels_reused_moved_camera": reused, "pixels": n}
    for k in ("first_frame", "same_camera", "moved_camera", "moved_camera_length_variance"):
        res[f"temporal_{k}"] = dict(cell(cells[k]), mpixel_s=round(n / float(np.median(cells[k])) / 1e3, 1))
    res["copy_82B_per_pixel"] = dict(cell(cells["copy"]), bytes_moved=moved * n, gbyte_s=round(moved * n / float(np.median(cells["copy"])) / 1e6, 1))
    copy = res["copy_82B_per_pixel"]["ms_median"]
    res["moved_camera_over_copy"] = round(res["temporal_moved_camera"]["ms_median"] / copy, 2)
    res["same_camera_over_copy"] = round(res["temporal_same_camera"]["ms_median"] / copy, 2)
    denoise_json = os.path.join(ROOT, "profiles", "denoise_time.json")
    if os.path.exists(denoise_json):                                          # quoted: measured by tools/denoise_time.py, not here
        with open(denoise_json) as f:
            passes = [p["ms"] for p in json.load(f)["added_by_pass"]]
        res["atrous_pass_ms_quoted"] = dict(source="profiles/denoise_time.json added_by_pass", mean_ms=round(float(np.mean(passes)), 4))
        res["moved_camera_over_atrous_pass"] = round(res["temporal_moved_camera"]["ms_median"] / float(np.mean(passes)), 2)
    res["not_measured"] = ["more than one view", "frame sizes other than this one", "the host entry mipt_temporal", "render_sequence end to end"]
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
