"""The guided upsampling at 1080p against a copy, and the whole frame of render_sequence with and without it.

One MI355X, the 10 M-triangle stand-in scene bench.py builds, 1920x1080, one view.  The inputs are real: the filtered frame and the
feature planes a short render_sequence(denoise="variance") leaves in HBM at 1/k of the frame, and the full-resolution planes of
mipt_render_features_device.  Timed with HIP events on the launch stream, around whole calls (the C ABI has no event between the two
passes of one call):
  (a) mipt_upsample_device with all four guides and `weight`, k = 2 and 4;
  (b) the same without `weight`;
  (c) the pack pass as a difference: the k = 2 low frame upsampled with k = 4 to 3840x2160 runs the same pack pass and a full-frame
      pass over four times the pixels, so pack = (4 * T(low, 2) - T(low, 4)) / 3 -- IF the full-frame pass costs the same per full
      pixel at both scales, which nothing here measures; the figure is reported with that condition;
  (d) a device-to-device copy that moves the bytes the call must move at least -- 32 B in and 12 B (16 B with `weight`) out per full
      pixel plus 44 B in per low pixel -- so a copy of half as many bytes, read once and written once;
  (e) one frame of render_sequence(denoise="variance") at 1 spp, depth 8, in steady state along a moving camera: upsample=None,
      upsample=2 at 1 spp and upsample=2 at 4 spp (the path budget of upsample=None).
All cells alternate inside every repetition; reported per cell: median, min and max of the repetitions and the spread
(max - min) / median.

    python tools/upsample_time.py [--tris 10000000] [--reps 7] [--json profiles/upsample_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GUIDES = ("normal", "depth", "albedo", "material")


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
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "upsample_time.json"))
    args = ap.parse_args()

    import torch

    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("upsample_time.py measures on an MI355X: no HIP device visible")
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

    def renderer(size, spp):
        return rrt.Renderer.new(rrt.RendererOptions(samples=spp, max_ray_depth=8, output_image_dimensions=size, output_image_path="/dev/null",
                                                    seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED, cull_margin=L.CULL_MARGIN_SAFE))

    def camera(f):
        c = rrt.Camera(position=(float(cam[0][0]) + 0.02 * f, float(cam[0][1]), float(cam[0][2]) + 0.01 * f), pitch=cam[1], yaw=cam[2] + 0.4 * f)
        c.update_view()
        return c

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        f()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    # ---- the call: inputs left in HBM by the pipeline at 1/k, and the full-resolution planes
    def call_for(k, full):
        """-> a function (with_weight) that queues one mipt_upsample_device of the W/k x H/k frame to `full`, and its sizes"""
        fw, fh = full
        lw, lh = fw // k, fh // k
        for fr in renderer((lw, lh), 1).render_sequence(scene, [camera(f) for f in range(args.frames)], denoise="variance"):
            last = fr
        hi, _ = renderer(full, 1).render_features(scene, [camera(args.frames - 1)], GUIDES, device=True)
        torch.cuda.synchronize()
        keep = dict(lo_hdr=last["out"], out=torch.empty((1, fh, fw, 3), dtype=torch.float32, device=dev),
                    weight=torch.empty((1, fh, fw), dtype=torch.float32, device=dev))
        for g in GUIDES:
            keep["lo_" + g], keep[g] = last["features"][g], hi[g]
        need = int(lib.mipt_upsample_workspace_bytes(fw, fh, 1, k))
        assert need == lw * lh * 32
        keep["workspace"] = torch.empty((need // 16, 4), dtype=torch.float32, device=dev)
        o = L.MiptUpsampleOptions()
        o.width, o.height, o.n_views, o.scale, o.sigma_normal, o.sigma_depth = fw, fh, 1, k, 0.5, 0.5
        bufs = []
        for with_weight in (False, True):
            b = L.MiptUpsampleBuffers()
            for name, t in keep.items():
                if name != "workspace" and (name != "weight" or with_weight):
                    setattr(b, name, t.data_ptr())
            bufs.append(b)

        def run(with_weight):
            L.check(lib.mipt_upsample_device(C.byref(o), C.byref(bufs[int(with_weight)]), C.c_void_p(keep["workspace"].data_ptr()), need, sp), "mipt_upsample_device")

        run(True)
        torch.cuda.synchronize()
        fallback = float((keep["weight"] == 0).float().mean().item())
        return run, keep, dict(low=f"{lw}x{lh}", full=f"{fw}x{fh}", workspace_bytes=need, pixels_without_an_accepted_tap=round(fallback, 4))

    calls = {k: call_for(k, (w, h)) for k in (2, 4)}
    big = call_for(4, (2 * w, 2 * h))                                         # the k = 2 low frame size, upsampled four times

    def copy_pair(nbytes):                                                    # moves nbytes: half of them read, half written
        src = torch.empty(((nbytes // 2 + 3) // 4,), dtype=torch.float32, device=dev)
        src.normal_()
        return src, torch.empty_like(src)

    copies = {}
    for k in (2, 4):
        for with_weight in (False, True):
            copies[k, with_weight] = copy_pair(n * (32 + (16 if with_weight else 12)) + (n // (k * k)) * 44)

    # ---- the frame: three sequences in steady state, one frame of each per repetition
    total = args.frames + args.warmup + args.reps
    path = [camera(f) for f in range(total)]
    sequences = dict(frame_full_1spp=renderer((w, h), 1).render_sequence(scene, path, denoise="variance"),
                     frame_upsample2_1spp=renderer((w, h), 1).render_sequence(scene, path, denoise="variance", upsample=2),
                     frame_upsample2_4spp=renderer((w, h), 4).render_sequence(scene, path, denoise="variance", upsample=2))
    for _ in range(args.frames):                                              # histories of every length up to `frames`
        for gen in sequences.values():
            next(gen)
    torch.cuda.synchronize()

    def rounds(reps):
        cells = {name: [] for name in sequences}
        for k in (2, 4):
            cells.update({f"upsample_k{k}": [], f"upsample_k{k}_no_weight": [], f"copy_k{k}": [], f"copy_k{k}_no_weight": []})
        cells["upsample_k4_to_2x_frame"] = []
        for _ in range(reps):                                                 # every cell once per repetition
            for k in (2, 4):
                run = calls[k][0]
                cells[f"upsample_k{k}"].append(timed(lambda: run(True)))
                cells[f"upsample_k{k}_no_weight"].append(timed(lambda: run(False)))
                for with_weight in (True, False):
                    src, dst = copies[k, with_weight]
                    cells[f"copy_k{k}" + ("" if with_weight else "_no_weight")].append(timed(lambda: dst.copy_(src)))
            cells["upsample_k4_to_2x_frame"].append(timed(lambda: big[0](True)))
            for name, gen in sequences.items():
                cells[name].append(timed(lambda: next(gen)))
        return cells

    rounds(args.warmup)
    cells = rounds(args.reps)
    res = {"scene": dict(n_tris=n_tris),
           "config": dict(frame=f"{w}x{h}", views=1, max_ray_depth=8, guides=list(GUIDES), sigma_normal=0.5, sigma_depth=0.5,
                          frames_before_timing=args.frames, warmup=args.warmup, reps=args.reps, device=torch.cuda.get_device_name(0),
                          timing="HIP events on the launch stream around whole calls; a frame is one next() of render_sequence, host work between its launches included")}
    for k in (2, 4):
        res[f"upsample_k{k}"] = dict(cell(cells[f"upsample_k{k}"]), **calls[k][2])
        res[f"upsample_k{k}_no_weight"] = cell(cells[f"upsample_k{k}_no_weight"])
        for with_weight in (True, False):
            name = f"copy_k{k}" + ("" if with_weight else "_no_weight")
            nbytes = 2 * copies[k, with_weight][0].numel() * 4
            res[name] = dict(cell(cells[name]), bytes_the_call_must_move=nbytes, bytes_copied=nbytes // 2,
                             gbyte_s=round(nbytes / float(np.median(cells[name])) / 1e6, 1))
            up = res[f"upsample_k{k}" + ("" if with_weight else "_no_weight")]
            up["over_copy"] = round(up["ms_median"] / res[name]["ms_median"], 2)
        res[f"upsample_k{k}"]["mpixel_s"] = round(n / res[f"upsample_k{k}"]["ms_median"] / 1e3, 1)
    res["upsample_k4_to_2x_frame"] = dict(cell(cells["upsample_k4_to_2x_frame"]), **big[2])
    t2, t4 = res["upsample_k2"]["ms_median"], res["upsample_k4_to_2x_frame"]["ms_median"]
    res["pack_pass_k2_ms_by_difference"] = dict(ms=round((4.0 * t2 - t4) / 3.0, 4), formula="(4 * upsample_k2 - upsample_k4_to_2x_frame) / 3",
                                                condition="the full-frame pass costs the same per full pixel at k = 2 and k = 4: not measured")
    base = cell(cells["frame_full_1spp"])
    res["frame_full_1spp"] = base
    for name in ("frame_upsample2_1spp", "frame_upsample2_4spp"):
        res[name] = dict(cell(cells[name]), over_frame_full_1spp=round(float(np.median(cells[name])) / base["ms_median"], 3))
    res["not_measured"] = ["the pack pass alone (only as the difference above)", "whether the 64/k + 1 low texels a tile row shares are served from the vector L1: no counters were collected",
                           "k other than 2 and 4", "more than one view"]
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
