"""The count-aware temporal blend and the filling sample map: what the image gains and what the two calls cost.

One MI355X.
  (1) quality, section 20's experiment unchanged: the oracle's 20 k-triangle atrium at 64x36, depth 8, the 8 moving frames, RMSE of
      the last frame's `out` against the 1024-sample frame of the last camera, and the paths traced, for five configurations of
      render_sequence(denoise="variance"): uniform 2 spp; adaptive = (min 1, max 8, budget 2) as it was; with blend="counts"; with
      rounds=4; with both.  Also the share of T = floor(budget * N) the map spends at 1, 2, 4 and 8 rounds, on the planes of every
      frame of the plain adaptive run.
  (2) cost, on the 10 M-triangle stand-in scene bench.py builds at 1920x1080, one view: a frame, its feature planes, a history and a
      count plane made by two frames of render_sequence(adaptive = min 1, max 16, budget 2); then mipt_temporal_counts_device
      against mipt_temporal_device on that frame, and mipt_sample_map_fill_device at 1, 2 and 4 rounds against
      mipt_sample_map_device on that frame's variance_out, out and albedo.  Every cell of a section alternates inside every
      repetition after a warm-up, all in this one process; per cell the median, min and max of the repetitions and the spread
      (max - min) / median, by HIP events on the launch stream around the call.

    python tools/weighted_time.py [--tris 10000000] [--reps 15] [--skip-timing] [--json profiles/weighted_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--skip-timing", action="store_true", help="section 1 alone")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "weighted_time.json"))
    args = ap.parse_args()

    import torch

    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("weighted_time.py measures on an MI355X: no HIP device visible")
    lib = rrt.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    res = {}

    def renderer(size, spp, depth=8):
        return rrt.Renderer.new(rrt.RendererOptions(samples=spp, max_ray_depth=depth, output_image_dimensions=size, output_image_path="/dev/null",
                                                    seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED, cull_margin=L.CULL_MARGIN_SAFE))

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        f()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def alternate(cells):
        t = {k: [] for k in cells}
        for rep in range(args.warmup + args.reps):
            for k, f in cells.items():
                ms = timed(f)
                if rep >= args.warmup:
                    t[k].append(ms)
        return {k: cell(v) for k, v in t.items()}

    # ---- (1) quality at equal path budget: the 20 k-triangle atrium, 64x36, 8 moving frames
    tris, mats, texs, pose = synth.make_scene("atrium", n_target=20000, tex_size=64)
    small = rrt.Scene.from_arrays(tris, mats, texs)
    qw, qh, frames = 64, 36, 8

    def camera(f):
        c = rrt.Camera(position=(float(pose[0][0]) + 0.02 * f, float(pose[0][1]), float(pose[0][2]) + 0.01 * f), pitch=pose[1], yaw=pose[2] + 0.4 * f)
        c.update_view()
        return c

    path = [camera(f) for f in range(frames)]
    small.set_camera(path[-1])
    o = rrt.make_options(qw, qh, 1024, 8, seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED, sample_begin=1000, cull_margin=L.CULL_MARGIN_SAFE)
    target = np.zeros((qh, qw, 3), dtype=np.float32)
    L.check(lib.mipt_render(small.upload(0), L.ptr(path[-1].uniform), C.byref(o), L.ptr(target), None, None), "mipt_render")

    def rmse(a, b):
        d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
        return float(np.sqrt(np.mean(d * d)))

    base = dict(min_samples=1, max_samples=8, budget=2.0)
    total = int(np.floor(2.0 * qw * qh))
    configs = (("uniform_2spp", None), ("adaptive_as_merged", base), ("adaptive_blend_counts", dict(base, blend="counts")),
               ("adaptive_rounds4", dict(base, rounds=4)), ("adaptive_blend_counts_rounds4", dict(base, blend="counts", rounds=4)))
    quality, spend = {}, {str(r): [] for r in (1, 2, 4, 8)}
    r2 = renderer((qw, qh), 2)
    for name, adaptive in configs:
        paths, per_frame = 0, []
        for fr in r2.render_sequence(small, path, denoise="variance", adaptive=adaptive):
            torch.cuda.synchronize()
            traced = int(fr["counts"].sum().item()) if "counts" in fr else 2 * qw * qh
            paths += traced
            per_frame.append(traced)
            out, noisy, acc = fr["out"][0].cpu().numpy(), fr["noisy"][0].cpu().numpy(), fr["accumulated"][0].cpu().numpy()
            if name == "adaptive_as_merged":
                for rounds in (1, 2, 4, 8):
                    c = r2.sample_map(fr["variance_out"], fr["out"], fr["features"]["albedo"], rounds=rounds, **base)
                    spend[str(rounds)].append(round(int(c.sum().item()) / total, 4))
        quality[name] = dict(rmse_out=round(rmse(out, target), 4), rmse_accumulated=round(rmse(acc, target), 4),
                             rmse_noisy_last_frame=round(rmse(noisy, target), 4), paths_traced=paths, paths_per_frame=per_frame,
                             mean_length_last_frame=round(float(fr["length"].mean().item()), 3))
        print("quality", name, json.dumps(quality[name]), flush=True)
    res["quality"] = dict(scene="atrium, 20 k triangles, 64x36, depth 8, 8 moving frames, target 1024 samples from 1000 at the last camera",
                          uniform_paths=2 * qw * qh * frames, **quality)
    res["share_of_T_spent"] = dict(note="sum(counts) / T per frame of the plain adaptive run, the map made with this many rounds", T=total,
                                   per_frame=spend, mean={k: round(float(np.mean(v)), 4) for k, v in spend.items()})
    print("share_of_T_spent", json.dumps(res["share_of_T_spent"]["mean"]), flush=True)
    small.release()

    # ---- (2) cost at 1080p on the 10 M-triangle scene
    if not args.skip_timing:
        tris, mats, texs, cam = synth.atrium_scene(n_target=args.tris, tex_size=args.tex_size)
        scene = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
        n_tris = len(tris)
        del tris
        scene.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
        scene.upload_from_triangles(0)
        w, h = args.width, args.height
        amap = dict(min_samples=1, max_samples=16, budget=2.0)
        big = renderer((w, h), 2)
        keep = []
        for fr in big.render_sequence(scene, [scene.camera] * 2, denoise="variance", adaptive=amap):
            torch.cuda.synchronize()
            keep.append(dict(noisy=fr["noisy"].clone(), counts=fr["counts"].clone(), history=fr["history"].clone(), out=fr["out"].clone(),
                             variance_out=fr["variance_out"].clone(), features={k: v.clone() for k, v in fr["features"].items()}))
        first, last = keep
        table = [scene.camera]
        hist_out = torch.empty_like(first["history"])
        counts = last["counts"]
        hist = np.bincount(counts.cpu().numpy().reshape(-1), minlength=17)

        def plain():
            big.temporal(last["noisy"], last["features"], table, history=first["history"], want_length=True, want_variance=True, stream=sp.value,
                         history_out=hist_out)

        def counted():
            big.temporal(last["noisy"], last["features"], table, history=first["history"], want_length=True, want_variance=True, stream=sp.value,
                         history_out=hist_out, counts=counts, samples_cap=16)

        t = alternate({"mipt_temporal_device": plain, "mipt_temporal_counts_device": counted})
        t["ratio"] = round(t["mipt_temporal_counts_device"]["ms_median"] / t["mipt_temporal_device"]["ms_median"], 4)
        t["counts_histogram"] = {str(i): int(c) for i, c in enumerate(hist) if c}
        t["note"] = "through Renderer.temporal (tensor checks and two small allocations included in both cells alike)"
        res["temporal"] = t
        print("temporal", json.dumps(t), flush=True)

        # the raw entries, nothing but the library call between the events
        n = w * h
        mo = L.MiptSampleMapOptions()
        mo.width, mo.height, mo.n_views, mo.min_samples, mo.max_samples, mo.budget = w, h, 1, 1, 16, 2.0
        out_counts = torch.empty((1, h, w), dtype=torch.int32, device=dev)
        workspace = torch.empty((64,), dtype=torch.int32, device=dev)
        mb = L.MiptSampleMapBuffers()
        mb.variance, mb.hdr, mb.albedo, mb.counts = (last["variance_out"].data_ptr(), last["out"].data_ptr(), last["features"]["albedo"].data_ptr(),
                                                     out_counts.data_ptr())

        def run_map():
            L.check(lib.mipt_sample_map_device(C.byref(mo), C.byref(mb), C.c_void_p(workspace.data_ptr()), sp), "mipt_sample_map_device")

        def run_fill(rounds):
            fo = L.MiptSampleMapFillOptions()
            fo.width, fo.height, fo.n_views, fo.min_samples, fo.max_samples, fo.budget, fo.rounds = w, h, 1, 1, 16, 2.0, rounds
            return lambda: L.check(lib.mipt_sample_map_fill_device(C.byref(fo), C.byref(mb), C.c_void_p(workspace.data_ptr()), sp), "mipt_sample_map_fill_device")

        cells = {"mipt_sample_map_device": run_map}
        cells.update({f"fill_rounds_{r}": run_fill(r) for r in (1, 2, 4)})
        m = alternate(cells)
        for r in (1, 2, 4):
            m[f"ratio_rounds_{r}"] = round(m[f"fill_rounds_{r}"]["ms_median"] / m["mipt_sample_map_device"]["ms_median"], 4)
            run_fill(r)()
            torch.cuda.synchronize()
            m[f"share_of_T_rounds_{r}"] = round(int(out_counts.sum().item()) / int(np.floor(2.0 * n)), 4)
        res["sample_map_fill"] = m
        print("sample_map_fill", json.dumps(m), flush=True)

        # the raw temporal entries
        f = last["features"]
        to = L.MiptTemporalOptions()
        to.width, to.height, to.n_views = w, h, 1
        to.alpha_min, to.max_history, to.normal_tol, to.depth_tol = 0.0, 32.0, 0.1, 0.1
        acc = torch.empty_like(last["noisy"])
        length, variance = torch.empty((1, h, w), dtype=torch.float32, device=dev), torch.empty((1, h, w), dtype=torch.float32, device=dev)
        tb = L.MiptTemporalBuffers()
        tb.hdr, tb.position, tb.normal, tb.depth, tb.material, tb.albedo = (last["noisy"].data_ptr(), f["position"].data_ptr(), f["normal"].data_ptr(),
                                                                            f["depth"].data_ptr(), f["material"].data_ptr(), f["albedo"].data_ptr())
        tb.history_in, tb.history_out, tb.out, tb.length, tb.variance = (first["history"].data_ptr(), hist_out.data_ptr(), acc.data_ptr(), length.data_ptr(),
                                                                         variance.data_ptr())
        cams = np.ascontiguousarray(np.asarray(scene.camera.uniform, dtype=L.CAMERA).reshape(1))

        def raw_plain():
            L.check(lib.mipt_temporal_device(C.byref(to), L.ptr(cams), C.byref(tb), sp), "mipt_temporal_device")

        def raw_counted():
            L.check(lib.mipt_temporal_counts_device(C.byref(to), L.ptr(cams), C.byref(tb), C.c_void_p(counts.data_ptr()), 16, sp), "mipt_temporal_counts_device")

        t = alternate({"mipt_temporal_device": raw_plain, "mipt_temporal_counts_device": raw_counted})
        t["ratio"] = round(t["mipt_temporal_counts_device"]["ms_median"] / t["mipt_temporal_device"]["ms_median"], 4)
        res["temporal_raw_entries"] = t
        print("temporal_raw_entries", json.dumps(t), flush=True)
        res["scene"] = dict(n_tris=n_tris)
        res["config"] = dict(frame=f"{w}x{h}", views=1, warmup=args.warmup, reps=args.reps, device=torch.cuda.get_device_name(0),
                             timing="HIP events on the launch stream around the call; the cells of a section alternate inside every repetition")
        scene.release()

    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
