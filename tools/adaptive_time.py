"""Adaptive sampling at 1080p: what the count plane costs, what a skewed map buys, what the map itself costs, and what the image gains
(DESIGN.md section 20).

One MI355X.  Timing runs on the 10 M-triangle stand-in scene bench.py builds, 1920x1080, one view, depth 8, per-sample seeds, culled
traversal; every cell of a section alternates inside every repetition, after a warm-up; reported per cell: median, min and max of
the repetitions and the spread (max - min) / median.  Two clocks per render call: `kernel_ms`, the library's HIP events around the
trace kernel alone, and `call_ms`, HIP events on the launch stream around the whole call (the frame's memset, the camera table, the
launches behind the trace and the host's wait included).
  (1) overhead: mipt_render_adaptive_device with a uniform plane of k against mipt_render_batch_device with samples = k, k = 1, 2, 4,
      frames compared bit for bit;
  (2) skew: a real map made by render_sequence(adaptive = min 1, max 16, budget 2) on the same view, its histogram, the adaptive
      frame with it against the uniform 2-sample batch frame; rays and Mray/s from a MIPT_FLAG_COUNT run of each, taken separately;
      with --ordered-lib (a build variant that hands the pixels out by decreasing count) the A/B of the two work orders on that map;
  (3) mipt_sample_map_device against a device copy of the bytes it must move (16 or 28 B per pixel in, 4 out);
  (4) quality, on the oracle's 20 k-triangle atrium at 64x36 over the 8 moving frames the temporal and variance rows use: RMSE of
      render_sequence(denoise="variance") against the 1024-sample frame of the last camera at a uniform 2 spp and with
      adaptive = (min 1, max 8, budget 2), with the paths each run traced.

    python tools/adaptive_time.py [--tris 10000000] [--reps 7] [--ordered-lib rust_ray_tracing_amd/variants/adaptive_ordered.so]
                                  [--json profiles/adaptive_time.json]
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
    ap.add_argument("--frames", type=int, default=4, help="frames of the sequence that makes the map of section 2")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ordered-lib", default=None, help="a variant built with EXTRA=-DMIPT_ADAPTIVE_ORDERED=1 (tools/experiments)")
    ap.add_argument("--skip-timing", action="store_true", help="section 4 alone")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "adaptive_time.json"))
    args = ap.parse_args()

    import torch

    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("adaptive_time.py measures on an MI355X: no HIP device visible")
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
        out = f()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b), out

    if not args.skip_timing:
        tris, mats, texs, cam = synth.atrium_scene(n_target=args.tris, tex_size=args.tex_size)
        scene = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
        n_tris = len(tris)
        del tris
        scene.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
        handle = scene.upload_from_triangles(0)
        w, h = args.width, args.height
        n = w * h
        table = np.ascontiguousarray(np.asarray(scene.camera.uniform, dtype=L.CAMERA).reshape(1))
        libs = {"plain": (lib, handle)}
        if args.ordered_lib:
            other = L._bind(C.CDLL(os.path.abspath(args.ordered_lib), mode=C.RTLD_LOCAL))
            desc, hnd = scene.desc(), C.c_void_p()
            assert other.mipt_scene_create_from_triangles(C.byref(desc), 0, C.byref(hnd)) == 0, other.mipt_last_error()
            libs["ordered"] = (other, hnd)

        def options(samples, flags=0):
            return rrt.make_options(w, h, samples, 8, seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED, flags=flags, cull_margin=L.CULL_MARGIN_SAFE)

        frame = [torch.empty((1, h, w, 3), dtype=torch.float32, device=dev) for _ in range(2)]

        def batch(samples, flags=0, out=frame[0]):
            st = L.MiptStats()
            L.check(lib.mipt_render_batch_device(handle, L.ptr(table), 1, C.byref(options(samples, flags)), out.data_ptr(), None, sp, C.byref(st)), "mipt_render_batch_device")
            return st

        def adaptive(counts, cap, flags=0, which="plain", out=frame[1]):
            st = L.MiptStats()
            use, hnd = libs[which]
            rc = use.mipt_render_adaptive_device(hnd, L.ptr(table), 1, C.byref(options(cap, flags)), counts.data_ptr(), out.data_ptr(), None, sp, C.byref(st))
            assert rc == 0, use.mipt_last_error()
            return st

        def rounds(cells, reps):
            """cells: {name: function -> MiptStats}; every cell once per repetition -> {name: (call ms list, kernel ms list)}"""
            out = {name: ([], []) for name in cells}
            for _ in range(reps):
                for name, f in cells.items():
                    ms, st = timed(f)
                    out[name][0].append(ms)
                    out[name][1].append(st.kernel_ms)
            return out

        def report(times):
            return {name: dict(call=cell(t[0]), kernel=cell(t[1])) for name, t in times.items()}

        # ---- (1) overhead of the count plane
        overhead = {}
        for k in (1, 2, 4):
            uniform = torch.full((1, h, w), k, dtype=torch.int32, device=dev)
            cells = {f"batch_{k}spp": lambda k=k: batch(k), f"adaptive_uniform_{k}": lambda k=k, u=uniform: adaptive(u, k)}
            rounds(cells, args.warmup)
            same = bool(torch.equal(frame[0].view(torch.int32), frame[1].view(torch.int32)))
            r = report(rounds(cells, args.reps))
            r["bit_identical"] = same
            r["kernel_ratio"] = round(r[f"adaptive_uniform_{k}"]["kernel"]["ms_median"] / r[f"batch_{k}spp"]["kernel"]["ms_median"], 4)
            r["call_ratio"] = round(r[f"adaptive_uniform_{k}"]["call"]["ms_median"] / r[f"batch_{k}spp"]["call"]["ms_median"], 4)
            overhead[f"k{k}"] = r
            print("overhead", k, json.dumps(r), flush=True)
        res["overhead"] = overhead

        # ---- (2) a real, skewed map on the same view; a second map with a cap of 4 shows what the longest chain costs
        for key, amap in (("skew", dict(min_samples=1, max_samples=16, budget=2.0)), ("skew_max4", dict(min_samples=1, max_samples=4, budget=2.0))):
            cap = amap["max_samples"]
            for fr in renderer((w, h), 2).render_sequence(scene, [scene.camera] * args.frames, denoise="variance", adaptive=amap):
                pass
            torch.cuda.synchronize()
            if key == "skew":
                last = fr
            counts = fr["counts"].clone()
            hist = np.bincount(counts.cpu().numpy().reshape(-1), minlength=17)
            skew = dict(map=amap, frames=args.frames, histogram={str(i): int(c) for i, c in enumerate(hist) if c},
                        mean_count=round(float(counts.float().mean().item()), 4), paths=int(counts.sum().item()))
            cells = {"batch_2spp": lambda: batch(2), "adaptive_map": lambda: adaptive(counts, cap)}
            if "ordered" in libs:
                cells["adaptive_map_ordered"] = lambda: adaptive(counts, cap, which="ordered", out=frame[0])
            rounds(cells, args.warmup)
            if "ordered" in libs:
                adaptive(counts, cap)
                adaptive(counts, cap, which="ordered", out=frame[0])
                skew["ordered_bit_identical"] = bool(torch.equal(frame[0].view(torch.int32), frame[1].view(torch.int32)))
            skew.update(report(rounds(cells, args.reps)))
            for name, f in (("batch_2spp", lambda: batch(2, L.FLAG_COUNT)), ("adaptive_map", lambda: adaptive(counts, cap, L.FLAG_COUNT))):
                st = f()                                                     # a counting build: its time is not the frame's
                skew[name]["rays"] = int(st.rays)
                skew[name]["pixels"] = int(st.pixels)
                skew[name]["tail_share"] = round(st.diag[10] / max(st.diag[8], 1), 4)
                skew[name]["mray_s"] = round(st.rays / skew[name]["kernel"]["ms_median"] / 1e3, 1)
            res[key] = skew
            print(key, json.dumps(skew), flush=True)

        # ---- (3) the map against a copy
        variance, hdr, albedo = last["variance_out"], last["out"], last["features"]["albedo"]
        mo = L.MiptSampleMapOptions()
        mo.width, mo.height, mo.n_views, mo.min_samples, mo.max_samples, mo.budget = w, h, 1, 1, 16, 2.0
        out_counts = torch.empty((1, h, w), dtype=torch.int32, device=dev)
        workspace = torch.empty((int(lib.mipt_sample_map_workspace_bytes(w, h, 1)) // 4,), dtype=torch.int32, device=dev)
        cost = {}
        for name, a in (("variance_hdr_albedo", (variance, hdr, albedo)), ("variance", (variance, None, None))):
            nbytes = n * ((28 if a[1] is not None else 4) + 4)
            src = torch.empty((nbytes // 8,), dtype=torch.float32, device=dev).normal_()
            dst = torch.empty_like(src)
            mb = L.MiptSampleMapBuffers()
            mb.variance, mb.counts = a[0].data_ptr(), out_counts.data_ptr()
            mb.hdr, mb.albedo = (a[1].data_ptr(), a[2].data_ptr()) if a[1] is not None else (None, None)

            def run_map(mb=mb):
                L.check(lib.mipt_sample_map_device(C.byref(mo), C.byref(mb), C.c_void_p(workspace.data_ptr()), sp), "mipt_sample_map_device")

            cells = {"map": run_map, "copy": lambda: dst.copy_(src)}
            t = {k: [] for k in cells}
            for rep in range(args.warmup + args.reps):
                for k, f in cells.items():
                    ms, _ = timed(f)
                    if rep >= args.warmup:
                        t[k].append(ms)
            cost[name] = dict(map=cell(t["map"]), copy=cell(t["copy"]), bytes_the_call_must_move=nbytes,
                              over_copy=round(float(np.median(t["map"]) / np.median(t["copy"])), 2))
        res["sample_map"] = cost
        print("sample_map", json.dumps(cost), flush=True)
        res["scene"] = dict(n_tris=n_tris)
        res["config"] = dict(frame=f"{w}x{h}", views=1, max_ray_depth=8, seed_mode="per sample", traversal="culled", warmup=args.warmup, reps=args.reps,
                             device=torch.cuda.get_device_name(0),
                             timing="kernel = the library's HIP events around the trace kernel; call = HIP events on the launch stream around the whole call")
        if "ordered" in libs:
            libs["ordered"][0].mipt_scene_destroy(libs["ordered"][1])
        scene.release()

    # ---- (4) quality at equal path budget: the 20 k-triangle atrium, 64x36, 8 moving frames
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

    quality = {}
    for name, kw in (("uniform_2spp", {}), ("adaptive_min1_max8_budget2", dict(adaptive=dict(min_samples=1, max_samples=8, budget=2.0)))):
        paths, per_frame = 0, []
        for fr in renderer((qw, qh), 2).render_sequence(small, path, denoise="variance", **kw):
            torch.cuda.synchronize()
            traced = int(fr["counts"].sum().item()) if "counts" in fr else 2 * qw * qh
            paths += traced
            per_frame.append(traced)
            out, noisy = fr["out"][0].cpu().numpy(), fr["noisy"][0].cpu().numpy()
        quality[name] = dict(rmse_out=round(rmse(out, target), 4), rmse_noisy_last_frame=round(rmse(noisy, target), 4), paths_traced=paths, paths_per_frame=per_frame)
    res["quality"] = dict(scene="atrium, 20 k triangles, 64x36, depth 8, 8 moving frames, target 1024 samples from 1000 at the last camera", **quality)
    print("quality", json.dumps(res["quality"]), flush=True)
    small.release()

    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
