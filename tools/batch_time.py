"""N views of one scene: N sequential mipt_render_device calls against ONE mipt_render_batch_device call.

For each view size and view count: kernel ms (HIP events: the sum over the N single launches, the one batch launch), wall ms (host
clock around the N calls / the one call, every call blocks until its kernel is done), the rays of the whole set from a separate
MIPT_FLAG_COUNT batch (the same count the singles trace: the batch's counters are the sums over its views), and Mray/s for both.
The bench scene (10 M triangles, synth.atrium_scene) at 8 spp, depth 64, culled traversal; view 0 is the bench camera, the others are
seeded random poses around it.

    python tools/batch_time.py [--tris 10000000] [--reps 3] [--json OUT]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--tex-size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3, help="timed repetitions per cell (median reported)")
    ap.add_argument("--sizes", default="64x64,128x128,256x256,1920x1080")
    ap.add_argument("--counts", default="1,8,64")
    ap.add_argument("--json", help="also write the rows to this file")
    args = ap.parse_args()

    import torch

    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth

    lib = rrt.load()
    dev = torch.device("cuda:0")
    tris, mats, texs, cam = synth.atrium_scene(n_target=args.tris, tex_size=args.tex_size)
    scene = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    del tris
    handle = scene.upload_from_triangles(0)
    counts = [int(x) for x in args.counts.split(",")]
    rng = np.random.default_rng(2026)
    poses = [rrt.Camera(position=tuple(cam[0]), pitch=cam[1], yaw=cam[2])]
    for _ in range(max(counts) - 1):
        pos = tuple(float(x) for x in np.array(cam[0]) + rng.uniform(-14.0, 14.0, 3) * np.array([1.0, 0.25, 1.0]))
        poses.append(rrt.Camera(position=pos, pitch=float(rng.uniform(-30, 30)), yaw=float(rng.uniform(-180, 180))))
    for p in poses:
        p.update_view()
    table_all = np.ascontiguousarray(np.stack([p.uniform for p in poses]))
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)

    rows = []
    for size in args.sizes.split(","):
        w, h = (int(x) for x in size.split("x"))
        npx = w * h
        for n in counts:
            if n * npx >= (1 << 32):
                continue
            o = rrt.make_options(w, h, args.spp, args.depth, traversal=L.TRAVERSAL_CULLED)
            oc = rrt.make_options(w, h, args.spp, args.depth, traversal=L.TRAVERSAL_CULLED, flags=L.FLAG_COUNT)
            buf = torch.empty(n * npx * 3, dtype=torch.float32, device=dev)
            st = L.MiptStats()
            table = table_all[:n]

            def singles():
                k = 0.0
                t0 = time.perf_counter()
                for v in range(n):
                    L.check(lib.mipt_render_device(handle, L.ptr(poses[v].uniform), C.byref(o), C.c_void_p(buf[v * npx * 3:].data_ptr()),
                                                   None, sp, C.byref(st)), "mipt_render_device")
                    k += st.kernel_ms
                return k, (time.perf_counter() - t0) * 1e3

            def batch(opt=o):
                t0 = time.perf_counter()
                L.check(lib.mipt_render_batch_device(handle, L.ptr(table), n, C.byref(opt), C.c_void_p(buf.data_ptr()), None, sp,
                                                     C.byref(st)), "mipt_render_batch_device")
                return st.kernel_ms, (time.perf_counter() - t0) * 1e3

            singles(); batch()                                             # warm-up (and workspace growth)
            s = [singles() for _ in range(args.reps)]
            b = [batch() for _ in range(args.reps)]
            batch(oc)
            rays = int(st.rays)
            sk, sw = float(np.median([x[0] for x in s])), float(np.median([x[1] for x in s]))
            bk, bw = float(np.median([x[0] for x in b])), float(np.median([x[1] for x in b]))
            row = dict(size=f"{w}x{h}", views=n, rays=rays, single_kernel_ms=round(sk, 3), single_wall_ms=round(sw, 3),
                       batch_kernel_ms=round(bk, 3), batch_wall_ms=round(bw, 3),
                       single_mray_s=round(rays / sw / 1e3, 1), batch_mray_s=round(rays / bw / 1e3, 1),
                       single_kernel_mray_s=round(rays / sk / 1e3, 1), batch_kernel_mray_s=round(rays / bk / 1e3, 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del buf
    print()
    print("| view | views | rays | N singles: kernel ms / wall ms | batch: kernel ms / wall ms | Mray/s (wall) singles -> batch |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['size']} | {r['views']} | {r['rays'] / 1e6:.2f} M | {r['single_kernel_ms']:.2f} / {r['single_wall_ms']:.2f} | "
              f"{r['batch_kernel_ms']:.2f} / {r['batch_wall_ms']:.2f} | {r['single_mray_s']:.0f} -> {r['batch_mray_s']:.0f} |")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    scene.release()


if __name__ == "__main__":
    main()
