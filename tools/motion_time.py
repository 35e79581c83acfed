"""The previous-position pass against a position-only feature pass of the same frame, and what tracking adds to an update
(DESIGN.md section 17).

One MI355X, the 10 M-triangle bench mesh with 64 parts as tools/mesh_time.py builds it, 1920x1080, culled traversal with
MIPT_CULL_MARGIN_SAFE, one sample, MIPT_SEED_PIXEL_STREAM.  The scene tracks motion and has had one mipt_scene_set_transforms, so the
previous generation differs from the current one.  HIP events around whole calls, and MiptStats.kernel_ms beside them, of
  (a) mipt_render_motion_device with the tracked source,
  (b) mipt_render_motion_device with the explicit source (the previous generation's expansion in HBM),
  (c) mipt_render_features_device with only `position` wanted: the same traversal, the same 12 B stored per pixel, nothing gathered.
The three alternate inside every repetition.  Then, alternating as well, a REFIT by mipt_scene_set_transforms and one by
mipt_scene_update_mesh_device with new positions, each on the tracked and on the untracked scene.  Median of the repetitions after
the warm-ups, min, max and spread per cell; the ratios (a) / (c) and (b) / (c); the bytes a hit pixel gathers in each form.

    python tools/motion_time.py [--tris 10000000] [--parts 64] [--reps 7] [--json profiles/motion_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))


def cell(ms, kernel_ms=None):
    ms = np.asarray(ms, dtype=np.float64)
    med = float(np.median(ms))
    out = dict(call_ms_median=round(med, 4), call_ms_min=round(float(ms.min()), 4), call_ms_max=round(float(ms.max()), 4),
               spread=round(float((ms.max() - ms.min()) / med), 4), reps=len(ms))
    if kernel_ms is not None:
        out["kernel_ms_median"] = round(float(np.median(kernel_ms)), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--tex-size", type=int, default=1024)
    ap.add_argument("--parts", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "motion_time.json"))
    args = ap.parse_args()

    import torch

    import mesh_model
    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth

    if not torch.cuda.is_available():
        raise SystemExit("motion_time.py measures on an MI355X: no HIP device visible")
    lib = rrt.load()
    dev = torch.device("cuda:0")
    tris, mats, texs, cam = synth.atrium_scene(n_target=args.tris, tex_size=args.tex_size)
    mesh, _ = mesh_model.mesh_from_triangles(tris, args.parts)
    n_tris = len(tris)
    del tris
    n_parts = len(mesh["parts"])
    rng = np.random.default_rng(1)

    def pose(k):
        m = np.zeros((n_parts, 4, 4), dtype=np.float32)
        m[:, 0, 0] = m[:, 1, 1] = m[:, 2, 2] = m[:, 3, 3] = 1.0
        m[:, 3, :3] = rng.normal(0, 1e-3 * (k + 1), (n_parts, 3))
        return m.reshape(n_parts, 16)

    poses = [pose(k) for k in range(4)]
    scene = rrt.Scene.from_mesh(materials=mats, textures=texs, **mesh)
    scene.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    handle = scene.upload_from_mesh(0)
    plain = scene.mesh_info()
    scene.track_motion()
    tracked_info = scene.mesh_info()
    # the previous generation: pose 0; the current one: pose 1.  The explicit source is pose 0's expansion, made on the host.
    L.check(lib.mipt_scene_set_transforms(handle, L.ptr(poses[0]), n_parts, L.UPDATE_REFIT, None), "mipt_scene_set_transforms")
    tmp = rrt.Scene()
    tmp.mesh = dict(scene.mesh)
    tmp._set_mesh_transforms(poses[0])
    d_prev = torch.from_numpy(tmp.expand_mesh().view(np.uint8)).to(dev)
    del tmp
    L.check(lib.mipt_scene_set_transforms(handle, L.ptr(poses[1]), n_parts, L.UPDATE_REFIT, None), "mipt_scene_set_transforms")
    torch.cuda.synchronize()

    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    w, h = args.width, args.height
    n = w * h
    st = L.MiptStats()
    o = rrt.make_options(w, h, 1, 1, traversal=L.TRAVERSAL_CULLED, cull_margin=L.CULL_MARGIN_SAFE)
    table = np.ascontiguousarray(np.asarray(scene.camera.uniform, dtype=L.CAMERA).reshape(1))
    out_t, out_x, out_p = (torch.empty(n * 3, dtype=torch.float32, device=dev) for _ in range(3))
    prim = torch.empty(n, dtype=torch.int32, device=dev)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        k = call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), k

    def motion(out, prev):
        b = L.MiptMotionBuffers()
        b.prev_position = out.data_ptr()
        if prev is not None:
            b.prev_tris, b.n_prev_tris = prev.data_ptr(), n_tris
        L.check(lib.mipt_render_motion_device(handle, L.ptr(table), 1, C.byref(o), C.byref(b), sp, C.byref(st)), "mipt_render_motion_device")
        return st.kernel_ms

    def features(want_prim=False):
        b = L.MiptFeatureBuffers()
        b.position = out_p.data_ptr()
        if want_prim:
            b.prim = prim.data_ptr()
        L.check(lib.mipt_render_features_device(handle, L.ptr(table), 1, C.byref(o), C.byref(b), sp, C.byref(st)), "mipt_render_features_device")
        return st.kernel_ms

    cells = (("motion_tracked", lambda: motion(out_t, None)), ("motion_explicit", lambda: motion(out_x, d_prev)), ("features_position_only", features))
    for _ in range(args.warmup):
        for _, call in cells:
            call()
    ms = {name: ([], []) for name, _ in cells}
    for _ in range(args.reps):                                       # the cells alternate inside every repetition
        for name, call in cells:
            t, k = timed(call)
            ms[name][0].append(t)
            ms[name][1].append(k)
    features(want_prim=True)
    torch.cuda.synchronize()
    hit = int((prim != -1).sum().item())
    same = bool(torch.equal(out_t.view(torch.int32), out_x.view(torch.int32)))
    moved = float((out_t - out_p).abs().max().item())

    # ---- what tracking adds to an update: the same REFITs on the tracked and on the untracked scene, alternating ----
    d_pos = torch.from_numpy(scene.mesh["positions"]).to(dev)
    inf = L.MiptUpdateInfo()
    it = iter(range(10 ** 6))

    def xf():
        L.check(lib.mipt_scene_set_transforms(handle, L.ptr(poses[2 + next(it) % 2]), n_parts, L.UPDATE_REFIT, C.byref(inf)), "mipt_scene_set_transforms")

    def pos():
        L.check(lib.mipt_scene_update_mesh_device(handle, d_pos.data_ptr(), None, None, L.UPDATE_REFIT, sp, C.byref(inf)), "mipt_scene_update_mesh_device")

    upd = {k: [] for k in ("set_transforms_tracked", "set_transforms_untracked", "update_positions_tracked", "update_positions_untracked")}
    for rep in range(args.warmup + args.reps):
        for on in (True, False):
            scene.track_motion(on)
            torch.cuda.synchronize()
            for name, call in (("set_transforms", xf), ("update_positions", pos)):
                t, _ = timed(call)
                if rep >= args.warmup:
                    upd[f"{name}_{'tracked' if on else 'untracked'}"].append(t)

    out = {"scene": dict(n_tris=n_tris, n_parts=n_parts, n_positions=int(plain["n_positions"]), hbm_bytes=int(plain["hbm_bytes"]),
                         hbm_bytes_tracked=int(tracked_info["hbm_bytes"]), tracking_bytes=int(tracked_info["hbm_bytes"] - plain["hbm_bytes"])),
           "config": dict(frame=f"{w}x{h}", samples=1, seed_mode="pixel_stream", traversal="culled", cull_margin=L.CULL_MARGIN_SAFE, warmup=args.warmup,
                          reps=args.reps, device=torch.cuda.get_device_name(0), timing="HIP events around the whole call"),
           "hit_pixels": hit, "pixels": n, "tracked_equals_explicit": same, "largest_motion": round(moved, 6),
           "gathered_bytes_per_hit_pixel": dict(
               motion_explicit="4 (tri_order) + 3 x 12 at 112 T + 32 c: three 32-B sectors of one or two 128-B lines",
               motion_tracked=f"4 (tri_order) + 4 x {max(1, int(np.ceil(np.log2(max(n_parts, 2)))))} (first_tri, bisection over {n_parts} parts of 96 B) + 12 (three indices, one "
                              "run) + 3 x 12 (positions, three sectors anywhere) + 52 (matrix columns and has_xf of one part)",
               features_position_only="0")}
    for name, _ in cells:
        out[name] = dict(cell(*ms[name]), store_bytes_per_pixel=12)
    base = out["features_position_only"]
    for key in ("motion_tracked", "motion_explicit"):
        out[key]["over_features_position_only"] = round(out[key]["call_ms_median"] / base["call_ms_median"], 3)
        out[key]["kernel_over_features_position_only"] = round(out[key]["kernel_ms_median"] / base["kernel_ms_median"], 3)
    for k, v in upd.items():
        out[k] = cell(v)
    for k in ("set_transforms", "update_positions"):
        out[f"{k}_tracked"]["over_untracked"] = round(out[f"{k}_tracked"]["call_ms_median"] / out[f"{k}_untracked"]["call_ms_median"], 3)
    for key in [name for name, _ in cells] + sorted(upd):
        print(key, json.dumps(out[key]), flush=True)
    print(f"tracked == explicit: {same}; {hit} of {n} pixels hit; largest |prev_position - position| {moved:.6f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    scene.release()
    if not same:
        sys.exit("the tracked and the explicit source disagree")


if __name__ == "__main__":
    main()
