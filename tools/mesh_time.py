"""GPU box: what a resident indexed mesh costs and saves against fat triangles, at config M (10 M triangles, synth atrium).

    python tools/mesh_time.py [--tris N] [--reps R] [--parts P] [--out FILE]

The bench scene is turned into a mesh by tests/tools/mesh_model.py mesh_from_triangles(tris, P) (the part count it yields is
reported).  One process, one warm-up then the median of R, host clock of the whole call plus the MiptSceneInfo / MiptUpdateInfo split:
  (a) mipt_scene_create_from_triangles from host fat triangles  vs  mipt_scene_create_from_mesh, with the bytes each sends over PCIe;
  (b) the host entry mipt_scene_update_triangles with triangles expanded beforehand (expansion not charged)  vs
      mipt_scene_set_transforms, REFIT and REBUILD;
  (c) mipt_scene_update_triangles_device  vs  mipt_scene_update_mesh_device(transforms only), REFIT: the difference is the expansion;
      the expansion's HIP-event time (difference of the two build_ms) and a device-to-device copy of the expanded array timed in the
      same run as the memory-bound yardstick.
Prints one JSON line per measurement and a summary; --out writes all of them to a file.  Not part of bench.py."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parts", type=int, default=64)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    import mesh_model
    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth
    lib = rrt.load()
    results = []

    def emit(**kw):
        kw = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in kw.items()}
        results.append(kw)
        print(json.dumps(kw), flush=True)

    def timed(fn, before=None):
        ms, last = [], None
        for i in range(a.reps + 1):
            if before:
                before()                                           # e.g. destroying the previous scene: not charged
            t0 = time.perf_counter()
            last = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if i:
                ms.append(dt)
        return float(np.median(ms)), [round(x, 2) for x in ms], last

    t0 = time.perf_counter()
    tris, mats, texs, _ = synth.atrium_scene(n_target=a.tris, tex_size=1024)
    mesh, perm = mesh_model.mesh_from_triangles(tris, a.parts)
    tris = np.ascontiguousarray(tris[perm])
    n_parts = len(mesh["parts"])
    mesh_bytes = sum(v.nbytes for v in mesh.values() if v is not None)
    emit(op="scene", n_tris=len(tris), n_parts=n_parts, n_positions=len(mesh["positions"]), n_normals=len(mesh["normals"]),
         n_tex_coords=len(mesh["tex_coords"]), fat_bytes=int(tris.nbytes), mesh_bytes=int(mesh_bytes), prepare_s=time.perf_counter() - t0)

    rng = np.random.default_rng(1)
    def pose(k):
        m = np.zeros((n_parts, 4, 4), dtype=np.float32)
        m[:, 0, 0] = m[:, 1, 1] = m[:, 2, 2] = m[:, 3, 3] = 1.0
        m[:, 3, :3] = rng.normal(0, 1e-3 * (k + 1), (n_parts, 3))
        return m.reshape(n_parts, 16)

    # ---- (a) create ----
    plain = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    med, ms, _ = timed(lambda: plain.upload_from_triangles(0), plain.release)
    emit(op="create_from_triangles", median_ms=med, ms=ms, pcie_bytes=int(tris.nbytes), **{k: v for k, v in plain.info().items() if k.endswith("_ms")})
    msc = rrt.Scene.from_mesh(materials=mats, textures=texs, **mesh)
    med, ms, _ = timed(lambda: msc.upload_from_mesh(0), msc.release)
    emit(op="create_from_mesh", median_ms=med, ms=ms, pcie_bytes=int(mesh_bytes), **{k: v for k, v in msc.info().items() if k.endswith("_ms")},
         **{k: v for k, v in msc.mesh_info().items() if k.endswith("_bytes")})

    # ---- (b) host routes, (c) device routes ----
    poses = [pose(k) for k in range(a.reps + 1)]
    tmp = rrt.Scene()
    tmp.mesh = dict(msc.mesh)
    tmp._set_mesh_transforms(poses[0])
    moved = tmp.expand_mesh().copy()                               # expanded on the host beforehand: not charged to the host entry
    d_moved = torch.from_numpy(moved.view(np.uint8)).to("cuda:0")
    d_xf = torch.from_numpy(poses[1]).to("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    summary = {}
    for mode, mname in ((L.UPDATE_REFIT, "refit"), (L.UPDATE_REBUILD, "rebuild")):
        inf = L.MiptUpdateInfo()

        def run(call):
            rc = call()
            if rc:
                raise RuntimeError(f"status {rc}: {lib.mipt_last_error().decode()}")
            return {k: v for k, v in inf.as_dict().items() if k.endswith("_ms")}

        it = iter(range(10 ** 6))
        cases = [("update_triangles_host", plain, lambda: lib.mipt_scene_update_triangles(plain._handle, L.ptr(moved), len(moved), mode, C.byref(inf)), int(moved.nbytes)),
                 ("set_transforms", msc, lambda: lib.mipt_scene_set_transforms(msc._handle, L.ptr(poses[next(it) % len(poses)]), n_parts, mode, C.byref(inf)), n_parts * 64)]
        if mode == L.UPDATE_REFIT:
            cases += [("update_triangles_device", plain, lambda: lib.mipt_scene_update_triangles_device(plain._handle, d_moved.data_ptr(), len(moved), mode, stream, C.byref(inf)), 0),
                      ("update_mesh_device_transforms", msc, lambda: lib.mipt_scene_update_mesh_device(msc._handle, None, None, d_xf.data_ptr(), mode, stream, C.byref(inf)), 0)]
        for name, _, call, sent in cases:
            run(call)                                              # the first REFIT of a tree also makes the refit plan
            med, ms, last = timed(lambda: run(call))
            summary[f"{name}_{mname}"] = dict(median_ms=med, **last)
            emit(op=f"{name}_{mname}", median_ms=med, ms=ms, pcie_bytes=sent, **last)

    # the yardstick: a device-to-device copy of the expanded array
    dst = torch.empty_like(d_moved)
    copies = []
    for i in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(d_moved)
        e1.record()
        torch.cuda.synchronize()
        if i:
            copies.append(e0.elapsed_time(e1))
    copy_ms = float(np.median(copies))
    expand_ms = summary["update_mesh_device_transforms_refit"]["build_ms"] - summary["update_triangles_device_refit"]["build_ms"]
    host_refit, mesh_refit = summary["update_triangles_host_refit"]["median_ms"], summary["set_transforms_refit"]["median_ms"]
    emit(op="summary", n_tris=len(tris), n_parts=n_parts, expanded_bytes=int(moved.nbytes), dtod_copy_ms=copy_ms, expansion_kernel_ms=expand_ms,
         expansion_over_copy=expand_ms / copy_ms,
         expansion_call_cost_ms=summary["update_mesh_device_transforms_refit"]["median_ms"] - summary["update_triangles_device_refit"]["median_ms"],
         host_refit_ms=host_refit, mesh_refit_ms=mesh_refit, mesh_refit_is_faster=bool(mesh_refit < host_refit))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    if not mesh_refit < host_refit:
        sys.exit("the mesh REFIT is not faster than the host-entry REFIT")


if __name__ == "__main__":
    main()
