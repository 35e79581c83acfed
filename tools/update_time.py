"""GPU box: what an update of a resident scene costs against making the scene, at config M (10 M triangles, synth atrium).

    python tools/update_time.py [--tris N] [--reps R]

Times five operations, each in a child process of its own under `timeout -k` (the scene is synthesised once and handed over as a
.npy file): mipt_scene_create_from_triangles; REFIT through the host entry and through the device entry (triangles in a torch tensor
in HBM); REBUILD through both entries.  Per operation: the host clock of every call and MiptSceneInfo / MiptUpdateInfo of the last;
the first REFIT of a tree also builds the refit plan (reported separately).  Stops at the first child that fails.  Not part of bench.py."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS = ("create", "refit_host", "refit_device", "rebuild_host", "rebuild_device")


def child(op, path, reps):
    import torch
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth
    tris = np.load(path)
    _, mats, texs, _ = synth.atrium_scene(n_target=1000, tex_size=1024)
    lib = rrt.load()
    times, extra = [], {}
    if op == "create":
        for _ in range(reps):
            sc = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
            t0 = time.perf_counter()
            sc.upload_from_triangles(0)
            times.append((time.perf_counter() - t0) * 1e3)
            extra = {k: v for k, v in sc.info().items() if k.endswith("_ms")}
            sc.release()
    else:
        sc = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
        h = sc.upload_from_triangles(0)
        mode = L.UPDATE_REFIT if op.startswith("refit") else L.UPDATE_REBUILD
        new = tris.copy()
        rng = np.random.default_rng(1)
        new["vertices"]["position"] += rng.normal(0, 1e-3, new["vertices"]["position"].shape).astype(np.float32)
        d_new = torch.from_numpy(new.view(np.uint8)).to("cuda:0") if op.endswith("device") else None
        stream = torch.cuda.current_stream().cuda_stream
        inf = L.MiptUpdateInfo()
        for i in range(reps + 1):
            t0 = time.perf_counter()
            if d_new is None:
                rc = lib.mipt_scene_update_triangles(h, L.ptr(new), len(new), mode, C.byref(inf))
            else:
                rc = lib.mipt_scene_update_triangles_device(h, d_new.data_ptr(), len(new), mode, stream, C.byref(inf))
            dt = (time.perf_counter() - t0) * 1e3
            if rc:
                raise RuntimeError(f"{op}: status {rc}: {lib.mipt_last_error().decode()}")
            if i == 0 and mode == L.UPDATE_REFIT:
                extra["first_call_ms_with_plan"] = dt
            else:
                times.append(dt)
        extra.update(inf.as_dict())
        sc.release()
    times = times[-reps:]
    print(json.dumps({"op": op, "n_tris": int(len(tris)), "ms": [round(t, 2) for t in times], "median_ms": round(float(np.median(times)), 2),
                      **{k: (round(v, 2) if isinstance(v, float) else v) for k, v in extra.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tris", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per operation")
    ap.add_argument("--op", choices=OPS)
    ap.add_argument("--scene")
    a = ap.parse_args()
    if a.op:
        child(a.op, a.scene, a.reps)
        return
    from rust_ray_tracing_amd import synth
    tris, _, _, _ = synth.atrium_scene(n_target=a.tris, tex_size=1024)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "tris.npy")
        np.save(path, tris)
        del tris
        for op in OPS:
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--op", op, "--scene", path, "--reps", str(a.reps)]
            r = subprocess.run(cmd)
            if r.returncode != 0:
                print(f"{op}: exit status {r.returncode}; stopping", flush=True)
                sys.exit(1)


if __name__ == "__main__":
    main()
