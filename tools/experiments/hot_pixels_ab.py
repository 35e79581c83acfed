"""GPU box: the hot pixels on config M -- kernel build variants interleaved in ONE process (scene generated and BVH built once), and the
premise behind them from the frame's real per-pixel costs.

    python tools/experiments/hot_pixels_ab.py [--reps R] [--rounds N] [--sim-lib NAME] parent.so head.so variant.so ...

Every library is loaded privately and gets its own scene replica.  Per round and library: the first frame, then `reps` frames of the
same view (kernel ms and the wall time of the render call, min / median / max, frame CRC); then a camera turning by 0.5 and by 2 degrees
per frame, and a re-render with per-sample seeds.  Last, the per-pixel costs, the tile order and the hot list are read from the handle
of --sim-lib through libmipt_diag.so (so the tree's own libraries must be built from the same source as that library) and a list
scheduling of those costs over --lanes resident lanes -- a lane takes the next pixel of the queue when it is free and is busy for the
pixel's rays -- gives, for the plain order, the tile order and the hot list, the makespan against the ideal, the idle share and when
the 1 000 most expensive pixels start; the same for the list behind the hot pixels cut at 1/2, 3/4 and all of the local slots (read
through mipt_diag_scene_list, so --sim-lib must be a build whose list is complete).  Variants with another H or another list length:
    make -C rust_ray_tracing_amd/csrc variant NAME=hot_q EXTRA="-DMIPT_HOT_LANES_NUM=1 -DMIPT_HOT_LANES_DEN=4"      (0 / 1 = no hot list)
    make -C rust_ray_tracing_amd/csrc variant NAME=list_half EXTRA="-DMIPT_LIST_NUM=1 -DMIPT_LIST_DEN=2"          (0 / 1 = the hot list alone)
"""
import argparse, ctypes as C, os, sys, time, zlib, json, heapq
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import rust_ray_tracing_amd as rrt
from rust_ray_tracing_amd import synth, _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--tris", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--extra", type=int, default=1, help="camera-turn and per-sample-seed series")
ap.add_argument("--sim-lib", default="", help="file name of the library whose handle feeds the list-scheduling simulation (empty = none)")
ap.add_argument("--lanes", type=int, default=256 * 5 * 256, help="resident lanes of the simulated launch: CUs x blocks per CU x 256 (MI355X, culled: 327 680)")
ap.add_argument("--out", default="", help="write the figures to this JSON file too")
ap.add_argument("libs", nargs="+")
args = ap.parse_args()
t0 = time.time()
tris, mats, texs, cam = synth.atrium_scene(n_target=args.tris, tex_size=1024)
sc = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
del tris
sc.build_bvh_device(0)
print(f"scene ready {time.time() - t0:.1f} s", flush=True)
w, h, spp, depth = 1920, 1080, 8, 64
buf = np.zeros(w * h * 3, dtype=np.float32)
desc = sc.desc()
vp = C.c_void_p
libs = {}
for path in args.libs:
    lib = C.CDLL(os.path.abspath(path), mode=C.RTLD_LOCAL)
    lib.mipt_scene_create.argtypes = [C.POINTER(L.MiptSceneDesc), C.c_int, C.POINTER(vp)]
    lib.mipt_render.argtypes = [vp, vp, C.POINTER(L.MiptOptions), vp, vp, C.POINTER(L.MiptStats)]
    lib.mipt_scene_destroy.argtypes = [vp]
    lib.mipt_last_error.restype = C.c_char_p
    hnd = vp()
    assert lib.mipt_scene_create(C.byref(desc), 0, C.byref(hnd)) == 0, lib.mipt_last_error()
    libs[os.path.basename(path)] = (lib, hnd)
print(f"handles ready {time.time() - t0:.1f} s", flush=True)

def frame(name, camera, seed_mode=0):
    lib, hnd = libs[name]
    o = rrt.make_options(w, h, spp, depth, seed_mode=seed_mode, traversal=1)
    st = L.MiptStats()
    t = time.perf_counter()
    rc = lib.mipt_render(hnd, L.ptr(camera.uniform), C.byref(o), L.ptr(buf), None, C.byref(st))
    wall = (time.perf_counter() - t) * 1e3
    assert rc == 0, lib.mipt_last_error()
    return st.kernel_ms, wall

def mkcam(yaw_add=0.0):
    c = rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2] + yaw_add)
    c.update_view()
    return c

def summ(ts):
    s = sorted(ts)
    return {"min": round(s[0], 3), "median": round(s[len(s) // 2], 3), "max": round(s[-1], 3), "n": len(s)}

base = mkcam()
res = {}
for rnd in range(args.rounds):
    for name in libs:
        ks, ws = [], []
        for rep in range(args.reps + 1):
            k, wl = frame(name, base)
            if rep == 0:
                res.setdefault(name, {})[f"round{rnd}_first_frame"] = round(k, 3)
                crc = zlib.crc32(buf.tobytes())
            else:
                ks.append(k); ws.append(wl)
        res[name][f"round{rnd}_kernel"] = summ(ks)
        res[name][f"round{rnd}_wall_render_call"] = summ(ws)
        res[name]["crc"] = f"{crc:08x}"
        assert zlib.crc32(buf.tobytes()) == crc
        print(name, rnd, res[name][f"round{rnd}_first_frame"], res[name][f"round{rnd}_kernel"], "wall", res[name][f"round{rnd}_wall_render_call"], res[name]["crc"], flush=True)
if args.extra:
    for deg in (0.5, 2.0):
        for name in libs:
            ks = [frame(name, mkcam(deg * (i + 1)))[0] for i in range(8)]
            res[name][f"turn_{deg}_deg_per_frame"] = summ(ks)
            print(name, "turn", deg, summ(ks), flush=True)
    for name in libs:
        ks = [frame(name, base, seed_mode=1)[0] for i in range(9)]
        res[name]["per_sample_seed_first"] = round(ks[0], 3)
        res[name]["per_sample_seed_rerender"] = summ(ks[1:])
        print(name, "seed_mode 1 first", ks[0], "re-render", summ(ks[1:]), flush=True)
    for name in libs:       # back on the base view for the simulation below
        frame(name, base); frame(name, base)
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)

if args.sim_lib:
    # premise: when do the heavy pixels start under the tile order?  list scheduling of the real per-pixel costs over the resident lanes
    hnd = libs[args.sim_lib][1]
    diag = rrt.load_diag()
    info = (C.c_uint32 * 3)()
    assert diag.mipt_diag_scene_hot_pixels(hnd, None, 0, None, 0, C.byref(info)) == 0
    n, nh = int(info[0]), int(info[1])
    pc, hot = np.zeros(n, dtype=np.uint32), np.zeros(max(nh, 1), dtype=np.uint32)
    assert diag.mipt_diag_scene_hot_pixels(hnd, pc.ctypes.data, n, hot.ctypes.data, nh, C.byref(info)) == 0
    nt = n // 64
    tc, order = np.zeros(nt, dtype=np.uint32), np.zeros(nt, dtype=np.uint32)
    assert diag.mipt_diag_scene_tile_order(hnd, tc.ctypes.data, order.ctypes.data, nt, C.byref(info)) == 0
    real = pc > 0
    mean = pc[real].mean()
    print(f"slots {n} H {nh}; pixels {real.sum()} rays {pc.sum()} mean {mean:.1f} max {pc.max()} ({pc.max() / mean:.2f}x); >2.5x mean: {(pc > 2.5 * mean).sum()}, >3.5x: {(pc > 3.5 * mean).sum()}")
    lanes = args.lanes
    def simulate(seq, label):
        costs = pc[seq].astype(np.int64)
        keep = costs > 0
        seq, costs = seq[keep], costs[keep]
        heap = [0] * lanes
        start = np.zeros(len(seq), dtype=np.int64)
        for i, c in enumerate(costs.tolist()):
            t = heapq.heappop(heap)
            start[i] = t
            heapq.heappush(heap, t + c)
        end = max(heap); ideal = costs.sum() / lanes
        first_idle = min(heap)
        top = np.argsort(-costs, kind="stable")[:1000]
        hist = np.histogram(start[top] / end, bins=[0, 0.1, 0.25, 0.5, 0.75, 1.0])[0]
        tail = sum(end - x for x in heap) / (end * lanes)
        print(f"{label}: makespan {end} ray-steps, ideal {ideal:.0f} ({end / ideal:.3f}x), idle share {tail:.4f}, first lane idle at {first_idle / end:.3f}; "
              f"start of the 1000 heaviest pixels in [0,.1) [.1,.25) [.25,.5) [.5,.75) [.75,1]: {hist.tolist()}; latest heavy start {start[top].max() / end:.3f}")
    plain = np.arange(n)
    ordered = (order.astype(np.int64)[:, None] * 64 + np.arange(64)[None, :]).reshape(-1)
    hotset = np.zeros(n, dtype=bool); hotset[hot[:nh]] = True
    with_hot = np.concatenate([hot[:nh].astype(np.int64), ordered[~hotset[ordered]]])
    simulate(plain, "plain order")
    simulate(ordered, "tile order")
    simulate(with_hot, "hot list + tile order")
    li = (C.c_uint32 * 2)()
    assert diag.mipt_diag_scene_list(hnd, None, 0, C.byref(li)) == 0
    full = np.zeros(max(int(li[0]), 1), dtype=np.uint32)
    assert diag.mipt_diag_scene_list(hnd, full.ctypes.data, int(li[0]), C.byref(li)) == 0
    print(f"list: {li[0]} entries, the last launch took {li[1]}")
    if int(li[0]) == n:
        for num, den in ((1, 2), (3, 4), (1, 1)):
            m = max(nh, n * num // den)
            inlist = np.zeros(n, dtype=bool); inlist[full[:m]] = True
            simulate(np.concatenate([full[:m].astype(np.int64), ordered[~inlist[ordered]]]), f"list of {num}/{den} of the slots + tile order")
for lib, hnd in libs.values():
    lib.mipt_scene_destroy(hnd)
print(f"done {time.time() - t0:.1f} s", flush=True)
