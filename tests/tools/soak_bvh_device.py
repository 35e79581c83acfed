"""GPU box: device BVH builder vs host builder on many random triangle soups (sizes across every builder class, with ties,
identical centroids, flat and degenerate triangles, boxes whose area overflows -- the distributions are bvh_corpus.soup / apply_mode, the ones
tests/test_gpu_bvh_corpus.py places at exact sizes).  Prints the number of soups whose node array or triangle order differs; must be 0."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import bvh_corpus
import rust_ray_tracing_amd as rrt
from rust_ray_tracing_amd import TRIANGLE
rng = np.random.default_rng(int(os.environ.get("SOAK_SEED", "7")))
n_iter = int(sys.argv[1]) if len(sys.argv) > 1 else 300
bad = 0
tot = 0
for it in range(n_iter):
    kind = it % 6
    n = int(rng.integers(1, 600)) if kind < 2 else int(rng.integers(600, 9000)) if kind < 4 else int(rng.integers(9000, 120000))
    scale = float(rng.choice([1e-3, 1.0, 1e3]))
    if it % 10 == 9: scale = 1e19                                              # surface areas overflow: no plane is usable, the split falls back to 0.0 on axis 0
    spread = float(rng.choice([0.05, 1.0, 20.0]))
    mode = it % 5
    p = bvh_corpus.apply_mode(rng, bvh_corpus.soup(rng, n, scale, spread), mode, scale)
    t = np.zeros(n, dtype=TRIANGLE)
    t["vertices"]["position"] = p.astype(np.float32)
    host = rrt.Scene.from_arrays(t, [rrt.material_default()])
    dev = rrt.Scene.from_arrays(t, [rrt.material_default()], build_bvh=False)
    dev.build_bvh_device(0)
    a, b = host.bvh_nodes.copy(), dev.bvh_nodes.copy()
    for k in ("bounds_min", "bounds_max"):
        a[k] += np.float32(0); b[k] += np.float32(0)
    same = dev.tris.tobytes() == host.tris.tobytes() and a.tobytes() == b.tobytes()
    tot += n
    if not same:
        bad += 1
        print("MISMATCH soup", it, "n", n, "mode", mode, flush=True)
    if it % 50 == 49: print(it + 1, "soups,", tot, "triangles, mismatching", bad, flush=True)
print("soups", n_iter, "triangles", tot, "mismatching", bad)
