"""The model of mipt_query_radiance (include/mipt.h "radiance queries") for tests/test_gpu_radiance.py and
tests/test_cpp_host_radiance.py: a Python loop over the oracle's one-ray entries -- orc_trace_ray_m (shading 0) and
orc_trace_ray_wgsl_m (shading 1), which take the cull margin and return the counters -- with one rng word carried across a ray's
samples and the f32 sum and divide done in numpy.  Nothing of the library under test is used here."""
import ctypes as C

import numpy as np

RAY = np.dtype([("origin", "<f4", 3), ("t_max", "<f4"), ("direction", "<f4", 3), ("reserved", "<u4")])   # reserved: the ray's seed
COUNTERS = ("rays", "inner_steps", "tri_tests", "hits", "texel_fetches")                                  # orc_trace_ray_wgsl's counters_out
_F3 = C.c_float * 3


def default_seeds(n, first=0):
    """cpu.rs:28-29 for i = first ... first + n - 1, 1 in place of 0 -- in Python integers"""
    return np.array([(987612486 * (i + 87636354)) % (1 << 32) or 1 for i in range(first, first + n)], dtype=np.uint32)


def make_rays(tris, n, seed, seeds=None):
    """n rays made from `seed` alone: origins in turn ON a triangle, JUST OFF one (1e-3 along its normal, either side) and
    anywhere INSIDE the scene's box; directions over the whole sphere, not normalised, lengths 0.25 ... 4; the seed word from
    `seeds` (default: default_seeds).  t_max is 0: the entry ignores it."""
    rng = np.random.default_rng(seed)
    P = np.asarray(tris["vertices"]["position"], dtype=np.float64)
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    d = rng.normal(size=(n, 3))
    d *= (rng.uniform(0.25, 4.0, n) / np.linalg.norm(d, axis=1))[:, None]
    t = rng.integers(0, len(P), n)
    b = rng.dirichlet((1.0, 1.0, 1.0), n)
    on = (P[t] * b[:, :, None]).sum(1)
    nrm = np.cross(P[t, 1] - P[t, 0], P[t, 2] - P[t, 0])
    ln = np.linalg.norm(nrm, axis=1)
    nrm = nrm / np.where(ln > 0, ln, 1.0)[:, None]
    off = on + nrm * (1e-3 * rng.choice([-1.0, 1.0], n))[:, None]
    box = rng.uniform(lo, hi, (n, 3))
    kind = np.arange(n) % 3
    o = np.where((kind == 0)[:, None], on, np.where((kind == 1)[:, None], off, box))
    r = np.zeros(n, dtype=RAY)
    r["origin"], r["direction"] = o.astype(np.float32), d.astype(np.float32)
    r["reserved"] = default_seeds(n) if seeds is None else np.asarray(seeds, dtype=np.uint32)
    return r


class Model:
    """The scene as the oracle takes it, kept alive for the calls"""

    def __init__(self, orc, sc):
        self.orc, self.lib = orc, orc.load()
        self.tris, self.nodes = np.ascontiguousarray(sc.tris), np.ascontiguousarray(sc.bvh_nodes)
        self.mats = np.ascontiguousarray(sc.materials_array())
        self.texs = [np.ascontiguousarray(t) for t in sc.textures]
        self.tex_array = orc._tex_array(self.texs)

    def trace(self, rays, samples, depth, shading=0, cull=0, margin=0.0):
        """-> dict: "sum" [n, 3] f32 (the samples added in order from +0), "mean" [n, 3] f32 (sum / f32(samples)), "state" [n] u32
        (the stream after the last sample) and "counters" [n, 5] int64 in the order of COUNTERS.  margin: the culled traversal's
        cull_margin (MiptRadianceOptions), ignored by the reference traversal."""
        lib, n = self.lib, len(rays)
        args = (self.tris.ctypes.data, self.tris.nbytes // 112, self.nodes.ctypes.data, self.nodes.nbytes // 32, self.mats.ctypes.data,
                self.mats.nbytes // 80, self.tex_array, len(self.texs))
        total = np.zeros((n, 3), dtype=np.float32)
        state = np.zeros(n, dtype=np.uint32)
        counters = np.zeros((n, 5), dtype=np.int64)
        out, cnt = _F3(), (C.c_uint64 * 5)()
        entry = lib.orc_trace_ray_m if shading == 0 else lib.orc_trace_ray_wgsl_m
        for i in range(n):
            o, d = _F3(*[float(x) for x in rays["origin"][i]]), _F3(*[float(x) for x in rays["direction"][i]])
            st = C.c_uint32(int(rays["reserved"][i]))
            acc = np.zeros(3, dtype=np.float32)
            for _ in range(samples):
                entry(*args, C.byref(o), C.byref(d), depth, C.byref(st), cull, C.c_float(margin), self.orc.LIBM_GLIBC235, C.byref(out), C.byref(cnt))
                counters[i] += np.array(list(cnt), dtype=np.int64)
                acc = acc + np.array(list(out), dtype=np.float32)                   # f32 + f32, rounded once
            total[i], state[i] = acc, st.value
        return dict(sum=total, mean=total / np.float32(samples), state=state, counters=counters)

    def first_hits(self, rays):
        """bool [n]: the ray's first segment hits a triangle (un-culled traversal; the wgsl entry counts it, whatever the seed)"""
        return self.trace(rays, 1, 1, shading=1)["counters"][:, 3] > 0


def conditions(model_out, first_hit):
    """What every scene-backed case asserts of the MODEL's output before anything is compared with it"""
    for k in ("sum", "mean"):
        assert not np.any(np.isnan(model_out[k])), k
    n = len(first_hit)
    assert 4 * int(first_hit.sum()) >= n, (int(first_hit.sum()), n)                 # at least a quarter hit on their first segment
    assert 10 * int((~first_hit).sum()) >= n, (int((~first_hit).sum()), n)          # at least a tenth miss


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
