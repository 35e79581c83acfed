"""The model of the previous-position pass (include/mipt.h "previous positions"), in Python over the HOST arrays of a Scene.  Nothing
comes from the library under test:

* the camera ray is features_model.camera_rays (the first record orc_debug_pixel writes for the sample number, 0 -> 1);
* the hit is query_model.traverse (Ray::traverse_bvh over orc_intersect_node / orc_intersect_tri, either arm), and its u and v are
  out[2] and out[3] of orc_intersect_tri on the winner;
* the previous corners come from a triangle array in the caller's order -- for the tracked source mesh_model.expand of the previous
  generation;
* the interpolation is numpy float32: w = (1 - u) - v, prev = ((P0*w) + (P1*u)) + (P2*v).

tests/test_motion_model.py holds the definition to the oracle geometrically; tests/test_gpu_motion.py holds the kernel to this model."""
import numpy as np

import features_model as F
import query_model as Q

F32 = np.float32


def interpolate(corners, u, v):
    """corners [..., 3, 3] (corner, component), u / v [...] float32 -> [..., 3]"""
    corners = np.asarray(corners, dtype=F32)
    u, v = np.asarray(u, dtype=F32)[..., None], np.asarray(v, dtype=F32)[..., None]
    with np.errstate(all="ignore"):
        w = (F32(1.0) - u) - v
        return ((corners[..., 0, :] * w) + (corners[..., 1, :] * u)) + (corners[..., 2, :] * v)


def hits(orc, sc, rays, cull=False, margin=0.0, tri_order=None):
    """every ray -> (T [n] uint32 in the caller's order, NONE = miss; u [n], v [n] float32; t [n] float32)"""
    lib = orc.load()
    tris, nodes = np.ascontiguousarray(sc.tris), np.ascontiguousarray(sc.bvh_nodes)
    n = len(rays)
    T = np.full(n, Q.NONE, dtype=np.uint32)
    tuv = np.zeros((n, 3), dtype=np.uint32)
    for i in range(n):
        t, u, v, tri, _ = Q.traverse(lib, tris, nodes, rays[i], cull, margin)
        tuv[i] = (t, u, v)
        if tri != Q.NONE:
            T[i] = tri if tri_order is None else tri_order[tri]
    f = tuv.view(F32)
    return T, f[:, 1].copy(), f[:, 2].copy(), f[:, 0].copy()


def from_hits(T, u, v, prev_tris):
    """[n,3] float32: the definition's value for hits found earlier; a miss is (0, 0, 0)"""
    prev_tris = np.ascontiguousarray(prev_tris)
    words = prev_tris.view(F32).reshape(len(prev_tris), 28)
    out = np.zeros((len(T), 3), dtype=F32)
    hit = T != Q.NONE
    t = T[hit].astype(np.int64)
    corners = np.stack([words[t, 0:3], words[t, 8:11], words[t, 16:19]], axis=1)
    out[hit] = interpolate(corners, u[hit], v[hit])
    return out


def frame(orc, sc, camera, width, height, seed_mode, prev_tris, sample_begin=0, cull=False, margin=0.0, tri_order=None, rays=None):
    """What mipt_render_motion writes for one view -> [H,W,3] float32.  `sc`: a Scene whose tris / bvh_nodes are the tree's; `tri_order`
    maps the tree's order to the caller's, the order of `prev_tris` (None: they are the same).  `rays`: a dict that keeps the camera
    rays of a sample number between calls."""
    s0 = sample_begin if sample_begin else 1
    rays = {} if rays is None else rays
    if s0 not in rays:
        rays[s0] = F.camera_rays(orc, sc, camera, width, height, seed_mode, s0)
    T, u, v, _ = hits(orc, sc, rays[s0][0], cull, margin, tri_order)
    return from_hits(T, u, v, prev_tris).reshape(height, width, 3)


same_bits = F.same_bits


def same_but_nan(a, b):
    """equal bits, except that where one is a NaN the other must be one too (the NaN rule: sign and payload are free)"""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
