"""CPU: the ray-query model (tests/tools/query_model.py) is held to the oracle's own traversal.  Every ray orc_debug_pixel records
for a few dozen pixels -- camera rays and scatter rays that start on a surface -- goes through the model with t_max = 1e30, which is
the reference call itself: the model must return the recorded triangle and t bit for bit, misses included."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import query_model as Q  # noqa: E402

W, H = 64, 48


def _scene(rrt, kind):
    from rust_ray_tracing_amd import synth
    kw = dict(n_target=2000, tex_size=32) if kind == "helmet" else {}
    tris, mats, texs, cam = synth.make_scene(kind, **kw)
    sc = rrt.Scene.from_arrays(tris, mats, texs)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    return sc


@pytest.mark.parametrize("kind", ["cornell", "helmet"])
def test_model_reproduces_every_ray_the_oracle_traces(rrt, orc, kind):
    sc = _scene(rrt, kind)
    if kind == "helmet":
        assert 1500 <= len(sc.tris) <= 2500
    pixels = np.linspace(0, W * H - 1, 40).astype(np.int64)               # a few dozen pixels spread over the frame
    rays, rec_tri, rec_t = Q.oracle_path_rays(orc, sc, W, H, pixels, spp=2, depth=8)
    assert len(rays) >= 2 * len(pixels)                                   # at least the camera rays
    assert np.any(rec_tri == Q.NONE) and np.any(rec_tri != Q.NONE)        # both hits and misses are in the set
    cam = np.asarray(sc.camera.uniform["position"], dtype=np.float32)
    assert np.any((rays["origin"] != cam).any(axis=1)), "no scatter rays recorded"
    hits, occ, counters = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays)
    hit = rec_tri != Q.NONE
    assert np.array_equal(occ != 0, hit)
    assert np.array_equal(hits["prim"][hit] & 0x01FFFFFF, rec_tri[hit])
    assert np.all(hits["prim"][~hit] == Q.NONE)
    assert Q.same_bits(hits["t"], rec_t)                                  # a miss records HitInfo::default's 1e30
    assert np.all(hits["u"][~hit] == 0) and np.all(hits["v"][~hit] == 0)
    assert counters["rays"] == len(rays) and counters["hits"] == int(hit.sum())
    # the culled arm with the safe margin finds the same hits on these scenes (include/mipt.h, MIPT_CULL_MARGIN_SAFE) in fewer steps
    chits, _, ccounters = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays, cull=True, margin=0.0078125)
    assert Q.same_bits(chits, hits)
    assert ccounters["inner_steps"] <= counters["inner_steps"] and ccounters["tri_tests"] <= counters["tri_tests"]


def test_model_t_max_and_occlusion(rrt, orc):
    """t_max cuts strictly (t < t_max), and the occlusion query is `closest.t < t_max` in the reference arm with no more work
    than the closest-hit query."""
    sc = _scene(rrt, "cornell")
    rays, rec_tri, rec_t = Q.oracle_path_rays(orc, sc, W, H, np.linspace(0, W * H - 1, 12).astype(np.int64), spp=1, depth=4)
    hit = rec_tri != Q.NONE
    rays, rec_t = rays[hit], rec_t[hit]
    lib = orc.load()
    for name, t_max, expect in (("at t", rec_t, False), ("one ulp above", np.nextafter(rec_t, np.float32(np.inf)), True),
                                ("one ulp below", np.nextafter(rec_t, np.float32(0)), False)):
        r = rays.copy()
        r["t_max"] = t_max
        hits, occ, c = Q.query(lib, sc.tris, sc.bvh_nodes, r)
        assert np.all((occ != 0) == expect), name
        _, occ2, c2 = Q.query(lib, sc.tris, sc.bvh_nodes, r, anyhit=True)
        assert np.array_equal(occ2, occ), name
        assert c2["tri_tests"] <= c["tri_tests"] and c2["inner_steps"] <= c["inner_steps"]
        if expect:
            assert Q.same_bits(hits["t"], rec_t)
