"""CPU: the geometry-update entry points of include/mipt.h (mipt_scene_update_triangles{,_device}, mipt_multi_update_triangles) --
bindings, argument checks that need no device, and the refit restatement (tests/tools/refit_model.py) against mipt_bvh_build's node
array and an independent per-node fold.  The device side is tests/test_gpu_scene_update.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import refit_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mipt_scene_update_triangles", "mipt_scene_update_triangles_device", "mipt_multi_update_triangles")


def test_bindings_and_header_agree(rrt):
    from rust_ray_tracing_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mipt.h")).read(), flags=re.S)
    for name in NEW:
        assert name in L.EXPORTS and re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(rrt.load(), name)
    assert "MIPT_UPDATE_REFIT   = 0" in text and "MIPT_UPDATE_REBUILD = 1" in text
    assert C.sizeof(L.MiptUpdateInfo) == 4 * 8 + 4 * 4
    assert (L.UPDATE_REFIT, L.UPDATE_REBUILD) == (0, 1)
    assert rrt.load().mipt_abi_version() == 4


def test_argument_errors_without_a_device(rrt):
    """null scene / null triangles / a bad mode / no triangles: MIPT_ERR_INVALID_ARG with a message, decided before any device call
    (a dummy non-null handle is never dereferenced for these)"""
    from rust_ray_tracing_amd import TRIANGLE
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    tris = np.zeros(4, dtype=TRIANGLE)
    dummy = np.zeros(64, dtype=np.uint8)                     # stands in for a handle: none of these cases may read it
    h = C.c_void_p(dummy.ctypes.data)
    for name, call in (("mipt_scene_update_triangles", lambda s, t, n, m: lib.mipt_scene_update_triangles(s, t, n, m, None)),
                       ("mipt_scene_update_triangles_device", lambda s, t, n, m: lib.mipt_scene_update_triangles_device(s, t, n, m, None, None)),
                       ("mipt_multi_update_triangles", lambda s, t, n, m: lib.mipt_multi_update_triangles(s, t, n, m, None))):
        assert call(None, L.ptr(tris), 4, 0) == L.ERR_INVALID_ARG and b"null" in lib.mipt_last_error(), name
        if name != "mipt_multi_update_triangles":             # (a multi handle is a real object: only the null check comes first)
            assert call(h, None, 4, 0) == L.ERR_INVALID_ARG and b"null" in lib.mipt_last_error(), name
            assert call(h, L.ptr(tris), 4, 2) == L.ERR_INVALID_ARG and b"mode" in lib.mipt_last_error(), name
            assert call(h, L.ptr(tris), 4, 0xFFFFFFFF) == L.ERR_INVALID_ARG, name
            assert call(h, L.ptr(tris), 0, 1) == L.ERR_INVALID_ARG and b"no triangles" in lib.mipt_last_error(), name
    assert not dummy.any()


def _soup(n, seed, degenerate=False):
    from rust_ray_tracing_amd import TRIANGLE
    rng = np.random.default_rng(seed)
    t = np.zeros(n, dtype=TRIANGLE)
    t["vertices"]["position"] = rng.uniform(-4, 4, (n, 1, 3)).astype(np.float32) + rng.normal(0, 0.3, (n, 3, 3)).astype(np.float32)
    if degenerate:
        t[n // 4: n // 2] = t[n // 4]
        t["vertices"]["position"][-(n // 8):, :, 2] = 0.0
        t["vertices"]["position"][-(n // 8):, :, 1] = -0.0
    return t


def _scenes():
    from rust_ray_tracing_amd import synth
    out = [(k, synth.make_scene(k, **kw)[0]) for k, kw in (("cornell", {}), ("helmet", dict(n_target=2000, tex_size=8)),
                                                           ("atrium", dict(n_target=5000, tex_size=8)), ("dragon", dict(n_target=5000)))]
    out += [("soup1", _soup(1, 1)), ("soup17", _soup(17, 2)), ("soup300d", _soup(300, 3, True)), ("soup4000d", _soup(4000, 4, True))]
    return out


@pytest.mark.parametrize("idx", range(8))
def test_refit_restatement(rrt, idx):
    from rust_ray_tracing_amd import host
    name, tris = _scenes()[idx]
    sc = rrt.Scene.from_arrays(tris, [rrt.material_default()])         # mipt_bvh_build: nodes + tris in tree order
    nodes = sc.bvh_nodes
    # unchanged triangles: the refit is BVH::build's own node array (sign of a zero aside)
    assert refit_model.same_nodes(refit_model.refit(nodes, sc.tris), nodes), name
    assert refit_model.same_nodes(host.refit_nodes(nodes, sc.tris), nodes), name
    # perturbed: every node equals a direct fold over its own subtree's triangles; the package's level-wise refit agrees
    rng = np.random.default_rng(idx)
    new = sc.tris.copy()
    new["vertices"]["position"] += rng.normal(0, 0.05, new["vertices"]["position"].shape).astype(np.float32)
    new["vertices"]["position"][: len(new) // 3] *= np.float32(2.0)
    got = refit_model.refit(nodes, new)
    assert np.array_equal(got["first_tri_or_child"], nodes["first_tri_or_child"]) and np.array_equal(got["num_tris"], nodes["num_tris"])
    which = range(len(nodes)) if len(nodes) < 600 else np.random.default_rng(7).choice(len(nodes), 600, replace=False)
    mn, mx = refit_model.per_node_fold(nodes, new, which)
    assert np.array_equal(mn, got["bounds_min"][list(which)]) and np.array_equal(mx, got["bounds_max"][list(which)]), name
    assert refit_model.same_nodes(host.refit_nodes(nodes, new), got), name
    if len(new) > 1:
        assert not refit_model.same_nodes(got, nodes)


def test_refit_ignores_nan_like_f32_min():
    """f32::min / f32::max (bvh.rs:185-193) return the other operand for a NaN: a NaN coordinate does not reach a bound"""
    from rust_ray_tracing_amd import NODE, TRIANGLE
    t = np.zeros(2, dtype=TRIANGLE)
    t["vertices"]["position"][0] = [[0, 0, 0], [1, 1, 1], [2, 0, 1]]
    t["vertices"]["position"][1] = [[np.nan, 5, 0], [1, 1, 1], [0, 0, 0]]
    n = np.zeros(1, dtype=NODE)
    n["num_tris"] = 2
    r = refit_model.refit(n, t)
    assert r["bounds_min"][0].tolist() == [0, 0, 0] and r["bounds_max"][0].tolist() == [2, 5, 1]
