"""tests/tools/refit_model.py's vectorised refit_by_levels (what the million-triangle REFIT test of test_gpu_scene_update.py is held
to) against the node-by-node `refit` and against `per_node_fold`, on the host builder's trees of the small cases.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import refit_model  # noqa: E402
from test_gpu_scene_update import _case, _deform  # noqa: E402

CASES = ["soup1", "soup17", "soup300d", "soup9000d", "cornell", "helmet"]


@pytest.mark.parametrize("name", CASES)
def test_refit_by_levels_is_refit(rrt, name):
    tris, mats, texs, _ = _case(name)
    sc = rrt.Scene.from_arrays(tris, mats, texs)                          # mipt_bvh_build: tris in tree order
    nodes = sc.bvh_nodes
    depth = refit_model.node_depths(nodes)
    assert depth[0] == 0 and (depth >= 0).all()
    inner = np.flatnonzero(nodes["num_tris"] == 0)
    kids = nodes["first_tri_or_child"][inner].astype(np.int64)
    assert np.array_equal(depth[kids], depth[inner] + 1) and np.array_equal(depth[kids + 1], depth[inner] + 1)
    same = refit_model.refit_by_levels(nodes, sc.tris)                    # the builder's own bounds are the fold already
    assert refit_model.same_nodes(same, nodes)
    rng = np.random.default_rng(len(nodes))
    for i, how in enumerate(("jitter", "rigid", "scale")):
        new = _deform(sc.tris, how, 50 + i)
        if len(new) > 2:                                                  # what fmin / fmax and the clamps are there for
            new["vertices"]["position"][len(new) // 2, 1, 0] = np.nan
            new["vertices"]["position"][1, 2] = (np.inf, -np.inf, 3e38)
        want = refit_model.refit(nodes, new)
        got = refit_model.refit_by_levels(nodes, new)
        assert refit_model.same_nodes(got, want), how
        assert not refit_model.same_nodes(got, nodes)
        assert np.array_equal(got["bounds_min"].view(np.uint32), want["bounds_min"].view(np.uint32))     # here even the sign of a zero
        assert np.array_equal(got["bounds_max"].view(np.uint32), want["bounds_max"].view(np.uint32))
        which = np.unique(np.concatenate([np.arange(min(len(nodes), 40)), rng.integers(0, len(nodes), 60)]))
        mn, mx = refit_model.per_node_fold(nodes, new, which)
        assert np.array_equal(mn, got["bounds_min"][which]) and np.array_equal(mx, got["bounds_max"][which]), how


def test_refit_by_levels_refuses_what_it_cannot_fold(rrt):
    """leaves that do not partition the triangles (a caller's tree with unreferenced triangles) are the node-by-node model's case"""
    tris, mats, texs, _ = _case("soup300d")
    sc = rrt.Scene.from_arrays(tris, mats, texs)
    nodes = sc.bvh_nodes.copy()
    two = np.flatnonzero(nodes["num_tris"] >= 2)
    nodes["num_tris"][two[0]] -= 1
    with pytest.raises(AssertionError):
        refit_model.refit_by_levels(nodes, sc.tris)
