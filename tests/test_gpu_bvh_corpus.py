"""-m gpu: the device BVH builder (csrc/bvh_build_device.hip) on the corpus of tests/tools/bvh_corpus.py, against the ORACLE's trees.

tests/test_bvh_corpus.py proves on the CPU what the corpus reaches -- every node class refusing to split, splitting one triangle off
and splitting evenly, roots at every class and chunk edge, child counts on a chunk edge, trees of more than two renumbering runs, wide
levels between runs -- and that the host builder agrees with the oracle on it.  Here the device builder has to reproduce every entry
exactly: the node array (sign of a zero bound aside) and the reordered triangle bytes, no tolerance anywhere.
  * every entry through mipt_bvh_build_device (Scene.build_bvh_device);
  * a subset through the product's path, mipt_scene_create_from_triangles + mipt_scene_get_bvh (bvh_build_resident without the gather);
  * three entries through one REBUILD update with the same triangles: the builder's second use inside a resident scene.
A failure names the first differing node, its class and its parent's split from the census, i.e. which kernel to open.  Nothing renders."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import bvh_corpus as bc  # noqa: E402

pytestmark = pytest.mark.gpu


def _assert_tree(name, how, nodes, tris, ref_nodes, ref_tris):
    bad = bc.first_difference(nodes, ref_nodes)
    if bad is not None:
        raise AssertionError(f"{name} ({how}): {len(nodes)} nodes against the oracle's {len(ref_nodes)}, first difference at "
                             + bc.describe(bc.census(ref_nodes), bad))
    if tris.tobytes() != ref_tris.tobytes():
        from rust_ray_tracing_amd import NODE
        a, b = np.ascontiguousarray(tris).view(np.uint8).reshape(-1, 112), np.ascontiguousarray(ref_tris).view(np.uint8).reshape(-1, 112)
        t = int(np.flatnonzero((a != b).any(axis=1))[0])
        cen = bc.census(ref_nodes)
        first = np.ascontiguousarray(ref_nodes).view(NODE).reshape(-1)["first_tri_or_child"]
        leaf = [int(i) for i, cnt in cen["leaves"] if first[i] <= t < first[i] + cnt][0]
        raise AssertionError(f"{name} ({how}): same nodes, triangle order differs first at slot {t}, in the leaf " + bc.describe(cen, leaf))


def _fetch(rrt, sc, src):
    """the resident scene's tree and the triangles in its order (mipt_scene_get_bvh)"""
    from rust_ray_tracing_amd import _lib as L
    nodes = np.zeros(2 * len(src), dtype=L.NODE)
    order = np.zeros(len(src), dtype=np.uint32)
    cnt = C.c_uint32()
    lib = rrt.load()
    assert lib.mipt_scene_get_bvh(sc._handle, L.ptr(nodes), len(nodes), C.byref(cnt), L.ptr(order)) == 0, lib.mipt_last_error()
    return nodes[: cnt.value], src[order]


@pytest.mark.parametrize("name", list(bc.ENTRIES))
def test_device_builder_matches_oracle(rrt, orc, name):
    tris, ref_tris, ref_nodes = bc.reference(orc, name)
    dev = rrt.Scene.from_arrays(tris, [rrt.material_default()], build_bvh=False)
    dev.build_bvh_device(0)
    _assert_tree(name, "mipt_bvh_build_device", dev.bvh_nodes, dev.tris, ref_nodes, ref_tris)


@pytest.mark.parametrize("name", bc.RESIDENT)
def test_resident_setup_matches_oracle(rrt, orc, name):
    from rust_ray_tracing_amd import _lib as L
    tris, ref_tris, ref_nodes = bc.reference(orc, name)
    sc = rrt.Scene.from_arrays(tris, [rrt.material_default()], build_bvh=False)
    sc.upload_from_triangles(0, fetch_bvh=True)
    assert sc.info()["built_on_device"] == 1
    _assert_tree(name, "mipt_scene_create_from_triangles", sc.bvh_nodes, sc.tris, ref_nodes, ref_tris)
    if name in bc.REBUILD:
        lib = rrt.load()
        src = np.ascontiguousarray(tris)
        inf = L.MiptUpdateInfo()
        assert lib.mipt_scene_update_triangles(sc._handle, L.ptr(src), len(src), L.UPDATE_REBUILD, C.byref(inf)) == 0, lib.mipt_last_error()
        assert inf.n_tris == len(src) and inf.n_nodes == len(ref_nodes)
        nodes, reordered = _fetch(rrt, sc, src)
        _assert_tree(name, "REBUILD with the same triangles", nodes, reordered, ref_nodes, ref_tris)
    sc.release()
