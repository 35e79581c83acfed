"""-m gpu: the device BVH builder (csrc/bvh_build_device.hip) on the corpus of tests/tools/bvh_corpus.py, against the ORACLE's trees.

tests/test_bvh_corpus.py proves on the CPU what the corpus reaches -- every node class refusing to split, splitting one triangle off
and splitting evenly, roots at every class and chunk edge, child counts on a chunk edge, trees of more than two renumbering runs, wide
levels between runs -- and that the host builder agrees with the oracle on it.  Here the device builder has to reproduce every entry
exactly: the node array (sign of a zero bound aside) and the reordered triangle bytes, no tolerance anywhere.
  * every entry through mipt_bvh_build_device (Scene.build_bvh_device);
  * a subset through the product's path, mipt_scene_create_from_triangles + mipt_scene_get_bvh (bvh_build_resident without the gather);
  * three entries through one REBUILD update with the same triangles: the builder's second use inside a resident scene.
A failure names the first differing node, its class and its parent's split from the census, i.e. which kernel to open.  Nothing renders.

The LARGE entries (574 674 to 3.3 M triangles) take the builder's and the layout's loops on their second trip -- grid-stride loops
over capped grids, big_scan's steps of 64 chunks, big_setup's strips of 1 024 nodes, the layout's scans of more than one tile per
workgroup; DESIGN section 21 has a row per launch, tests/test_bvh_corpus.py asserts the reach on the CPU.  The oracle takes 23 s and
more for one of them, so their reference is the HOST builder, which that file holds to the oracle at the smallest of them:
  * every LARGE entry through mipt_bvh_build_device;
  * three through the resident setup, where the device layout of both entries (from triangles, and mipt_scene_create given that tree)
    must also equal the host restatement of the layout byte for byte, fingerprint included, as in tests/test_gpu_scene_device.py;
  * one of those through a REBUILD with the same triangles;
  * `late_leaf` (140 053 triangles) through the resident setup: the largest leaf lies where only check_nodes' second trip finds it.
Each of the LARGE tests prints its seconds by part (generation and host reference are paid by the first test that asks for an entry)."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import bvh_corpus as bc  # noqa: E402

pytestmark = pytest.mark.gpu


def _assert_tree(name, how, nodes, tris, ref_nodes, ref_tris, census=None, whose="the oracle's"):
    """`census`: a function returning the census of ref_nodes, where a caller keeps one; it is asked only when something differs."""
    census = census or (lambda: bc.census(ref_nodes))
    bad = bc.first_difference(nodes, ref_nodes)
    if bad is not None:
        raise AssertionError(f"{name} ({how}): {len(nodes)} nodes against {whose} {len(ref_nodes)}, first difference at "
                             + bc.describe(census(), bad))
    if tris.tobytes() != ref_tris.tobytes():
        from rust_ray_tracing_amd import NODE
        a, b = np.ascontiguousarray(tris).view(np.uint8).reshape(-1, 112), np.ascontiguousarray(ref_tris).view(np.uint8).reshape(-1, 112)
        t = int(np.flatnonzero((a != b).any(axis=1))[0])
        cen = census()
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


# ---- the LARGE entries, against the host builder ----------------------------------------------------------------------------------------
def _assert_large(rrt, name, how, nodes, tris):
    _, ref_tris, ref_nodes = bc.reference_host(rrt, name)
    _assert_tree(name, how, nodes, tris, ref_nodes, ref_tris, census=lambda: bc.census_host(rrt, name), whose="the host builder's")


def _report(name, what, first, parts):
    gen, host = bc.reference_host_seconds[name] if first else (0.0, 0.0)
    print(f"{name} ({what}): generation {gen:.2f} s, host reference {host:.2f} s, "
          + ", ".join(f"{k} {v:.2f} s" for k, v in parts.items()))


def _device_layout(rrt, handle):
    """both buffers of a resident scene and their fingerprint (libmipt_diag.so), as tests/test_gpu_scene_device.py reads them"""
    diag = rrt.load_diag()
    sizes = (C.c_uint64 * 2)()
    assert diag.mipt_diag_scene_sizes(handle, C.byref(sizes)) == 0
    geom, attr = np.zeros(sizes[0], dtype=np.uint8), np.zeros(sizes[1], dtype=np.uint8)
    assert diag.mipt_diag_scene_read(handle, 0, geom.ctypes.data, sizes[0]) == 0
    assert diag.mipt_diag_scene_read(handle, 1, attr.ctypes.data, sizes[1]) == 0
    h = (C.c_uint64 * 2)()
    assert diag.mipt_diag_scene_hash(handle, C.byref(h)) == 0
    return geom, attr, (int(h[0]), int(h[1]))


def _assert_layout(rrt, name, dev, hd):
    """tests/test_gpu_scene_device.py::_check_scene, step 2: the layout of the scene made from triangles, and of mipt_scene_create
    given the tree it reports, against the host restatement of the layout of that tree"""
    mats = [rrt.material_default()]
    ref = rrt.Scene.from_arrays(dev.tris, mats, build_bvh=False)
    ref.bvh_nodes = dev.bvh_nodes.copy()
    hr = ref.upload(0)
    g0, a0, i0 = ref.host_layout()
    diag = rrt.load_diag()
    h0 = []
    for buf in (g0, a0):                                        # Scene.host_layout_fingerprint, without laying out a second time
        h = C.c_uint64()
        assert diag.mipt_diag_hash_words(buf.ctypes.data, buf.size // 4, C.byref(h)) == 0
        h0.append(int(h.value))
    for entry, handle in (("from_triangles", hd), ("from_nodes", hr)):
        g1, a1, h1 = _device_layout(rrt, handle)
        assert g1.size == g0.size and a1.size == a0.size, f"{name}, {entry}"
        assert np.array_equal(a1, a0), f"{name}, {entry}: attribute stream differs"
        if not np.array_equal(g1, g0):
            bad = np.flatnonzero(g1 != g0)
            raise AssertionError(f"{name}, {entry}: geometry differs in {bad.size} bytes, first at {bad[0]} (record {bad[0] // 64}) of {g1.size}; "
                                 f"{i0['n_pair_records']} pair records come first")
        assert h1 == tuple(h0), f"{name}, {entry}"
    ri, hi = ref.info(), dev.info()
    assert ri["built_on_device"] == 0 and hi["built_on_device"] == 1
    for k in ("n_tris", "n_nodes", "n_pair_records", "max_leaf", "geometry_bytes"):
        assert ri[k] == hi[k], k
    assert hi["n_pair_records"] == i0["n_pair_records"] and hi["max_leaf"] == i0["max_leaf"]
    ref.release()


@pytest.mark.parametrize("name", list(bc.LARGE))
def test_device_builder_matches_host_past_the_caps(rrt, name):
    first = name not in bc.reference_host_seconds
    tris, _, _ = bc.reference_host(rrt, name)
    dev = rrt.Scene.from_arrays(tris, [rrt.material_default()], build_bvh=False)
    t0 = time.perf_counter()
    dev.build_bvh_device(0)
    t1 = time.perf_counter()
    _assert_large(rrt, name, "mipt_bvh_build_device", dev.bvh_nodes, dev.tris)
    _report(name, "mipt_bvh_build_device", first, {"device call": t1 - t0, "compare": time.perf_counter() - t1})


@pytest.mark.parametrize("name", bc.LARGE_RESIDENT)
def test_resident_setup_matches_host_past_the_caps(rrt, name):
    from rust_ray_tracing_amd import _lib as L
    first = name not in bc.reference_host_seconds
    tris, _, ref_nodes = bc.reference_host(rrt, name)
    sc = rrt.Scene.from_arrays(tris, [rrt.material_default()], build_bvh=False)
    parts = {}
    t0 = time.perf_counter()
    hd = sc.upload_from_triangles(0, fetch_bvh=True)
    parts["device call"] = time.perf_counter() - t0
    assert sc.info()["built_on_device"] == 1
    t0 = time.perf_counter()
    _assert_large(rrt, name, "mipt_scene_create_from_triangles", sc.bvh_nodes, sc.tris)
    parts["compare"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    _assert_layout(rrt, name, sc, hd)
    parts["layout, host and both entries"] = time.perf_counter() - t0
    if name in bc.LARGE_REBUILD:
        lib = rrt.load()
        src = np.ascontiguousarray(tris)
        inf = L.MiptUpdateInfo()
        t0 = time.perf_counter()
        assert lib.mipt_scene_update_triangles(sc._handle, L.ptr(src), len(src), L.UPDATE_REBUILD, C.byref(inf)) == 0, lib.mipt_last_error()
        assert inf.n_tris == len(src) and inf.n_nodes == len(ref_nodes)
        nodes, reordered = _fetch(rrt, sc, src)
        parts["REBUILD call and fetch"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        _assert_large(rrt, name, "REBUILD with the same triangles", nodes, reordered)
        parts["REBUILD compare"] = time.perf_counter() - t0
    sc.release()
    _report(name, "resident setup", first, parts)


def test_largest_leaf_past_the_grid_of_check_nodes(rrt):
    """check_nodes (1 024 x 256 threads) finds the largest leaf, which the trace kernel's leaf loop is sized by.  In `late_leaf` the one
    leaf above four triangles is node 280 001 (tests/test_bvh_corpus.py::test_late_leaf), so max_leaf of both entries is the host
    layout's 48 only if the grid-stride loop takes its second trip."""
    name = "late_leaf"
    tris, _, _ = bc.reference_host(rrt, name)
    sc = rrt.Scene.from_arrays(tris, [rrt.material_default()], build_bvh=False)
    hd = sc.upload_from_triangles(0, fetch_bvh=True)
    _assert_large(rrt, name, "mipt_scene_create_from_triangles", sc.bvh_nodes, sc.tris)
    assert sc.info()["max_leaf"] == bc.LATE_LEAF
    _assert_layout(rrt, name, sc, hd)                          # max_leaf of both entries == the host layout's, and the layout itself
    sc.release()
