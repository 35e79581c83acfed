"""-m gpu: new geometry in a resident scene -- mipt_scene_update_triangles{,_device}, mipt_multi_update_triangles (csrc/scene_update.hip).

For scenes made both ways (mipt_scene_create from host-built nodes, mipt_scene_create_from_triangles) on the synth families, degenerate
soups and a caller's tree that leaves triangles unreferenced:
  * REFIT with the same triangles changes no layout byte and no pixel;
  * REFIT after a deformation gives the layout of mipt_scene_create from (new triangles, restated refit nodes), byte for byte with
    bounds modulo the sign of a zero, the refit tree from mipt_scene_get_bvh, and the oracle's frame and counters;
  * the device entry (a torch tensor in HBM) is byte-identical to the host entry and leaves the tensor alone;
  * REBUILD (also to another triangle count) is a fresh mipt_scene_create_from_triangles;
  * errors leave the scene untouched; sequences neither drift nor leak; replicas follow the root;
  * a REFIT of more than 2^20 triangles and one of more than 1024 big leaves take every capped launch past its grid."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import refit_model  # noqa: E402

CAM = ((12.0, 0.5, 0.3), 0.0, 0.0)


def _soup(n, seed, degenerate=False, sigma=0.3):
    from rust_ray_tracing_amd import TRIANGLE
    rng = np.random.default_rng(seed)
    t = np.zeros(n, dtype=TRIANGLE)
    c = rng.uniform(-4, 4, (n, 1, 3)).astype(np.float32)
    t["vertices"]["position"] = c + rng.normal(0, sigma, (n, 3, 3)).astype(np.float32)
    t["vertices"]["normal"] = rng.normal(0, 1, (n, 3, 3)).astype(np.float32)
    t["vertices"]["tex_coord_x"] = rng.uniform(0, 4, (n, 3)).astype(np.float32)
    t["vertices"]["tex_coord_y"] = rng.uniform(0, 4, (n, 3)).astype(np.float32)
    if degenerate:                          # coincident triangles (one leaf of thousands: BVH::build will not split them), slivers, zeros
        t[n // 4: n // 2] = t[n // 4]
        t["vertices"]["position"][n // 2: n // 2 + n // 8, 1] = t["vertices"]["position"][n // 2: n // 2 + n // 8, 0]
        t["vertices"]["position"][-(n // 8):, :, 2] = 0.0
    return t


def _cluster_soup(n_clusters=1500, seed=31):
    """clusters of 17 to 40 coincident triangles (copies of one triangle: BVH::build cannot split them, so each is one leaf of more
    than kSerialLeaf = 16), their centres on a jittered grid 0.65 apart, well clear of each other -> (triangles, cluster of each)"""
    rng = np.random.default_rng(seed)
    size = rng.integers(17, 41, n_clusters)
    cluster = np.repeat(np.arange(n_clusters), size)
    one = _soup(n_clusters, seed + 1, sigma=0.06)
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(11), indexing="ij"), -1).reshape(-1, 3)[:n_clusters]
    centre = (g * 0.65 - 3.6 + rng.uniform(-0.1, 0.1, g.shape)).astype(np.float32)
    p = one["vertices"]["position"]
    p += centre[:, None, :] - p.mean(axis=1, keepdims=True)
    return one[cluster], cluster


def _case(name):
    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import synth
    kw = {"cornell": {}, "helmet": dict(n_target=3000, tex_size=16), "atrium": dict(n_target=20000, tex_size=16),
          "dragon": dict(n_target=20000)}
    if name in kw:
        tris, mats, texs, cam = synth.make_scene(name, **kw[name])
        return tris, mats, texs, cam
    n, seed, deg = {"soup300d": (300, 5, True), "soup17": (17, 4, False), "soup1": (1, 1, False), "soup9000d": (9000, 7, True)}[name]
    return _soup(n, seed, deg), [rrt.material_default()], [], CAM


def _make(rrt, tris, mats, texs, cam, kind):
    """kind 'host': mipt_scene_create from host-built nodes (tris in tree order); 'device': mipt_scene_create_from_triangles with the
    tree fetched back (tris in tree order, the device keeps the caller's order)"""
    sc = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=(kind == "host"))
    if kind == "host":
        sc.upload(0)
    else:
        sc.upload_from_triangles(0, fetch_bvh=True)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    return sc


def _layout(rrt, handle):
    diag = rrt.load_diag()
    sizes = (C.c_uint64 * 2)()
    assert diag.mipt_diag_scene_sizes(handle, C.byref(sizes)) == 0
    geom = np.zeros(sizes[0], dtype=np.uint8)
    attr = np.zeros(sizes[1], dtype=np.uint8)
    assert diag.mipt_diag_scene_read(handle, 0, geom.ctypes.data, sizes[0]) == 0
    assert diag.mipt_diag_scene_read(handle, 1, attr.ctypes.data, sizes[1]) == 0
    h = (C.c_uint64 * 2)()
    assert diag.mipt_diag_scene_hash(handle, C.byref(h)) == 0
    return geom, attr, (int(h[0]), int(h[1]))


def _unsigned_zeros(geom, n_records):
    """the pair records with every -0.0 bound made +0.0 (the sign of a zero in a bound may depend on the fold order)"""
    g = geom.copy()
    f = g[: n_records * 64].view(np.float32).reshape(-1, 16)
    for col in (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14):
        v = f[:, col]
        v[v == 0.0] = 0.0
    return g


def _same_layout(a, b, n_records, what):
    ga, gb = _unsigned_zeros(a[0], n_records), _unsigned_zeros(b[0], n_records)
    assert ga.size == gb.size and a[1].size == b[1].size, what + ": sizes differ"
    assert np.array_equal(a[1], b[1]), what + ": attribute stream differs"
    if not np.array_equal(ga, gb):
        bad = np.flatnonzero(ga != gb)
        raise AssertionError(f"{what}: geometry differs in {bad.size} bytes, first at {bad[0]} (record {bad[0] // 64}) of {ga.size}")


def _render(rrt, sc, w=64, h=36, spp=2, depth=6):
    from rust_ray_tracing_amd import _lib as L
    r = rrt.Renderer.new(rrt.RendererOptions(samples=spp, max_ray_depth=depth, output_image_dimensions=(w, h), output_image_path="/dev/null"))
    return r.render_buffers(sc, flags=L.FLAG_COUNT)


def _oracle_check(rrt, orc, sc, tris, nodes, w=64, h=36, spp=2, depth=6):
    f, p, s = _render(rrt, sc, w, h, spp, depth)
    of, op_, os_ = orc.render(tris, nodes, sc.materials_array(), sc.textures, sc.camera.uniform, w, h, spp, depth)
    assert np.array_equal(f.view(np.uint32), of.view(np.uint32)) and np.array_equal(p, op_), "frame differs from the oracle's"
    assert s["rays"] == os_["rays"] and s["tri_tests"] == os_["tri_tests"] and s["hits"] == os_["hits"]
    return f, s


def _expected_layout(rrt, tris, nodes, mats, texs):
    ref = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    ref.bvh_nodes = nodes
    g, a, info = ref.host_layout()
    return (g, a), info


def _refit_layout(rrt, before, nodes0, new, want, mats, texs):
    """What a REFIT must leave: mipt_scene_create's layout of (new triangles, refit nodes) -- triangle streams and record contents --
    with the pair records in the order of the ORIGINAL tree.  (A REFIT keeps the record order; a fresh layout orders the records below
    the breadth-first top by child surface area, mipt_internal.h, which the new bounds may change.)"""
    from rust_ray_tracing_amd import _lib as L
    (g, a), info = _expected_layout(rrt, new, want, mats, texs)
    n_rec = info["n_pair_records"]
    order = np.zeros(n_rec + 4, dtype=np.uint32)
    cnt = C.c_uint32()
    assert rrt.load_diag().mipt_internal_pair_order(L.ptr(nodes0), len(nodes0), L.ptr(order), len(order), C.byref(cnt)) == 0
    rec = before[0][: n_rec * 64].copy().view(np.float32).reshape(-1, 16)
    j = np.flatnonzero(order[: cnt.value] != 0xFFFFFFFF)
    k = order[j].astype(np.int64)
    for w in (0, 1):
        nd = want[2 * k + 1 + w]
        rec[j, 8 * w: 8 * w + 3] = nd["bounds_min"]
        rec[j, 8 * w + 4: 8 * w + 7] = nd["bounds_max"]
    g = g.copy()
    g[: n_rec * 64] = rec.view(np.uint8).ravel()
    return g, a


def _deform(tris, how, seed):
    rng = np.random.default_rng(seed)
    t = tris.copy()
    p = t["vertices"]["position"]
    if how == "jitter":
        p += rng.normal(0, 0.02, p.shape).astype(np.float32)
    elif how == "rigid":                                            # a contiguous subset moves as one piece
        k0, k1 = len(t) // 3, len(t) // 3 + max(1, len(t) // 4)
        p[k0:k1] += np.array([0.25, -0.5, 0.125], dtype=np.float32)
    else:
        p *= np.float32(1.5)
    t["vertices"]["normal"] = -t["vertices"]["normal"]
    return t


CASES = ["cornell", "helmet", "atrium", "dragon", "soup1", "soup17", "soup300d", "soup9000d"]


@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("name", CASES)
def test_refit_identity_and_deformation(rrt, orc, name, kind):
    tris, mats, texs, cam = _case(name)
    sc = _make(rrt, tris, mats, texs, cam, kind)
    h = sc._handle
    n_rec = sc.info()["n_pair_records"]
    before = _layout(rrt, h)
    f0, _, s0 = _render(rrt, sc)
    # 1. the same triangles: nothing changes
    nodes0 = sc.bvh_nodes.copy()
    inf = sc.update_device(0)
    assert inf["n_tris"] == len(tris) and inf["n_pair_records"] == n_rec and inf["build_ms"] >= 0.0
    _same_layout(_layout(rrt, h), before, n_rec, "identity refit")
    f1, _, s1 = _render(rrt, sc)
    assert np.array_equal(f1.view(np.uint32), f0.view(np.uint32)) and s1["tri_tests"] == s0["tri_tests"]
    assert refit_model.same_nodes(sc.bvh_nodes, nodes0)
    # 2. deformations: layout == mipt_scene_create's from (new tris in tree order, restated refit nodes); frame == oracle's
    for i, how in enumerate(("jitter", "rigid", "scale")):
        new = _deform(sc.tris, how, 100 + i)
        want = refit_model.refit(sc.bvh_nodes, new)
        sc.tris = new
        sc.update_device(0)
        assert refit_model.same_nodes(sc.bvh_nodes, want), how          # device scenes: mipt_scene_get_bvh; host scenes: host.refit_nodes
        exp = _refit_layout(rrt, before, nodes0, new, want, mats, texs)
        _same_layout(_layout(rrt, h), exp, n_rec, how)
        _oracle_check(rrt, orc, sc, new, want)
    # the restatement against an independent fold per node
    mn, mx = refit_model.per_node_fold(sc.bvh_nodes, sc.tris, range(min(len(sc.bvh_nodes), 200)))
    assert np.array_equal(mn, sc.bvh_nodes["bounds_min"][: len(mn)]) and np.array_equal(mx, sc.bvh_nodes["bounds_max"][: len(mx)])


def test_refit_callers_tree_with_unreferenced_triangles(rrt, orc):
    """leaves that shrank (triangles no leaf refers to) and a root that is a leaf: the refit folds only what the leaves reference"""
    from rust_ray_tracing_amd import NODE, synth
    tris, mats, texs, cam = synth.make_scene("atrium", n_target=20000, tex_size=16)
    base = rrt.Scene.from_arrays(tris, mats, texs)
    nodes = base.bvh_nodes.copy()
    two = np.flatnonzero(nodes["num_tris"] == 2)
    nodes["num_tris"][two[::3]] = 1
    nodes["first_tri_or_child"][two[1::3]] += 1
    nodes["num_tris"][two[1::3]] = 1
    leaf = np.zeros(1, dtype=NODE)
    leaf["bounds_min"], leaf["bounds_max"] = base.bvh_nodes["bounds_min"][0], base.bvh_nodes["bounds_max"][0]
    leaf["num_tris"] = 5
    for t, n in ((base.tris, nodes), (base.tris[:9].copy(), leaf)):
        sc = rrt.Scene.from_arrays(t, mats, texs, build_bvh=False)
        sc.bvh_nodes = n.copy()
        h = sc.upload(0)
        sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
        n_rec = sc.info()["n_pair_records"]
        before = _layout(rrt, h)
        new = _deform(sc.tris, "jitter", 7)
        lv = n["num_tris"] > 0
        refd = np.concatenate([np.arange(f, f + c) for f, c in zip(n["first_tri_or_child"][lv], n["num_tris"][lv])])
        unref = np.setdiff1d(np.arange(len(new)), refd)
        assert len(unref) > 0
        new["vertices"]["position"][unref[0]] = np.float32(5e12)       # a triangle no leaf references reaches no bound
        want = refit_model.refit(n, new)
        sc.tris = new
        sc.update_device(0)
        assert refit_model.same_nodes(sc.bvh_nodes, want)
        exp = _refit_layout(rrt, before, n, new, want, mats, texs)
        _same_layout(_layout(rrt, h), exp, n_rec, "caller's tree")
        _oracle_check(rrt, orc, sc, new, want)
        sc.release()


def test_refit_with_more_big_leaves_than_workgroups(rrt, orc):
    """refit_big_leaves launches 1024 workgroups, one leaf child of more than kSerialLeaf = 16 triangles per trip with a
    __syncthreads inside the trip: 1500 clusters of coincident triangles are 1500 such leaves, so 476 workgroups fold a second one.
    Every cluster moves by its own offset: a leaf that is skipped, or folded from another leaf's slots, keeps or gets a wrong box."""
    tris, cluster = _cluster_soup()
    mats = [rrt.material_default()]
    sc = _make(rrt, tris, mats, [], CAM, "device")
    h = sc._handle
    nodes0 = sc.bvh_nodes.copy()
    assert int(np.count_nonzero(nodes0["num_tris"] > 16)) > 1024            # the condition: from the tree the device built
    n_rec = sc.info()["n_pair_records"]
    before = _layout(rrt, h)
    offset = np.random.default_rng(32).uniform(-0.25, 0.25, (cluster.max() + 1, 3)).astype(np.float32)
    new = sc.tris.copy()
    new["vertices"]["position"] += offset[cluster[sc._tri_order]][:, None, :]
    want = refit_model.refit(nodes0, new)
    assert not np.array_equal(want["bounds_min"][nodes0["num_tris"] > 16], nodes0["bounds_min"][nodes0["num_tris"] > 16])
    sc.tris = new
    sc.update_device(0)
    assert refit_model.same_nodes(sc.bvh_nodes, want)
    _same_layout(_layout(rrt, h), _refit_layout(rrt, before, nodes0, new, want, mats, []), n_rec, "1500 big leaves")
    _oracle_check(rrt, orc, sc, new, want)


def test_refit_past_the_grid_caps(rrt, orc):
    """A soup of 2^20 + 4099 triangles, one per leaf: 1 052 676 pair records, 351 783 of them in the fullest level.  Every capped
    launch of the REFIT takes a second trip or more:
      check_materials, rewrite_tris  4096 x 256 = 1 048 576 triangles          passed (1 052 675)
      refit_leaves, refit_level      4096 x 256 = 1 048 576 records            passed by refit_leaves (1 052 676 records); refit_level's
                                                                               fullest launch has 351 783 and stays in its first trip
      check_bounds                   2048 x 256 = 524 288 of 2 * records + 1   passed (more than 262 144 records)
      refit_nodes                    2048 x 256 = 524 288 plan entries         passed
      plan_level                     1024 x 256 = 262 144 records of a level   passed (the test asserts the level's size)
    The expected tree is refit_model.refit_by_levels (tests/test_refit_model.py holds it to `refit`).  The refusals sit in the strided
    part: the lower of two bad material ids past index 2^20 is named, and a coordinate of 3e12 in a triangle whose record lies behind
    check_bounds' first trip is refused (its box also reaches every ancestor up to record 0, so this alone could not tell a
    check_bounds that stops after one trip); after each the layout is byte for byte what it was, and the good REFIT that follows
    gives the expected layout.  The CPU oracle renders the 64x36 frame (2 spp, depth 6, 2194 hits) of this scene in about 50 ms."""
    from rust_ray_tracing_amd import _lib as L
    n = (1 << 20) + 4099
    tris = _soup(n, 21, sigma=float(0.3 * (300.0 / n) ** (1.0 / 3.0)))     # as dense as soup300: not a solid block of overlaps
    mats = [rrt.material_default()]
    sc = _make(rrt, tris, mats, [], CAM, "device")
    h, lib, order = sc._handle, rrt.load(), sc._tri_order
    n_rec = sc.info()["n_pair_records"]
    nodes0 = sc.bvh_nodes.copy()
    per_level = np.bincount(refit_model.node_depths(nodes0)[nodes0["num_tris"] == 0])     # a record per inner node, at its depth
    print(f"{n} triangles, {n_rec} pair records, {len(nodes0)} nodes, {per_level.size} levels, {per_level.max()} records in the fullest")
    assert n_rec > 1 << 20 and per_level.max() > 262144                     # which caps this tree passes (docstring)
    before = _layout(rrt, h)
    new = _deform(sc.tris, "jitter", 5)                                     # in the tree's order
    want = refit_model.refit_by_levels(nodes0, new)

    def device_order(t):
        src = np.empty_like(t)
        src[order] = t
        return src

    def refused(t, status, words):
        rc = lib.mipt_scene_update_triangles(h, L.ptr(t), len(t), 0, None)
        assert rc == status and words in lib.mipt_last_error(), (rc, lib.mipt_last_error())
        after = _layout(rrt, h)
        assert after[2] == before[2] and np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])

    src = device_order(new)
    bad = src.copy()
    i1, i2 = (1 << 20) + 1000, (1 << 20) + 3000                             # both in check_materials' second trip
    bad["material_id"][i2], bad["material_id"][i1] = 7, 9
    refused(bad, L.ERR_INVALID_ARG, b"triangle %d has material_id 9 " % i1)
    # a leaf child of the last record that has one: child 2j + w, far behind check_bounds' first 524 288
    rec = before[0][: n_rec * 64].view(np.uint32).reshape(-1, 16)
    slot_tri = before[0][n_rec * 64: (n_rec + n) * 64].view(np.uint32).reshape(-1, 16)[:, 9]
    assert np.array_equal(np.sort(slot_tri), np.arange(n, dtype=np.uint32))    # every slot names its triangle (tree order)
    j = int(np.flatnonzero((rec[:, 7] != 0) | (rec[:, 15] != 0))[-1])
    w = 0 if rec[j, 7] != 0 else 1
    assert 2 * j + w >= 2048 * 256
    far = new.copy()
    far["vertices"]["position"][slot_tri[rec[j, 8 * w + 3]], 1, 0] = np.float32(3e12)
    refused(device_order(far), L.ERR_SCENE_LIMIT, b"2^40")
    del bad, far
    # the good REFIT
    sc.tris = new
    sc.update_device(0)
    assert refit_model.same_nodes(sc.bvh_nodes, want)
    _same_layout(_layout(rrt, h), _refit_layout(rrt, before, nodes0, new, want, mats, []), n_rec, "REFIT of 2^20 + 4099 triangles")
    _oracle_check(rrt, orc, sc, new, want)
    sc.release()


@pytest.mark.parametrize("kind", ["host", "device"])
def test_device_entry_equals_host_entry(rrt, kind):
    import torch
    from rust_ray_tracing_amd import _lib as L
    tris, mats, texs, cam = _case("atrium")
    a = _make(rrt, tris, mats, texs, cam, kind)
    b = _make(rrt, tris, mats, texs, cam, kind)
    new = _deform(a.tris, "jitter", 3)
    a.tris = new
    a.update_device(0)                                                 # host entry (scattered back to the device's order)
    src = new if kind == "host" else np.empty_like(new)
    if kind == "device":
        src[b._tri_order] = new
    t = torch.from_numpy(src.view(np.uint8).copy()).to("cuda:0")
    keep = t.clone()
    lib = rrt.load()
    inf = L.MiptUpdateInfo()
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.mipt_scene_update_triangles_device(b._handle, t.data_ptr(), len(src), 0, stream, C.byref(inf)) == 0, lib.mipt_last_error()
    assert inf.upload_ms == 0.0 and inf.n_tris == len(src)
    torch.cuda.synchronize()
    assert torch.equal(t, keep), "the device entry modified its input"
    la, lb = _layout(rrt, a._handle), _layout(rrt, b._handle)
    assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1]) and la[2] == lb[2]
    # REBUILD straight from the tensor
    inf2 = L.MiptUpdateInfo()
    assert lib.mipt_scene_update_triangles_device(b._handle, t.data_ptr(), len(src), 1, stream, C.byref(inf2)) == 0, lib.mipt_last_error()
    fresh = rrt.Scene.from_arrays(src, mats, texs, build_bvh=False)
    fresh.upload_from_triangles(0)
    assert _layout(rrt, b._handle)[2] == _layout(rrt, fresh._handle)[2]
    assert torch.equal(t, keep)


@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("name,change", [("atrium", 0), ("atrium", -3001), ("dragon", 517), ("soup9000d", -1000), ("cornell", 0)])
def test_rebuild_is_a_fresh_create(rrt, orc, name, kind, change):
    from rust_ray_tracing_amd import _lib as L
    tris, mats, texs, cam = _case(name)
    sc = _make(rrt, tris, mats, texs, cam, kind)
    h = sc._handle
    src = np.empty_like(sc.tris)                                       # what the device was built from
    if sc._tri_order is not None:
        src[sc._tri_order] = sc.tris
    else:
        src[:] = sc.tris
    new = _deform(src, "rigid", 11)
    if change > 0:
        new = np.concatenate([new, _deform(new[:change], "scale", 12)])
    elif change < 0:
        new = new[:change].copy()
    lib = rrt.load()
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=4, output_image_dimensions=(32, 18), output_image_path="/dev/null"))
    r.render_buffers(sc, flags=L.FLAG_COUNT | L.FLAG_TOUCHED)          # allocates the bitmap for the old geometry
    inf = L.MiptUpdateInfo()
    assert lib.mipt_scene_update_triangles(h, L.ptr(new), len(new), 1, C.byref(inf)) == 0, lib.mipt_last_error()
    fresh = rrt.Scene.from_arrays(new, mats, texs, build_bvh=False)
    fresh.upload_from_triangles(0)
    assert _layout(rrt, h)[2] == _layout(rrt, fresh._handle)[2]
    i1, i2 = sc.info(), fresh.info()
    for k in ("n_tris", "n_nodes", "n_pair_records", "max_leaf", "geometry_bytes", "built_on_device"):
        assert i1[k] == i2[k], k
    assert inf.n_tris == len(new) and inf.n_nodes == i2["n_nodes"] and inf.n_pair_records == i2["n_pair_records"]
    nodes = np.zeros(2 * len(new), dtype=L.NODE)
    order = np.zeros(len(new), dtype=np.uint32)
    cnt = C.c_uint32()
    assert lib.mipt_scene_get_bvh(h, L.ptr(nodes), len(nodes), C.byref(cnt), L.ptr(order)) == 0
    host = rrt.Scene.from_arrays(new, mats, texs)                      # mipt_bvh_build
    assert refit_model.same_nodes(nodes[: cnt.value], host.bvh_nodes) and new[order].tobytes() == host.tris.tobytes()
    # the frame; MIPT_FLAG_TOUCHED's lazily allocated bitmap (sized by the old geometry before the update) follows the new size
    _oracle_check(rrt, orc, sc, new[order], nodes[: cnt.value])
    fresh.set_camera(sc.camera)
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=4, output_image_dimensions=(32, 18), output_image_path="/dev/null"))
    _, _, st = r.render_buffers(sc, flags=L.FLAG_COUNT | L.FLAG_TOUCHED)
    _, _, st2 = r.render_buffers(fresh, flags=L.FLAG_COUNT | L.FLAG_TOUCHED)
    assert st["touched_lines"] == st2["touched_lines"]


@pytest.mark.parametrize("kind", ["host", "device"])
def test_errors_leave_the_scene_untouched(rrt, kind):
    from rust_ray_tracing_amd import _lib as L
    tris, mats, texs, cam = _case("helmet")
    sc = _make(rrt, tris, mats, texs, cam, kind)
    h = sc._handle
    lib = rrt.load()
    src = np.empty_like(sc.tris)
    if sc._tri_order is not None:
        src[sc._tri_order] = sc.tris
    else:
        src[:] = sc.tris
    before = _layout(rrt, h)
    f0, _, _ = _render(rrt, sc)

    def bad(mutate, mode, status, words):
        t = src.copy()
        mutate(t)
        rc = lib.mipt_scene_update_triangles(h, L.ptr(t), len(t), mode, None)
        assert rc == status, (rc, lib.mipt_last_error())
        assert words in lib.mipt_last_error()
        assert _layout(rrt, h)[2] == before[2]
        f, _, _ = _render(rrt, sc)
        assert np.array_equal(f.view(np.uint32), f0.view(np.uint32))

    n_mat = len(sc.materials)
    for mode in (0, 1):
        bad(lambda t: t["material_id"].__setitem__(len(t) // 2, n_mat), mode, L.ERR_INVALID_ARG, b"material_id")
        if mode == 0:                                                 # (BVH::build itself is not fed infinities: the reference's binning is undefined there)
            bad(lambda t: t["vertices"]["position"].__setitem__((7, 1, 2), np.inf), mode, L.ERR_SCENE_LIMIT, b"2^40")
        bad(lambda t: t["vertices"]["position"].__setitem__((3, 0, 0), np.float32(3e12)), mode, L.ERR_SCENE_LIMIT, b"2^40")
    rc = lib.mipt_scene_update_triangles(h, L.ptr(src), len(src) - 1, 0, None)
    assert rc == L.ERR_INVALID_ARG and b"REFIT" in lib.mipt_last_error()
    assert lib.mipt_scene_update_triangles(h, L.ptr(src), len(src), 2, None) == L.ERR_INVALID_ARG
    assert lib.mipt_scene_update_triangles(h, None, len(src), 0, None) == L.ERR_INVALID_ARG
    assert _layout(rrt, h)[2] == before[2]


def test_sequences_and_memory(rrt):
    import torch
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth
    tris, mats, texs, cam = synth.make_scene("atrium", n_target=200000, tex_size=16)
    sc = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    h = sc.upload_from_triangles(0)                                    # tris stay in the caller's order
    lib = rrt.load()
    n_rec = sc.info()["n_pair_records"]
    cur = sc.tris.copy()
    for i in range(10):
        cur = _deform(cur, "jitter", 200 + i)
        assert lib.mipt_scene_update_triangles(h, L.ptr(cur), len(cur), 0, None) == 0, lib.mipt_last_error()
    assert lib.mipt_scene_update_triangles(h, L.ptr(cur), len(cur), 1, None) == 0
    assert lib.mipt_scene_update_triangles(h, L.ptr(cur), len(cur), 0, None) == 0
    fresh = rrt.Scene.from_arrays(cur, mats, texs, build_bvh=False)
    fresh.upload_from_triangles(0)
    n_rec = fresh.info()["n_pair_records"]
    _same_layout(_layout(rrt, h), _layout(rrt, fresh._handle), n_rec, "10 refits + rebuild + refit")
    fresh.release()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for i in range(20):
        cur = _deform(cur, "jitter", 300 + i)
        assert lib.mipt_scene_update_triangles(h, L.ptr(cur), len(cur), 1 if i % 5 == 4 else 0, None) == 0
    assert lib.mipt_scene_update_triangles(h, L.ptr(cur), len(cur), 0, None) == 0   # ends with the plan cached, as at free0
    free1 = torch.cuda.mem_get_info(0)[0]
    geom = sc.info()["geometry_bytes"]
    assert free0 - free1 < geom, f"{(free0 - free1) / 2**20:.1f} MiB more in use after 21 updates (geometry: {geom / 2**20:.1f} MiB)"


def test_failed_calls_give_their_memory_back(rrt):
    """Every call the library refuses -- by a check in its own kernels or host code, late enough that its device buffers exist --
    frees what it allocated: after eight refusals of each kind free device memory has fallen by less than ONE triangle array
    (n_tris x 112 B; a call that kept its triangles, or any of its larger builder buffers, would lose that much per call)."""
    import torch
    import mesh_model
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth
    lib = rrt.load()
    tris, mats, texs, cam = synth.make_scene("atrium", n_target=200000, tex_size=16)
    sc = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    h = sc.upload_from_triangles(0)                                    # tris stay in the caller's order
    good = sc.tris.copy()
    n, one_array = len(good), len(good) * 112
    bad_mat, far = good.copy(), good.copy()
    bad_mat["material_id"][n // 2] = len(mats)
    far["vertices"]["position"][n // 3, 1, 0] = np.float32(3e12)
    mesh, _ = mesh_model.mesh_from_triangles(good, 6)
    bad_mesh = dict(mesh, indices=mesh["indices"].copy())
    bad_mesh["indices"][bad_mesh["indices"].size // 2] = len(mesh["positions"])
    nodes = np.zeros(2 * n, dtype=L.NODE)
    n_nodes = C.c_uint32(0)

    def create(t):
        s = rrt.Scene.from_arrays(t, mats, texs, build_bvh=False)
        d, out = s.desc(), C.c_void_p(0x1234)
        rc = lib.mipt_scene_create_from_triangles(C.byref(d), 0, C.byref(out))
        assert rc != 0 and out.value is None
        return rc

    def create_mesh():
        s = rrt.Scene.from_mesh(materials=mats, textures=texs, **bad_mesh)
        d, md, out = s.desc(), s.mesh_desc(), C.c_void_p(0x1234)
        rc = lib.mipt_scene_create_from_mesh(C.byref(d), C.byref(md), 0, C.byref(out))
        assert rc != 0 and out.value is None
        return rc

    def build(cap):
        t = good.copy()                                                # a successful build reorders its triangles in place
        return lib.mipt_bvh_build_device(L.ptr(t), n, L.ptr(nodes), cap, C.byref(n_nodes), 0, None)

    # every kind of call once with success first: what a process pays once (streams, kernels, the scene's cached REFIT plan) is paid
    warm = rrt.Scene.from_arrays(good, mats, texs, build_bvh=False)
    warm.upload_from_triangles(0)
    warm.release()
    warm = rrt.Scene.from_mesh(materials=mats, textures=texs, **mesh)
    warm.upload_from_mesh(0)
    warm.release()
    assert build(len(nodes)) == 0, lib.mipt_last_error()
    cap_short = n_nodes.value - 1
    assert lib.mipt_scene_update_triangles(h, L.ptr(good), n, 1, None) == 0, lib.mipt_last_error()
    assert lib.mipt_scene_update_triangles(h, L.ptr(good), n, 0, None) == 0, lib.mipt_last_error()
    cases = [
        ("create, material_id out of range", lambda: create(bad_mat), L.ERR_INVALID_ARG, b"material_id"),
        ("create, coordinate 3e12", lambda: create(far), L.ERR_SCENE_LIMIT, b"2^40"),
        ("REFIT, material_id out of range", lambda: lib.mipt_scene_update_triangles(h, L.ptr(bad_mat), n, 0, None), L.ERR_INVALID_ARG, b"material_id"),
        ("REBUILD, material_id out of range", lambda: lib.mipt_scene_update_triangles(h, L.ptr(bad_mat), n, 1, None), L.ERR_INVALID_ARG, b"material_id"),
        ("REFIT, coordinate 3e12", lambda: lib.mipt_scene_update_triangles(h, L.ptr(far), n, 0, None), L.ERR_SCENE_LIMIT, b"2^40"),
        ("REBUILD, coordinate 3e12", lambda: lib.mipt_scene_update_triangles(h, L.ptr(far), n, 1, None), L.ERR_SCENE_LIMIT, b"2^40"),
        ("create from mesh, position index out of range", create_mesh, L.ERR_INVALID_ARG, b"index entry"),
        ("mipt_bvh_build_device, nodes_cap one short", lambda: build(cap_short), L.ERR_INVALID_ARG, b"nodes_cap"),
    ]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for what, call, status, words in cases:
        for _ in range(8):
            rc = call()
            assert rc == status and words in lib.mipt_last_error(), (what, rc, lib.mipt_last_error())
        torch.cuda.synchronize()
        lost = free0 - torch.cuda.mem_get_info(0)[0]
        print(f"{what}: {lost / 2**20:.1f} MiB less free than at the start (one triangle array: {one_array / 2**20:.1f} MiB)")
        assert lost < one_array, f"{what}: {lost / 2**20:.1f} MiB lost after 8 refused calls (one triangle array: {one_array / 2**20:.1f} MiB)"
    assert lib.mipt_scene_update_triangles(h, L.ptr(good), n, 0, None) == 0, lib.mipt_last_error()   # and the scene still takes an update


def test_destroy_gives_the_workspace_back(rrt):
    """mipt_scene_destroy frees the workspace a scene has grown, not only its geometry: a scene is created, renders 512 x 512 with
    RGBA8 (the frame buffers), answers 2^18 host rays (the staging pair), bakes 512 x 512 texels and gathers at their 2^18 points (the
    bake buffers, the triangle map) and is destroyed.  After eight such cycles free device memory has fallen by less than the
    smallest of those buffers, the 1 MiB RGBA8 frame: one buffer left behind per destroy would lose eight times its size."""
    import torch
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth
    tris, mats, texs, cam = synth.make_scene("cornell")
    n = 1 << 18
    rng = np.random.default_rng(11)
    rays = np.zeros(n, dtype=L.RAY)
    rays["origin"], rays["t_max"] = np.asarray(cam[0], dtype=np.float32), 1e30
    rays["direction"] = rng.standard_normal((n, 3)).astype(np.float32)
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=3, output_image_dimensions=(512, 512), output_image_path="/dev/null"))

    def cycle():
        sc = rrt.Scene.from_arrays(tris, mats, texs)
        sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
        sc.upload(0)
        _, rgba, _ = r.render_buffers(sc, want_rgba8=True)
        assert rgba.size == 512 * 512 * 4
        hits, _ = sc.query_closest(rays)
        assert hits["hit"].any()
        points, info = sc.bake_texels(512, 512)
        assert len(points) == n
        rad, _ = sc.bake_gather(points, samples=1)
        assert rad.shape == (n, 3)
        sc.release()

    cycle()                                                            # what a process pays once (kernels, streams) is paid
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(8):
        cycle()
    torch.cuda.synchronize()
    lost = free0 - torch.cuda.mem_get_info(0)[0]
    print(f"{lost / 2**20:.2f} MiB less free after 8 create ... destroy cycles")
    assert lost < 1 << 20, f"{lost / 2**20:.2f} MiB lost after 8 create ... destroy cycles (the RGBA8 frame: 1 MiB)"


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("from_triangles", [True, False])
def test_multi_replicas_follow_the_root(rrt, ranks, from_triangles):
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth
    mt = L.load_multitest()
    tris, mats, texs, cam = synth.make_scene("atrium", n_target=20000, tex_size=16)
    sc = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=not from_triangles)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    d = sc.desc()
    m = C.c_void_p()
    create = mt.mipt_multi_create_from_triangles if from_triangles else mt.mipt_multi_create
    assert create(C.byref(d), (C.c_int * ranks)(*([0] * ranks)), ranks, C.byref(m)) == 0, mt.mipt_last_error()
    single = rrt.Scene.from_arrays(sc.tris, mats, texs, build_bvh=False)
    single.bvh_nodes = sc.bvh_nodes.copy()
    single.set_camera(sc.camera)
    (single.upload_from_triangles(0) if from_triangles else single.upload(0))
    w, hh, spp, depth = 96, 54, 2, 6
    host_nodes = sc.bvh_nodes.copy()
    try:
        cur = sc.tris.copy()
        for step, mode in enumerate((0, 1, 0)):
            cur = _deform(cur, "rigid" if mode else "jitter", 400 + step)
            if mode == 1:
                cur = cur[: len(cur) - 777].copy()
            inf = L.MiptUpdateInfo()
            assert mt.mipt_multi_update_triangles(m, L.ptr(cur), len(cur), mode, C.byref(inf)) == 0, mt.mipt_last_error()
            assert rrt.load().mipt_scene_update_triangles(single._handle, L.ptr(cur), len(cur), mode, None) == 0
            hashes = {_layout(rrt, mt.mipt_multi_scene(m, i))[2] for i in range(ranks)}
            assert hashes == {_layout(rrt, single._handle)[2]}, f"step {step}: replicas differ"
            opt = rrt.make_options(w, hh, spp, depth, flags=L.FLAG_COUNT)
            ref = np.zeros((hh, w, 3), dtype=np.float32)
            st1 = L.MiptStats()
            assert rrt.load().mipt_render(single._handle, L.ptr(sc.camera.uniform), C.byref(opt), L.ptr(ref), None, C.byref(st1)) == 0
            # a multi made afresh from the tree the scene now holds (SAMPLES: the reduction order depends on the rank count)
            nodes = np.zeros(2 * len(cur), dtype=L.NODE)
            order = np.zeros(len(cur), dtype=np.uint32)
            cnt = C.c_uint32()
            if rrt.load().mipt_scene_get_bvh(single._handle, L.ptr(nodes), len(nodes), C.byref(cnt), L.ptr(order)) == 0:
                tree_tris, tree_nodes = cur[order], nodes[: cnt.value].copy()
            else:                                                     # host-built nodes, refit
                tree_tris, tree_nodes = cur, refit_model.refit(host_nodes, cur)
            fd = L.MiptSceneDesc(L.ptr(tree_tris), len(tree_tris), L.ptr(tree_nodes), len(tree_nodes), d.materials, d.n_materials, d.textures, d.n_textures)
            m2 = C.c_void_p()
            assert mt.mipt_multi_create(C.byref(fd), (C.c_int * ranks)(*([0] * ranks)), ranks, C.byref(m2)) == 0, mt.mipt_last_error()
            try:
                for mmode in (L.MULTI_TILES, L.MULTI_SAMPLES):
                    hdr = np.zeros((hh, w, 3), dtype=np.float32)
                    hdr2 = np.zeros((hh, w, 3), dtype=np.float32)
                    st = L.MiptMultiStats()
                    assert mt.mipt_render_multi(m, L.ptr(sc.camera.uniform), C.byref(opt), mmode, L.ptr(hdr), None, C.byref(st)) == 0, mt.mipt_last_error()
                    assert mt.mipt_render_multi(m2, L.ptr(sc.camera.uniform), C.byref(opt), mmode, L.ptr(hdr2), None, None) == 0, mt.mipt_last_error()
                    assert np.array_equal(hdr.view(np.uint32), hdr2.view(np.uint32)), f"step {step} mode {mmode}: differs from a fresh multi"
                    if mmode == L.MULTI_TILES:
                        assert np.array_equal(hdr.view(np.uint32), ref.view(np.uint32)) and st.total.rays == st1.rays
            finally:
                mt.mipt_multi_destroy(m2)
    finally:
        mt.mipt_multi_destroy(m)
