"""GPU: mipt_query_closest / mipt_query_occluded (csrc/ray_query.hip) against the model of tests/tools/query_model.py, which is held
to the oracle by tests/test_query_model.py.  Every comparison is bit for bit on the MiptHit words (and, with MIPT_FLAG_COUNT, on the
five counters); the distinct rays are few enough for the Python model, and batches larger than one launch holds in flight
repeat a modelled pool."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mesh_model  # noqa: E402
import query_model as Q  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 64, 48
SAFE = 0.0078125
REF, CULL = 0, 1
ARMS = [(REF, 0.0), (CULL, 0.0), (CULL, SAFE)]


def _make(rrt, kind):
    from rust_ray_tracing_amd import synth
    kw = dict(n_target=2000, tex_size=32) if kind == "helmet" else {}
    return synth.make_scene(kind, **kw)


def _host_scene(rrt, kind):
    tris, mats, texs, cam = _make(rrt, kind)
    sc = rrt.Scene.from_arrays(tris, mats, texs)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    return sc


_cache = {}


def _case(rrt, orc, kind):
    """(resident host-built Scene, path rays, {arm: model (hits, occ, counters)}) -- computed once per scene and left unchanged"""
    if kind not in _cache:
        sc = _host_scene(rrt, kind)
        rays, _, _ = Q.oracle_path_rays(orc, sc, W, H, np.linspace(0, W * H - 1, 40).astype(np.int64), spp=2, depth=8)
        ref = {arm: Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays, cull=arm[0] == CULL, margin=arm[1]) for arm in ARMS}
        sc.upload(0)
        _cache[kind] = (sc, rays, ref)
    return _cache[kind]


def _dev(rays):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).cuda()


def _closest(sc, rays, arm=(REF, 0.0), count=True, device=False, handle=None, stream=None):
    """-> (HIT records, stats) through the host or the device entry"""
    raw, st = sc._query(False, _dev(rays) if device else rays, None, arm[0], arm[1], count, handle, stream)
    if device:
        raw = raw.cpu().numpy().view(Q.HIT).reshape(-1)
    return raw, st


def _occluded(sc, rays, arm=(REF, 0.0), count=True, device=False, handle=None):
    raw, st = sc._query(True, _dev(rays) if device else rays, None, arm[0], arm[1], count, handle, None)
    return (raw.cpu().numpy() if device else raw), st


def _same_counters(st, model):
    return {k: st[k] for k in Q.COUNTERS} == {k: model[k] for k in Q.COUNTERS}


def _nan_canonical(h):
    """IEEE 754 leaves the sign and payload of a NaN an operation PRODUCES to the implementation (x86 SSE and gfx950 differ): NaNs
    are compared as NaNs, everything else bit for bit"""
    w = np.ascontiguousarray(h).view(np.uint32).reshape(-1, 4).copy()
    f = w[:, :3].view(np.float32)
    w[:, :3][np.isnan(f)] = 0x7FC00000
    return w


# ---- path rays: both arms, both entries, scenes made three ways ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cornell", "helmet"])
@pytest.mark.parametrize("arm", ARMS)
def test_path_rays_both_entries(rrt, orc, kind, arm):
    sc, rays, ref = _case(rrt, orc, kind)
    hits, _, counters = ref[arm]
    for device in (False, True):
        got, st = _closest(sc, rays, arm, count=True, device=device)
        assert Q.same_bits(got, hits), (kind, arm, device)
        assert _same_counters(st, counters), (st, counters)
        assert st["kernel_ms"] > 0 and st["stack_overflows"] == 0 and st["texel_fetches"] == 0 and st["pixels"] == 0 and not any(st["diag"])
        got, st = _closest(sc, rays, arm, count=False, device=device)          # the production instantiation
        assert Q.same_bits(got, hits), (kind, arm, device)
        assert st["rays"] == 0 and st["tri_tests"] == 0 and st["kernel_ms"] > 0


@pytest.mark.parametrize("how", ["from_triangles", "from_mesh"])
def test_prim_is_the_callers_index_on_device_built_scenes(rrt, orc, how):
    tris, mats, texs, cam = _make(rrt, "helmet")
    if how == "from_triangles":
        sc = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
        sc.upload_from_triangles(0, fetch_bvh=True)
        caller = tris
    else:
        mesh, perm = mesh_model.mesh_from_triangles(tris, 4)
        sc = rrt.Scene.from_mesh(materials=mats, textures=texs, **mesh)
        sc.upload_from_mesh(0, fetch_bvh=True)
        caller = tris[perm]
    order = sc._tri_order                                   # mipt_scene_get_bvh: tree triangle t = caller's triangle order[t]
    assert order is not None and not np.array_equal(order, np.arange(len(order)))
    assert np.array_equal(sc.tris.view(np.uint8), np.ascontiguousarray(caller)[order].view(np.uint8))
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    rays, _, _ = Q.oracle_path_rays(orc, sc, W, H, np.linspace(0, W * H - 1, 24).astype(np.int64), spp=2, depth=6)
    for arm in (ARMS[0], ARMS[2]):
        hits, _, counters = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays, cull=arm[0] == CULL, margin=arm[1], tri_order=order)
        assert np.any(hits["prim"] != Q.NONE)
        for device in (False, True):
            got, st = _closest(sc, rays, arm, device=device)
            assert Q.same_bits(got, hits) and _same_counters(st, counters), (how, arm, device)


# ---- ray counts: partial waves, the refill, the tail; nothing is written past the end ---------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_ray_counts_and_sentinel(rrt, orc, n):
    import torch
    from rust_ray_tracing_amd import _lib as L
    sc, rays, ref = _case(rrt, orc, "cornell")
    idx = (np.arange(n) * 7 + 3) % len(rays)                 # a fixed pick from the pool, repeated as needed
    r, want = np.ascontiguousarray(rays[idx]), ref[ARMS[0]][0][idx]
    want_occ = ref[ARMS[0]][1][idx]
    lib = rrt.load()
    opt = L.MiptQueryOptions()
    # host entry: the caller's buffer has one more record, which must stay as it is
    out = np.full(n + 1, 0xA5A5A5A5, dtype=np.uint32).repeat(4).view(Q.HIT)
    assert lib.mipt_query_closest(sc._handle, L.ptr(r), n, C.byref(opt), L.ptr(out), None) == 0
    assert Q.same_bits(out[:n], want) and np.all(out[n:].view(np.uint32) == 0xA5A5A5A5)
    occ = np.full(n + 16, 0x5A, dtype=np.uint8)
    assert lib.mipt_query_occluded(sc._handle, L.ptr(r), n, C.byref(opt), L.ptr(occ), None) == 0
    assert np.array_equal(occ[:n], want_occ) and np.all(occ[n:] == 0x5A)
    # device entry: the same with the sentinel in device memory
    d_r = _dev(r)
    d_out = torch.full((n + 1, 4), 0x25A5A5A5, dtype=torch.int32, device="cuda")
    d_occ = torch.full((n + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    assert lib.mipt_query_closest_device(sc._handle, d_r.data_ptr(), n, C.byref(opt), d_out.data_ptr(), None, None) == 0
    assert lib.mipt_query_occluded_device(sc._handle, d_r.data_ptr(), n, C.byref(opt), d_occ.data_ptr(), None, None) == 0
    h_out, h_occ = d_out.cpu().numpy(), d_occ.cpu().numpy()
    assert Q.same_bits(h_out[:n].view(Q.HIT).reshape(-1), want) and np.all(h_out[n:] == 0x25A5A5A5)
    assert np.array_equal(h_occ[:n], want_occ) and np.all(h_occ[n:] == 0x5A)


# ---- batches larger than one launch holds in flight: the refill into a partly busy wave -----------------------------------------------
# query_launch sizes the grid as min(n_cu * blocks_per_cu, ceil(n / 256)) blocks of 256 lanes, so up to grid * 256 rays every wave
# takes its rays in its first fetch and every later refill only retires lanes.  blocks_per_cu is what the occupancy query returns,
# clamped to 8 by query_blocks_per_cu (ray_query.hip): more than n_cu * 8 * 256 rays exceed the launch whatever that query says.
# The model cannot trace a million rays and need not: a ray's answer and counts do not depend on scheduling, so the batch is a pool
# of a few hundred modelled rays gathered through Q.tiled (48 short and 16 long rays in any 64 consecutive positions), which
# tests/test_query_model.py shows to refill waves whose other lanes are mid-traversal.
BLOCKS_PER_CU_CAP, BLOCK_LANES = 8, 256
BIG = [(2, 77), (1, 1)]                        # n = k * n_cu * 8 * 256 + extra: several refills per wave and a ragged tail; the queue
                                               # runs out inside a refill (one lane gets a ray, its neighbours retire)


def _launch_capacity():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * BLOCKS_PER_CU_CAP * BLOCK_LANES


_pools = {}


def _pool(rrt, orc, which):
    """(resident Scene, {(arm, anyhit): (rays, model hits, model occ, per-ray counters, classes)}, filled on demand and left unchanged)"""
    if which not in _pools:
        if which == "helmet":                                                  # host-built: the scene of _case
            sc = _case(rrt, orc, "helmet")[0]
            pool = Q.refill_pool(orc, sc)
        elif which == "helmet-device":                                         # built on the device: prim goes through tri_order
            tris, mats, texs, cam = _make(rrt, "helmet")
            sc = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
            sc.upload_from_triangles(0, fetch_bvh=True)
            sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
            pool = Q.refill_pool(orc, sc)
        else:
            from test_gpu_batch import _chain_bvh
            sc = _chain_bvh(rrt, 40)                                           # stack occupancy 40: 16 in LDS, the rest spilled
            sc.upload(0)
            pool = Q.chain_rays()
        _pools[which] = (sc, pool, {})
    return _pools[which]


def _pool_model(rrt, orc, which, arm, anyhit):
    sc, pool, models = _pool(rrt, orc, which)
    if (arm, anyhit) not in models:
        kw = dict(cull=arm[0] == CULL, margin=arm[1], tri_order=sc._tri_order)
        rays = pool
        if anyhit:
            rays = Q.occlusion_t_max(pool, _pool_model(rrt, orc, which, ARMS[0], False)[2])
        hits, occ, per = Q.per_ray(orc.load(), sc.tris, sc.bvh_nodes, rays, anyhit=anyhit, **kw)
        n_steps = Q.steps(per)
        classes = Q.classify(n_steps)
        if which == "helmet-device":                                           # this tree exists only here: the other pools are
            Q.refill_conditions(n_steps, classes)                              # held to the conditions by tests/test_query_model.py
        models[arm, anyhit] = (sc, rays, hits, occ, per, classes)
    return models[arm, anyhit]


def _big_query(rrt, sc, rays, d_rays, n, arm, anyhit, count, device):
    """One call of the C entry with a sentinel behind the output -> (HIT records or occlusion bytes [n], stats dict)"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    opt = L.MiptQueryOptions()
    opt.traversal, opt.cull_margin, opt.flags = arm[0], arm[1], (L.FLAG_COUNT if count else 0)
    st = L.MiptStats()
    if device:                                                                 # one extra MiptHit / 16 extra bytes keep their pattern
        if anyhit:
            d_out = torch.full((n + 16,), 0x5A, dtype=torch.uint8, device="cuda")
            rc = lib.mipt_query_occluded_device(sc._handle, d_rays.data_ptr(), n, C.byref(opt), d_out.data_ptr(), None, C.byref(st))
        else:
            d_out = torch.full((n + 1, 4), 0x25A5A5A5, dtype=torch.int32, device="cuda")
            rc = lib.mipt_query_closest_device(sc._handle, d_rays.data_ptr(), n, C.byref(opt), d_out.data_ptr(), None, C.byref(st))
        out = d_out.cpu().numpy()
        assert rc == 0 and np.all(out[n:] == (0x5A if anyhit else 0x25A5A5A5)), (rc, arm, anyhit, count)
        return (out[:n] if anyhit else out[:n].view(Q.HIT).reshape(-1)), st.as_dict()
    if anyhit:                                                                 # the caller's buffer is longer than n and stays so
        out = np.full(n + 16, 0x5A, dtype=np.uint8)
        rc = lib.mipt_query_occluded(sc._handle, L.ptr(rays), n, C.byref(opt), L.ptr(out), C.byref(st))
        assert rc == 0 and np.all(out[n:] == 0x5A), (rc, arm, count)
    else:
        out = np.full(4 * (n + 1), 0xA5A5A5A5, dtype=np.uint32).view(Q.HIT)
        rc = lib.mipt_query_closest(sc._handle, L.ptr(rays), n, C.byref(opt), L.ptr(out), C.byref(st))
        assert rc == 0 and np.all(out[n:].view(np.uint32) == 0xA5A5A5A5), (rc, arm, count)
    return out[:n], st.as_dict()


def _mismatch(got, want, idx):
    """for the message of a failed comparison: the first differing rays, their pool members and what was written"""
    g, w = np.ascontiguousarray(got).view(np.uint32).reshape(len(idx), -1), np.ascontiguousarray(want).view(np.uint32).reshape(len(idx), -1)
    bad = np.flatnonzero((g != w).any(axis=1))
    return [(int(i), int(idx[i]), g[i].tolist(), w[i].tolist()) for i in bad[:4]], len(bad)


def _check_big(rrt, orc, which, n, arm, anyhit, entries=(False, True)):
    sc, pool_rays, hits, occ, per, classes = _pool_model(rrt, orc, which, arm, anyhit)
    assert n > _launch_capacity()                                              # some wave gets a second block of real rays
    idx = Q.tiled(len(pool_rays), classes, n)
    rays = np.ascontiguousarray(pool_rays[idx])
    want = occ[idx] if anyhit else hits[idx]
    sums = {k: int(per[k][idx].sum()) for k in ("inner_steps", "tri_tests", "hits")}
    sums.update(rays=n, max_stack=int(per["max_stack"][idx].max()))
    assert np.all(per["stack_overflows"] == 0) and 0 < sums["hits"] < n
    d_rays = _dev(rays) if True in entries else None
    for device in entries:
        for count in (True, False):                                            # the counting twin, then the production instantiation
            got, st = _big_query(rrt, sc, rays, d_rays, n, arm, anyhit, count, device)
            same = np.array_equal(got, want) if anyhit else Q.same_bits(got, want)
            assert same, (which, n, arm, anyhit, device, count, _mismatch(got, want, idx))
            assert st["stack_overflows"] == 0 and st["kernel_ms"] > 0
            if count:
                assert {k: st[k] for k in Q.COUNTERS} == sums, (which, n, arm, anyhit, device, st, sums)
            else:
                assert st["rays"] == 0 and st["tri_tests"] == 0
    return sums


@pytest.mark.parametrize("size", BIG, ids=lambda s: "%dx+%d" % s)
@pytest.mark.parametrize("arm", ARMS)
def test_closest_hit_on_batches_larger_than_the_launch(rrt, orc, arm, size):
    _check_big(rrt, orc, "helmet", size[0] * _launch_capacity() + size[1], arm, False)


@pytest.mark.parametrize("size", BIG, ids=lambda s: "%dx+%d" % s)
@pytest.mark.parametrize("arm", [ARMS[0], ARMS[2]])
def test_occlusion_on_batches_larger_than_the_launch(rrt, orc, arm, size):
    _check_big(rrt, orc, "helmet", size[0] * _launch_capacity() + size[1], arm, True)


@pytest.mark.parametrize("anyhit", [False, True], ids=["closest", "occluded"])
def test_spilled_stacks_across_refills(rrt, orc, anyhit):
    """The chain tree: a long ray holds 40 stack entries, 24 of them in the lane's HBM spill slots, and an occluded one stops
    with them still stacked.  The lane's next ray, short or spilled, must not read its predecessor's entries."""
    sums = _check_big(rrt, orc, "chain", _launch_capacity() + 4099, ARMS[0], anyhit)
    assert sums["max_stack"] > 16


def test_renders_and_queries_share_one_spill_buffer(rrt):
    """Renders and queries of one scene spill into the same per-wave HBM stack slots, which grow with the launch's grid: a one-block
    render, a five-block query (the slots must grow), the render again, a one-block query.  Each call's result and counters are bit for
    bit those of the same call as the first on a fresh scene."""
    from test_gpu_batch import _chain_bvh
    from rust_ray_tracing_amd import _lib as L
    spilled = Q.chain_rays()[:70]                                              # the rays along +x: 40 stack entries each
    big, small = np.resize(spilled, 4 * 256 + 1), np.resize(spilled, 65)

    def render(sc):
        r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=3, output_image_dimensions=(8, 8), output_image_path="/dev/null"))
        hdr, _, st = r.render_buffers(sc, want_rgba8=False, flags=L.FLAG_COUNT)
        return hdr.view(np.uint32).copy(), st

    calls = [render, lambda sc: _closest(sc, big), render, lambda sc: _closest(sc, small)]

    def scene():
        sc = _chain_bvh(rrt, 40)
        sc.upload(0)
        return sc

    def counters(st):                                                          # all but the clock readings: kernel_ms and diag[7 .. 10]
        return dict({k: v for k, v in st.items() if k != "kernel_ms"}, diag=st["diag"][:7])

    shared = scene()
    for i, call in enumerate(calls):
        want, want_st = call(scene())
        got, got_st = call(shared)
        assert want_st["max_stack"] > 16 and want_st["stack_overflows"] == 0, (i, want_st)   # the call spills
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), i
        assert counters(got_st) == counters(want_st), (i, got_st, want_st)


def test_host_entries_share_their_staging(rrt, orc):
    """The host entries of the queries, the radiance queries and the bake stage their items and results in one pair of scene-owned
    buffers, which grow on demand, are reused while they are too large and change their element size from call to call (a byte, a
    16-byte hit or point, a 12-byte radiance; the texels stage no input at all).  Every call of the sequence on one handle returns,
    bit for bit, what the same call returns on a handle of the same scene that has seen no other call."""
    _, pool, _ = _case(rrt, orc, "cornell")

    def words(a):
        return np.ascontiguousarray(a).view(np.uint8)

    def closest(n):
        return lambda sc, _: words(sc._query(False, np.resize(pool, n), None, REF, 0.0, False, None, None)[0])

    def occluded(n):
        return lambda sc, _: words(sc.query_occluded(np.resize(pool, n))[0])

    def radiance(n):
        return lambda sc, _: words(sc.query_radiance(np.resize(pool, n), samples=2, max_ray_depth=4)[0])

    def texels(sc, _):
        return sc.bake_texels(8, 8)[0]

    def gather(n):
        return lambda sc, points: words(sc.bake_gather(points[:n])[0])

    calls = [occluded(1), closest(65), radiance(3), texels, gather(64), closest(1000), occluded(1000), radiance(257), gather(5)]
    shared = _host_scene(rrt, "cornell")
    shared.upload(0)
    points = None
    for i, call in enumerate(calls):
        fresh = _host_scene(rrt, "cornell")
        fresh.upload(0)
        want, got = call(fresh, points), call(shared, points)
        fresh.release()
        assert want.dtype == got.dtype and want.shape == got.shape and want.size > 0, i
        assert np.array_equal(words(got), words(want)), i
        if call is texels:
            points = got
            assert len(points) == 64
    shared.release()


def test_prim_through_tri_order_on_a_batch_larger_than_the_launch(rrt, orc):
    """A device-built scene: the hit's triangle goes through q.tri_order when the refill writes it, after neighbours were refilled"""
    sc, _, hits, _, _, classes = _pool_model(rrt, orc, "helmet-device", ARMS[2], False)
    order = sc._tri_order
    assert order is not None and not np.array_equal(order, np.arange(len(order)))
    hit = (hits["prim"] != Q.NONE) & (classes != Q.UNUSED)
    tree = Q.per_ray(orc.load(), sc.tris, sc.bvh_nodes, _pools["helmet-device"][1][hit], cull=True, margin=SAFE)[0]
    assert hit.sum() >= 16 and np.any(tree["prim"] != hits["prim"][hit])       # the permutation shows in the expected records
    _check_big(rrt, orc, "helmet-device", BIG[0][0] * _launch_capacity() + BIG[0][1], ARMS[2], False, entries=(True,))


# ---- degenerate scenes -----------------------------------------------------------------------------------------------------------
def _tri(rrt, p0, p1, p2):
    t = np.zeros(1, dtype=rrt.TRIANGLE)
    t["vertices"]["position"][0] = [p0, p1, p2]
    t["vertices"]["normal"] = (0, 0, 1)
    return t


def _fan_rays(n, seed, target=(0.3, 0.3, 0.0), spread=0.6):
    rng = np.random.default_rng(seed)
    o = np.tile(np.array([0.2, 0.1, 3.0], np.float32), (n, 1)) + rng.normal(0, 0.05, (n, 3)).astype(np.float32)
    d = (np.asarray(target, np.float32) + rng.normal(0, spread, (n, 3)).astype(np.float32)) - o
    return Q.make_rays(o, d.astype(np.float32))


@pytest.mark.parametrize("n_tris", [1, 2])
def test_one_and_two_triangles(rrt, orc, n_tris):
    tris = np.concatenate([_tri(rrt, (0, 0, 0), (1, 0, 0), (0, 1, 0)), _tri(rrt, (0, 0, -1), (0, 1, -1), (1, 0, -1))][:n_tris])
    sc = rrt.Scene.from_arrays(tris, [rrt.material_default()])
    if n_tris == 1:
        assert len(sc.bvh_nodes) == 1                                          # the root is the leaf
    sc.upload(0)
    rays = _fan_rays(130, 5)
    for arm in ARMS:
        hits, occ, counters = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays, cull=arm[0] == CULL, margin=arm[1])
        assert 0 < occ.sum() < len(rays)
        got, st = _closest(sc, rays, arm)
        assert Q.same_bits(got, hits) and _same_counters(st, counters), arm
        _, occ_m, counters_m = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays, cull=arm[0] == CULL, margin=arm[1], anyhit=True)
        got, st = _occluded(sc, rays, arm)
        assert np.array_equal(got, occ_m) and _same_counters(st, counters_m), arm


def test_big_leaf_of_coincident_triangles_keeps_the_first(rrt, orc):
    """A leaf of 70 coincident triangles behind a nearer leaf whose triangle the rays miss: the big leaf is pushed in the child-ref
    form, re-read on the pop, and the tie goes to the first triangle in visit order."""
    from rust_ray_tracing_amd import NODE
    near = _tri(rrt, (5, 0.8, 0.8), (5, 1, 0.8), (5, 0.8, 1))                   # in a corner of its box: rays along the axis miss it
    big = np.repeat(_tri(rrt, (10, -1, -1), (10, 1, -1), (10, 0, 1)), 70)
    tris = np.concatenate([near, big])
    nodes = np.zeros(3, dtype=NODE)
    nodes[0]["bounds_min"], nodes[0]["bounds_max"], nodes[0]["first_tri_or_child"] = (5, -1, -1), (10, 1, 1), 1
    nodes[1]["bounds_min"], nodes[1]["bounds_max"] = (5, -1, -1), (5, 1, 1)
    nodes[1]["first_tri_or_child"], nodes[1]["num_tris"] = 0, 1
    nodes[2]["bounds_min"], nodes[2]["bounds_max"] = (10, -1, -1), (10, 1, 1)
    nodes[2]["first_tri_or_child"], nodes[2]["num_tris"] = 1, 70
    sc = rrt.Scene.from_arrays(tris, [rrt.material_default()], build_bvh=False)
    sc.bvh_nodes = nodes
    sc.upload(0)
    rng = np.random.default_rng(11)
    o = np.zeros((40, 3), np.float32)
    o[:, 1:] = rng.uniform(-0.3, 0.3, (40, 2))
    rays = Q.make_rays(o, np.tile(np.float32([1, 0, 0]), (40, 1)))
    for arm in ARMS:
        hits, _, counters = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays, cull=arm[0] == CULL, margin=arm[1])
        assert np.all(hits["prim"] & 0x01FFFFFF == 1)                          # the first of the seventy
        got, st = _closest(sc, rays, arm)
        assert Q.same_bits(got, hits) and _same_counters(st, counters), arm


def test_deep_trees_spill_and_overflow(rrt, orc):
    from test_gpu_batch import _chain_bvh
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    rng = np.random.default_rng(3)
    o = np.zeros((70, 3), np.float32)
    o[:, 1:] = rng.uniform(-0.2, 0.2, (70, 2))
    rays = Q.make_rays(o, np.tile(np.float32([1, 0, 0]), (70, 1)))
    sc = _chain_bvh(rrt, 40)                                                   # stack occupancy 40: 16 in LDS, the rest spilled
    sc.upload(0)
    hits, _, counters = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays)
    assert counters["max_stack"] > 16 and np.all(hits["prim"] != Q.NONE)
    got, st = _closest(sc, rays)
    assert Q.same_bits(got, hits) and _same_counters(st, counters)
    _, occ_m, counters_m = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays, anyhit=True)
    got, st = _occluded(sc, rays)
    assert np.array_equal(got, occ_m) and _same_counters(st, counters_m)
    deep = _chain_bvh(rrt, 120)                                                # deeper than the 64-entry stack
    dh = deep.upload(0)
    model_c = {}
    Q.traverse(orc.load(), deep.tris, deep.bvh_nodes, rays[0], counters=model_c)
    assert model_c.get("stack_overflows", 0) > 0
    out = np.full(4 * len(rays), 0xA5A5A5A5, dtype=np.uint32).view(Q.HIT)
    stt = L.MiptStats()
    opt = L.MiptQueryOptions()
    assert lib.mipt_query_closest(dh, L.ptr(rays), len(rays), C.byref(opt), L.ptr(out), C.byref(stt)) == L.ERR_STACK
    assert stt.stack_overflows > 0 and "stack" in lib.mipt_last_error().decode()
    assert not np.any(out.view(np.uint32) == 0xA5A5A5A5)                       # the results were written all the same
    got, st = _closest(sc, rays)                                               # a normal scene queries as before
    assert Q.same_bits(got, hits) and st["stack_overflows"] == 0


# ---- hard rays: the model decides ------------------------------------------------------------------------------------------------
def test_hard_rays(rrt, orc):
    sc, path, ref = _case(rrt, orc, "helmet")
    tris, nodes = sc.tris, sc.bvh_nodes
    rng = np.random.default_rng(7)
    eye = np.float32([3.0, 0.55, 0.0])
    P = tris["vertices"]["position"]
    pick = rng.choice(len(tris) - 2, 24, replace=False)
    o, d, tm = [], [], []

    def add(oo, dd, t=1e30):
        o.append(np.asarray(oo, np.float32)); d.append(np.asarray(dd, np.float32)); tm.append(np.float32(t))
    for k, special in enumerate([0.0, -0.0, 2.0 ** -70, 4.0]):                  # components outside ray_safe's fast path
        for axis in range(3):
            dd = np.float32([-1.0, -0.1, 0.05])
            dd[axis] = special if axis else -abs(special)
            add(eye, dd)
            add(np.float32([0.1, 3.0, 0.1]), np.where(np.arange(3) == axis, np.float32(special), np.float32([0.01, -1.0, 0.02])))
    add(np.float32([2.0 ** 41, 0, 0]), (-1, 0, 0)); add(np.float32([0, 2.0 ** 41, 0.1]), (0, -1, 0))
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            dd = np.float32([-1.0, -0.1, 0.05]); dd[axis] = bad; add(eye, dd)
            oo = eye.copy(); oo[axis] = bad; add(oo, (-1.0, -0.1, 0.05))
    add(eye, (0, 0, 0)); add(eye, (-1, -0.1, 0.05), np.nan); add(eye, (-1, -0.1, 0.05), 0.0); add(eye, (-1, -0.1, 0.05), -1.0)
    for t in pick[:8]:                                                          # in the plane of a triangle (det = 0 up to rounding)
        v0, v1, v2 = P[t]
        add(v0 - (v1 - v0), (v1 - v0) + np.float32(0.5) * (v2 - v0))
    for t in pick:                                                              # through vertices and shared-edge midpoints of the mesh
        v0, v1, v2 = P[t]
        add(eye, v0 - eye); add(eye, (np.float32(0.5) * (v0 + v1)) - eye); add(eye, (np.float32(0.5) * (v1 + v2)) - eye)
    rays = Q.make_rays(np.stack(o), np.stack(d), np.array(tm, np.float32))
    # t_max equal to, one ulp above and one ulp below a hit's t
    hit = ref[ARMS[0]][0]["prim"] != Q.NONE
    base, t_hit = path[hit][:30], ref[ARMS[0]][0]["t"][hit][:30]
    edge = [base.copy(), base.copy(), base.copy()]
    edge[0]["t_max"], edge[1]["t_max"], edge[2]["t_max"] = t_hit, np.nextafter(t_hit, np.float32(np.inf)), np.nextafter(t_hit, np.float32(0))
    rays = np.concatenate([rays] + edge)
    with np.errstate(all="ignore"):
        for arm in ARMS:
            hits, _, counters = Q.query(orc.load(), tris, nodes, rays, cull=arm[0] == CULL, margin=arm[1])
            for device in (False, True):
                got, st = _closest(sc, rays, arm, device=device)
                assert np.array_equal(_nan_canonical(got), _nan_canonical(hits)), (arm, device, np.flatnonzero((_nan_canonical(got) != _nan_canonical(hits)).any(1)))
                assert _same_counters(st, counters), (arm, st, counters)
            _, occ_m, counters_m = Q.query(orc.load(), tris, nodes, rays, cull=arm[0] == CULL, margin=arm[1], anyhit=True)
            got, st = _occluded(sc, rays, arm)
            assert np.array_equal(got, occ_m) and _same_counters(st, counters_m), arm
    m = len(base)
    assert m >= 10
    e = ref[ARMS[0]][0][hit][:m]
    got, _ = _closest(sc, rays[len(rays) - 3 * m:])
    assert np.all(got["prim"][:m] == Q.NONE) and Q.same_bits(got[m:2 * m], e) and np.all(got["prim"][2 * m:] == Q.NONE)


def test_rays_through_shared_edges_and_vertices_of_a_grid_mesh(rrt, orc):
    """A 9 x 9-vertex height field of 128 triangles; rays aimed exactly at every vertex (shared by up to six triangles) and at the
    midpoint of every edge (shared by two), straight down (two zero direction components) and from an eye point."""
    k = 8
    gx, gy = np.meshgrid(np.arange(k + 1, dtype=np.float32), np.arange(k + 1, dtype=np.float32), indexing="ij")
    gz = (np.float32(0.25) * np.sin(gx * np.float32(0.9)) * np.cos(gy * np.float32(0.7))).astype(np.float32)
    V = np.stack([gx, gy, gz], axis=-1)
    tri_p, targets = [], [V.reshape(-1, 3)]
    for i in range(k):
        for j in range(k):
            a, b, c, d = V[i, j], V[i + 1, j], V[i + 1, j + 1], V[i, j + 1]
            tri_p += [(a, b, c), (a, c, d)]
            targets.append(np.float32(0.5) * np.stack([a + b, a + d, a + c, b + c, c + d]))      # edges incl. the shared diagonal
    tris = np.zeros(len(tri_p), dtype=rrt.TRIANGLE)
    tris["vertices"]["position"] = np.asarray(tri_p, dtype=np.float32)
    tris["vertices"]["normal"] = (0, 0, 1)
    sc = rrt.Scene.from_arrays(tris, [rrt.material_default()])
    sc.upload(0)
    T = np.concatenate(targets).astype(np.float32)
    down_o = T + np.float32([0, 0, 5])
    eye = np.float32([3.7, -2.1, 6.3])
    rays = np.concatenate([Q.make_rays(down_o, np.tile(np.float32([0, 0, -1]), (len(T), 1))),
                           Q.make_rays(np.tile(eye, (len(T), 1)), T - eye),
                           Q.make_rays(T - (T - eye) * np.float32(0.5), T - eye)])                   # from below the eye, un-normalised
    for arm in ARMS:
        hits, occ, counters = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays, cull=arm[0] == CULL, margin=arm[1])
        assert occ.sum() > len(rays) // 2
        for device in (False, True):
            got, st = _closest(sc, rays, arm, device=device)
            assert Q.same_bits(got, hits) and _same_counters(st, counters), (arm, device)
        _, occ_m, counters_m = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays, cull=arm[0] == CULL, margin=arm[1], anyhit=True)
        got, st = _occluded(sc, rays, arm)
        assert np.array_equal(got, occ_m) and _same_counters(st, counters_m), arm


# ---- occlusion -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cornell", "helmet"])
def test_occlusion_is_closest_t_below_t_max(rrt, orc, kind):
    sc, path, ref = _case(rrt, orc, kind)
    closest = ref[ARMS[0]][0]
    t = closest["t"].copy()
    factor = np.float32([0.5, 1.0, 2.0, 0.999, 1.001])[np.arange(len(t)) % 5]
    rays = path.copy()
    rays["t_max"] = t * factor
    rays["t_max"][3::7] = np.nextafter(t[3::7], np.float32(np.inf))
    rays["t_max"][5::7] = np.nextafter(t[5::7], np.float32(0))
    want = (closest["t"] < rays["t_max"]) & (closest["prim"] != Q.NONE)
    assert 0 < want.sum() < len(want)
    for arm in ARMS:
        _, occ_m, counters_m = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays, cull=arm[0] == CULL, margin=arm[1], anyhit=True)
        if arm[0] == REF:
            assert np.array_equal(occ_m != 0, want)
        for device in (False, True):
            got, st = _occluded(sc, rays, arm, device=device)
            assert np.array_equal(got, occ_m), (kind, arm, device)
            assert _same_counters(st, counters_m), (st, counters_m)           # the model's early-exit counts
            got, st = _occluded(sc, rays, arm, count=False, device=device)
            assert np.array_equal(got, occ_m) and st["rays"] == 0
    occ, _ = sc.query_occluded((np.ascontiguousarray(rays["origin"]), np.ascontiguousarray(rays["direction"])), t_max=rays["t_max"])
    assert occ.dtype == np.bool_ and np.array_equal(occ, want)


# ---- updates: queries see the geometry of the last successful update ---------------------------------------------------------------
def _render(rrt, sc):
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=3, output_image_dimensions=(32, 24), output_image_path="/dev/null"))
    return r.render_buffers(sc)[0].view(np.uint32).copy()


def test_queries_follow_refit_and_rebuild(rrt, orc):
    from rust_ray_tracing_amd import _lib as L
    sc = _host_scene(rrt, "helmet")
    sc.upload(0)
    rays, _, _ = Q.oracle_path_rays(orc, sc, W, H, np.linspace(0, W * H - 1, 16).astype(np.int64), spp=1, depth=5)
    before = _render(rrt, sc)
    hits0, _, c0 = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays)
    got, st = _closest(sc, rays)
    assert Q.same_bits(got, hits0) and _same_counters(st, c0)
    assert np.array_equal(_render(rrt, sc), before)                          # a query leaves the next render as it was
    # REFIT: squash the geometry, keep the tree
    sc.tris["vertices"]["position"][:, :, 1] *= np.float32(0.75)
    sc.update_device(L.UPDATE_REFIT)
    hits1, _, c1 = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays)
    assert not Q.same_bits(hits1, hits0)
    for arm in (ARMS[0], ARMS[2]):
        h, _, c = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays, cull=arm[0] == CULL, margin=arm[1])
        got, st = _closest(sc, rays, arm)
        assert Q.same_bits(got, h) and _same_counters(st, c), arm
    # REBUILD with a different triangle count: a new tree, prim in the order of the array just passed
    kept = np.ascontiguousarray(sc.tris[: len(sc.tris) - 37])
    sc.tris = kept.copy()
    sc.update_device(L.UPDATE_REBUILD)
    assert sc._tri_order is not None and len(sc.tris) == len(kept)
    assert np.array_equal(sc.tris.view(np.uint8), kept[sc._tri_order].view(np.uint8))
    for arm in (ARMS[0], ARMS[2]):
        h, _, c = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays, cull=arm[0] == CULL, margin=arm[1], tri_order=sc._tri_order)
        for device in (False, True):
            got, st = _closest(sc, rays, arm, device=device)
            assert Q.same_bits(got, h) and _same_counters(st, c), (arm, device)
    mid = _render(rrt, sc)
    _closest(sc, rays, count=False)
    assert np.array_equal(_render(rrt, sc), mid)


def test_queries_follow_set_transforms(rrt, orc):
    from rust_ray_tracing_amd import _lib as L
    tris, mats, texs, cam = _make(rrt, "helmet")
    mesh, perm = mesh_model.mesh_from_triangles(tris, 4)
    sc = rrt.Scene.from_mesh(materials=mats, textures=texs, **mesh)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    sc.upload_from_mesh(0, fetch_bvh=True)
    rays, _, _ = Q.oracle_path_rays(orc, sc, W, H, np.linspace(0, W * H - 1, 16).astype(np.int64), spp=1, depth=5)
    hits0, _, _ = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays, tri_order=sc._tri_order)
    n_parts = len(sc.mesh["parts"])
    xf = np.tile(np.eye(4, dtype=np.float32).reshape(16), (n_parts, 1))
    xf[:, 12:15] = np.random.default_rng(2).normal(0, 0.2, (n_parts, 3)).astype(np.float32)      # Mat4f data[col][row]: column 3 = translation
    for mode in (L.UPDATE_REFIT, L.UPDATE_REBUILD):
        sc.set_transforms(xf if mode == L.UPDATE_REFIT else xf * np.float32(1.0), mode)
        h, _, c = Q.query(orc.load(), sc.tris, sc.bvh_nodes, rays, tri_order=sc._tri_order)
        assert not Q.same_bits(h, hits0)
        got, st = _closest(sc, rays)
        assert Q.same_bits(got, h) and _same_counters(st, c), mode
        xf[:, 12:15] *= np.float32(-0.5)


# ---- the torch path, errors, replicas -----------------------------------------------------------------------------------------------
def test_torch_tensors_on_a_side_stream_match_the_host_entry(rrt, orc):
    import torch
    sc, rays, ref = _case(rrt, orc, "helmet")
    host, _ = sc.query_closest(rays.view(np.float32).reshape(-1, 8), traversal=CULL, cull_margin=SAFE)
    occ_host, _ = sc.query_occluded(rays.view(np.float32).reshape(-1, 8))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_rays = _dev(rays) * 1.0                            # produced on the side stream: the query is ordered after it
        dev, st = sc.query_closest(d_rays, traversal=CULL, cull_margin=SAFE)
        o, d = d_rays[:, 0:3].contiguous(), d_rays[:, 4:7].contiguous()
        dev2, _ = sc.query_closest((o, d), t_max=1e30, traversal=CULL, cull_margin=SAFE, stream=side)
        occ_dev, _ = sc.query_occluded(d_rays, stream=side.cuda_stream)
    side.synchronize()
    for k in ("t", "u", "v", "prim", "front_face", "hit"):
        assert dev[k].is_cuda
        a, b, c = host[k], dev[k].cpu().numpy(), dev2[k].cpu().numpy()
        if a.dtype == np.float32:
            assert Q.same_bits(a, b) and Q.same_bits(a, c), k
        else:
            assert np.array_equal(a, b) and np.array_equal(a, c), k
    want = ref[ARMS[2]][0]
    assert Q.same_bits(host["t"], want["t"]) and np.array_equal(host["hit"], want["prim"] != Q.NONE)
    assert np.array_equal(host["prim"][host["hit"]], (want["prim"] & 0x01FFFFFF)[host["hit"]]) and np.all(host["prim"][~host["hit"]] == -1)
    assert np.array_equal(host["front_face"], (want["prim"] != Q.NONE) & ((want["prim"] & Q.FRONT) != 0))
    assert np.array_equal(occ_host, occ_dev.cpu().numpy()) and np.array_equal(occ_host, ref[ARMS[0]][1] != 0)


def test_device_entries_refuse_host_memory_and_the_scene_still_works(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc, rays, ref = _case(rrt, orc, "cornell")
    r = np.ascontiguousarray(rays[:64])
    d_r = _dev(r)
    d_out = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
    h_out = np.zeros(64 + 1, dtype=Q.HIT)
    h_ptr = h_out.ctypes.data + (-h_out.ctypes.data) % 16
    opt = L.MiptQueryOptions()
    assert lib.mipt_query_closest_device(sc._handle, d_r.data_ptr(), 64, C.byref(opt), h_ptr, None, None) == L.ERR_INVALID_ARG
    assert "d_hits is not device memory" in lib.mipt_last_error().decode()
    h_rays = np.zeros(64 * 32 + 16, dtype=np.uint8)                            # an aligned address inside an over-allocated buffer
    r_ptr = h_rays.ctypes.data + (-h_rays.ctypes.data) % 16
    assert lib.mipt_query_occluded_device(sc._handle, r_ptr, 64, C.byref(opt), d_out.data_ptr(), None, None) == L.ERR_INVALID_ARG
    assert "d_rays is not device memory" in lib.mipt_last_error().decode()
    assert torch.count_nonzero(d_out).item() == 0
    got, st = _closest(sc, r)
    assert Q.same_bits(got, ref[ARMS[0]][0][:64])


def test_replica_handle_answers_the_same(rrt, orc):
    sc, rays, ref = _case(rrt, orc, "cornell")
    multi = sc.upload_multi([0])
    replica = rrt.load().mipt_multi_scene(multi, 0)
    got, st = _closest(sc, rays, ARMS[2], handle=replica)
    assert Q.same_bits(got, ref[ARMS[2]][0]) and _same_counters(st, ref[ARMS[2]][2])
    got, st = _occluded(sc, rays, handle=replica, device=True)
    assert np.array_equal(got, ref[ARMS[0]][1])
