"""GPU: mipt_render_motion / mipt_render_motion_device and mipt_scene_track_motion (csrc/first_hit.hip in its MOTION form,
csrc/scene_mesh.hip) against the model of tests/tools/motion_model.py, bit for bit on uint32 views.  The mesh is the smallest that
gives the device-built tree a triangle order of its own (a ground, a box, a fan of thin triangles); the frames are ragged 8x8 tiles,
less than one wave and one pixel.  A model frame's hits are computed once per (geometry, camera, options) and shared."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import features_model as F  # noqa: E402
import launch_thresholds as LT  # noqa: E402
import motion_model as M  # noqa: E402
import motion_world as MW  # noqa: E402
import query_model as Q  # noqa: E402
import temporal_model as T  # noqa: E402

pytestmark = pytest.mark.gpu

SAFE = 0.0078125
REF, CULL = 0, 1
ARMS = [(REF, 0.0), (CULL, SAFE)]
SIZES = [(1, 1), (5, 5), (65, 9), (61, 37)]
POISON_F, POISON_I = 0x7FA5A5A5, 0x25A5A5A5


# ---- the three-part mesh and its generations ------------------------------------------------------------------------------------------
def _camera(rrt, pose, dp=(0.0, 0.0, 0.0), dyaw=0.0):
    c = rrt.Camera(position=tuple(float(pose[0][i]) + dp[i] for i in range(3)), pitch=pose[1], yaw=pose[2] + dyaw)
    c.update_view()
    return c


def _poses():
    a = np.deg2rad(25.0)
    rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return np.stack([MW.mat4(np.eye(3), (0.05, -0.02, 0.1)),                       # the ground slides
                     MW.mat4(rot @ np.diag([1.0, 1.2, 0.9]), (0.1, 0.15, 0.2)),    # the box turns, stretches and moves
                     MW.mat4(np.diag([1.0, 1.0, -1.0]), (0.1, -0.1, 0.3))])        # the fan is mirrored


def _deformed(pos):
    p = np.asarray(pos, dtype=np.float64)
    return (p + 0.04 * np.sin(5.0 * p[:, [1, 2, 0]] + 0.3)).astype(np.float32)


def _world(rrt, generation, track=True):
    """A fresh resident three-part mesh taken to `generation` (0: as created; 1: transforms; 2: deformed positions, the matrices kept;
    3: transforms back to none), tracking on before the first update.  -> (Scene with the device's tree mirrored, the expansion of
    the generation before -- at 0 of the generation itself -- by mesh_model, the mesh arguments)"""
    import torch
    mesh, mats, pose = MW.three_parts()
    sc = rrt.Scene.from_mesh(materials=mats, **mesh)
    sc.camera = _camera(rrt, pose)
    sc.upload_from_mesh(0, fetch_bvh=True)
    assert not np.array_equal(sc._tri_order, np.arange(len(sc.tris)))          # the tree has an order of its own
    if track:
        sc.track_motion()
    states = [(mesh["positions"], None)]
    if generation >= 1:
        sc.set_transforms(_poses().reshape(-1, 4, 4))
        states.append((mesh["positions"], _poses()))
    if generation >= 2:
        new = _deformed(mesh["positions"])
        sc.update_mesh_device(positions=torch.from_numpy(new).cuda())
        states.append((new, _poses()))
    if generation >= 3:
        sc.set_transforms(None)
        states.append((states[-1][0], None))
    p, xf = states[-2] if generation else states[-1]
    prev = MW.expand(mesh, transforms=xf, positions=p)
    cur = MW.expand(mesh, transforms=states[-1][1], positions=states[-1][0])
    assert F.same_bits(cur.view(np.uint32), sc.tris[np.argsort(sc._tri_order)].view(np.uint32))   # the mirror is the model's generation
    return sc, prev, mesh


_hits = {}


def _model_hits(orc, sc, key, cam, size, seed_mode, sample_begin, arm):
    """(T, u, v) of one view, computed once per key"""
    k = (key, cam.tobytes(), size, seed_mode, sample_begin if seed_mode else 0, arm)
    if k not in _hits:
        rays = F.camera_rays(orc, sc, cam, size[0], size[1], seed_mode, sample_begin)[0]
        _hits[k] = M.hits(orc, sc, rays, arm[0] == CULL, arm[1], sc._tri_order)[:3]
    return _hits[k]


def _model(orc, sc, key, cams, size, seed_mode, sample_begin, arm, prev_tris):
    return np.stack([M.from_hits(*_model_hits(orc, sc, key, np.asarray(getattr(c, "uniform", c)), size, seed_mode, sample_begin, arm), prev_tris)
                     .reshape(size[1], size[0], 3) for c in cams])


def _cam_table(cams):
    from rust_ray_tracing_amd import _lib as L
    return np.ascontiguousarray(np.stack([np.asarray(getattr(c, "uniform", c), dtype=L.CAMERA).reshape(()) for c in cams]))


def _motion(rrt, handle, cams, size, prev_tris=None, seed_mode=0, arm=ARMS[0], sample_begin=0, device=False, stream=None, expect=0, samples=1):
    """one call of the C entry: prev_position poisoned beforehand with a sentinel word behind it -> ([V,H,W,3] float32, stats)"""
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    w, h = size
    n = len(cams) * w * h
    table = _cam_table(cams)
    opt = rrt.make_options(w, h, samples, 1, seed_mode=seed_mode, traversal=arm[0], sample_begin=sample_begin, cull_margin=arm[1])
    b, st = L.MiptMotionBuffers(), L.MiptStats()
    if prev_tris is not None:
        prev_tris = np.ascontiguousarray(prev_tris)
        b.n_prev_tris = len(prev_tris)
    if device:
        import torch
        store = torch.full((n * 3 + 1,), POISON_I, dtype=torch.int32, device="cuda")
        d_prev = torch.from_numpy(prev_tris.view(np.uint8).copy()).cuda() if prev_tris is not None else None
        torch.cuda.synchronize()
        b.prev_position, b.prev_tris = store.data_ptr(), d_prev.data_ptr() if d_prev is not None else None
        rc = lib.mipt_render_motion_device(handle, L.ptr(table), len(cams), C.byref(opt), C.byref(b), stream, C.byref(st))
        raw, poison = store.cpu().numpy().view(np.uint32), POISON_I
    else:
        store = np.full(n * 3 + 1, POISON_F, dtype=np.uint32)
        b.prev_position, b.prev_tris = store.ctypes.data, prev_tris.ctypes.data if prev_tris is not None else None
        rc = lib.mipt_render_motion(handle, L.ptr(table), len(cams), C.byref(opt), C.byref(b), C.byref(st))
        raw, poison = store, POISON_F
    assert rc == expect, (rc, lib.mipt_last_error())
    assert raw[-1] == poison                                                  # nothing is written behind the last pixel
    if rc == 0:
        assert not (raw[:-1] == poison).any()                                 # and every word in front of it is
    s = st.as_dict()
    if rc == 0:
        assert s["pixels"] == n and s["tex_clamped"] == 0 and s["stack_overflows"] == 0 and s["rays"] == 0 and s["kernel_ms"] > 0
    return raw[:-1].view(np.float32).reshape(len(cams), h, w, 3), s


def _render(rrt, sc, handle=None):
    from rust_ray_tracing_amd import _lib as L
    hdr = np.zeros((12, 16, 3), dtype=np.float32)
    o = rrt.make_options(16, 12, 2, 3)
    L.check(rrt.load().mipt_render(handle if handle is not None else sc._handle, L.ptr(sc.camera.uniform), C.byref(o), L.ptr(hdr), None, None), "mipt_render")
    return hdr.view(np.uint32)


# ---- the generations: the tracked source is the model of the generation before, and so is the explicit one -----------------------------
@pytest.mark.parametrize("generation", [0, 1, 2, 3])
def test_generations_tracked_and_explicit(rrt, orc, generation):
    sc, prev, _ = _world(rrt, generation)
    size = (61, 37)
    cams = [sc.camera]
    for seed_mode, arm in ((0, ARMS[0]), (1, ARMS[1])):
        want = _model(orc, sc, ("three", generation), cams, size, seed_mode, 0, arm, prev)
        hit = int((want != 0).any(-1).sum())
        assert 0.15 * size[0] * size[1] < hit < size[0] * size[1]              # hits and sky
        for device in (False, True):
            tracked, _ = _motion(rrt, sc._handle, cams, size, None, seed_mode, arm, device=device)
            explicit, _ = _motion(rrt, sc._handle, cams, size, prev, seed_mode, arm, device=device)
            assert M.same_bits(tracked, want), (generation, seed_mode, device, "tracked")
            assert M.same_bits(explicit, want), (generation, seed_mode, device, "explicit")
    if generation:                                                            # the geometry did move: previous != current
        position, _ = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=1, output_image_dimensions=size, output_image_path="/dev/null")
                                       ).render_features(sc, features=("position",))
        assert not M.same_bits(position["position"], tracked)
    sc.release()


# ---- frame shapes x views x arms x seed modes x sample_begin x entries, on the generation with all three kinds of matrix ----------------
@pytest.mark.parametrize("views", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_frame_shapes(rrt, orc, size, views):
    sc, prev, _ = _world(rrt, 1)
    pose = MW.three_parts()[2]
    cams = [sc.camera, _camera(rrt, pose, dp=(-0.3, 0.2, 0.25), dyaw=6.0), _camera(rrt, pose, dp=(0.1, -0.3, -0.4), dyaw=-9.0)][:views]
    for arm in ARMS:
        for seed_mode, sample_begin in ((0, 0), (1, 0), (1, 5)):
            want = _model(orc, sc, ("three", 1), cams, size, seed_mode, sample_begin, arm, prev)
            for device in (False, True):
                for source in (None, prev):
                    got, _ = _motion(rrt, sc._handle, cams, size, source, seed_mode, arm, sample_begin, device=device)
                    assert M.same_bits(got, want), (size, views, arm, seed_mode, sample_begin, device, source is None)
    # samples is validated and otherwise unused; sample_begin 0 is sample 1
    got, _ = _motion(rrt, sc._handle, cams, size, None, 1, ARMS[0], 5, samples=4)
    assert M.same_bits(got, _model(orc, sc, ("three", 1), cams, size, 1, 5, ARMS[0], prev))
    got, _ = _motion(rrt, sc._handle, cams, size, None, 1, ARMS[0], 1)
    assert M.same_bits(got, _model(orc, sc, ("three", 1), cams, size, 1, 0, ARMS[0], prev))
    sc.release()


# ---- more views than the launch holds lanes: both motion forms of first_hit_kernel on refilled lanes -----------------------------------
# As tests/test_gpu_features.py::test_more_views_than_the_launch_holds_lanes: launch_thresholds.FULL_F work items as views of 61 x 37,
# the three cameras of test_frame_shapes cycled with stride 2 from camera 1.  Every view equals the same entry called on its camera
# alone, and the three single frames equal motion_model.
@pytest.mark.parametrize("source", ["explicit", "tracked"])
def test_more_views_than_the_launch_holds_lanes(rrt, orc, source):
    sc, prev, _ = _world(rrt, 1)
    pose = MW.three_parts()[2]
    cams = [sc.camera, _camera(rrt, pose, dp=(-0.3, 0.2, 0.25), dyaw=6.0), _camera(rrt, pose, dp=(0.1, -0.3, -0.4), dyaw=-9.0)]
    size = (61, 37)
    n_cu = LT.device_n_cu()
    n = LT.views_for(LT.full_f(n_cu), *size)
    LT.check_full_f(n_cu, n * LT.view_work(*size))
    cycle = (2 * np.arange(n) + 1) % 3
    prev_tris = prev if source == "explicit" else None
    t_singles = t_call = t_cmp = 0.0
    for (seed_mode, arm), device in zip(((0, ARMS[0]), (1, ARMS[1])), (False, True)):
        t0 = time.perf_counter()
        want = _model(orc, sc, ("three", 1), cams, size, seed_mode, 0, arm, prev)
        singles = np.concatenate([_motion(rrt, sc._handle, [c], size, prev_tris, seed_mode, arm)[0] for c in cams])
        assert M.same_bits(singles, want), (source, seed_mode)
        assert not M.same_bits(want[0], want[1]) and not M.same_bits(want[1], want[2]) and not M.same_bits(want[0], want[2])
        t_singles += time.perf_counter() - t0
        t0 = time.perf_counter()
        got, _ = _motion(rrt, sc._handle, [cams[c] for c in cycle], size, prev_tris, seed_mode, arm, device=device)
        t_call += time.perf_counter() - t0
        t0 = time.perf_counter()
        same = (got.view(np.uint32) == singles[cycle].view(np.uint32)).reshape(n, -1).all(axis=1)
        assert same.all(), (source, seed_mode, device, int((~same).sum()), [(int(v), int(cycle[v])) for v in np.flatnonzero(~same)[:6]])
        t_cmp += time.perf_counter() - t0
    print(f"motion-{source}: {n} views of {size[0]}x{size[1]} = {n * LT.view_work(*size)} work items on {n_cu} CUs: models and singles {t_singles:.2f} s, "
          f"two batch calls {t_call:.2f} s, compare {t_cmp:.2f} s")
    sc.release()


def test_torch_tensors_on_a_side_stream(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    sc, prev, _ = _world(rrt, 2)
    size = (61, 37)
    want = _model(orc, sc, ("three", 2), [sc.camera], size, 1, 0, ARMS[1], prev)
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=4, output_image_dimensions=size, output_image_path="/dev/null", seed_mode=1,
                                             traversal=L.TRAVERSAL_CULLED))
    host, st = r.render_motion(sc)
    host_x, _ = r.render_motion(sc, prev_tris=prev)
    d_prev = torch.from_numpy(prev.view(np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = torch.ones((1 << 22,), device="cuda").cumsum(0)                 # work in front of the pass on the side stream
        dev, st_d = r.render_motion(sc, device=True)
        dev_x, _ = r.render_motion(sc, cameras=[sc.camera, sc.camera.uniform], prev_tris=d_prev, device=True, stream=side)
        dev_n, _ = r.render_motion(sc, prev_tris=prev, device=True, stream=side)
    side.synchronize()
    assert busy[-1].item() == float(1 << 22)
    assert isinstance(host, np.ndarray) and host.shape == (1, size[1], size[0], 3) and dev.is_cuda and tuple(dev.shape) == host.shape
    assert st["pixels"] == size[0] * size[1] == st_d["pixels"]
    for got in (host, host_x, dev.cpu().numpy(), dev_x.cpu().numpy()[0:1], dev_x.cpu().numpy()[1:2], dev_n.cpu().numpy()):
        assert M.same_bits(got, want)
    sc.release()


# ---- the explicit source on every kind of scene ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["host nodes", "from triangles", "replica"])
def test_explicit_source_on_each_kind_of_scene(rrt, orc, how):
    mesh, mats, pose = MW.three_parts()
    from rust_ray_tracing_amd import _lib as L
    tris = np.ascontiguousarray(MW.expand(mesh)).view(L.TRIANGLE).reshape(-1)
    rng = np.random.default_rng(3)
    if how == "from triangles":
        sc = rrt.Scene.from_arrays(tris, mats, [], build_bvh=False)
        sc.upload_from_triangles(0, fetch_bvh=True)
        order, handle = sc._tri_order, sc._handle
        caller = tris
    else:
        sc = rrt.Scene.from_arrays(tris, mats, [])                             # BVH::build on the host: the caller's order is the tree's
        sc.upload(0)
        order, handle, caller = None, sc._handle, sc.tris
        if how == "replica":
            handle = rrt.load().mipt_multi_scene(sc.upload_multi([0]), 0)
    sc.camera = _camera(rrt, pose)
    prev = caller.copy()
    prev["vertices"]["position"] += rng.normal(0.0, 0.05, prev["vertices"]["position"].shape).astype(np.float32)
    size = (61, 37)
    before = _render(rrt, sc, handle).copy()
    for seed_mode, arm in ((0, ARMS[1]), (1, ARMS[0])):
        rays = F.camera_rays(orc, sc, sc.camera.uniform, size[0], size[1], seed_mode, 0)[0]
        Th, u, v, _ = M.hits(orc, sc, rays, arm[0] == CULL, arm[1], order)
        want = M.from_hits(Th, u, v, prev).reshape(1, size[1], size[0], 3)
        for device in (False, True):
            got, _ = _motion(rrt, handle, [sc.camera], size, prev, seed_mode, arm, device=device)
            assert M.same_bits(got, want), (how, seed_mode, device)
    # a scene that is no tracked mesh has no previous generation of its own
    lib = rrt.load()
    _motion(rrt, handle, [sc.camera], size, None, expect=L.ERR_INVALID_ARG)
    assert b"prev_tris is NULL and the scene is not a mesh that tracks motion" in lib.mipt_last_error()
    assert lib.mipt_scene_track_motion(handle, 1) == L.ERR_INVALID_ARG and b"no mesh" in lib.mipt_last_error()
    assert np.array_equal(_render(rrt, sc, handle), before)
    sc.release()


def test_infinite_and_nan_corners(rrt, orc):
    """a NaN where the model has one, equal bits everywhere else"""
    sc, prev, _ = _world(rrt, 1)
    size = (61, 37)
    Th, _, _ = _model_hits(orc, sc, ("three", 1), sc.camera.uniform, size, 0, 0, ARMS[0])
    seen = np.unique(Th[Th != Q.NONE])
    bad = prev.copy()
    t_inf, t_ninf, t_nan = (int(seen[i]) for i in (0, len(seen) // 2, len(seen) - 1))
    bad["vertices"]["position"][t_inf, 0, 1] = np.inf
    bad["vertices"]["position"][t_ninf, 2, 0] = -np.inf
    bad["vertices"]["position"][t_nan, 1] = np.nan
    want = _model(orc, sc, ("three", 1), [sc.camera], size, 0, 0, ARMS[0], bad)
    assert np.isnan(want).any() and np.isinf(want).any()
    for device in (False, True):
        got, _ = _motion(rrt, sc._handle, [sc.camera], size, bad, device=device)
        assert M.same_but_nan(got, want), device
    sc.release()


# ---- tracking: its life cycle, its memory, and updates that fail -----------------------------------------------------------------------
def test_tracking_lifecycle(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc, prev, mesh = _world(rrt, 1, track=False)
    size = (61, 37)
    cams = [sc.camera]
    info0 = sc.mesh_info()
    _motion(rrt, sc._handle, cams, size, None, expect=L.ERR_INVALID_ARG)      # not tracked yet
    assert b"tracks motion" in lib.mipt_last_error()
    sc.track_motion()
    sc.track_motion()                                                         # twice is once
    info1 = sc.mesh_info()
    held = mesh["positions"].nbytes + 96 * len(mesh["parts"])                 # the positions and a third part table
    assert info1["array_bytes"] == info0["array_bytes"] + held and info1["hbm_bytes"] == info0["hbm_bytes"] + held
    # right after enabling, previous == current (generation 1, with its matrices)
    cur = MW.expand(mesh, transforms=_poses())
    want_same = _model(orc, sc, ("three", 1), cams, size, 0, 0, ARMS[0], cur)
    got, _ = _motion(rrt, sc._handle, cams, size, None)
    assert M.same_bits(got, want_same)
    # an update that is refused leaves both generations, the motion output and a render as they were
    frame = _render(rrt, sc).copy()
    big = _poses()
    big[1, 12] = 3e12
    for mode in (0, 1):
        assert lib.mipt_scene_set_transforms(sc._handle, L.ptr(big), 3, mode, None) == L.ERR_SCENE_LIMIT
        d_big = torch.from_numpy(big).cuda()
        assert lib.mipt_scene_update_mesh_device(sc._handle, None, None, d_big.data_ptr(), mode, None, None) == L.ERR_SCENE_LIMIT
        got, _ = _motion(rrt, sc._handle, cams, size, None)
        assert M.same_bits(got, want_same), mode
        assert np.array_equal(_render(rrt, sc), frame)
    # two updates: only the second step is tracked (REBUILD, then deformed positions with the matrices kept)
    sc.set_transforms(None, mode=L.UPDATE_REBUILD)
    new = _deformed(mesh["positions"])
    sc.update_mesh_device(positions=torch.from_numpy(new).cuda())
    want = _model(orc, sc, ("three", "rebuilt"), cams, size, 0, 0, ARMS[0], MW.expand(mesh))
    got, _ = _motion(rrt, sc._handle, cams, size, None)
    assert M.same_bits(got, want)
    # position updates in a row: each makes the positions before it the previous ones
    sc.update_mesh_device(positions=torch.from_numpy(mesh["positions"]).cuda())
    back = _model(orc, sc, ("three", "back"), cams, size, 0, 0, ARMS[0], MW.expand(mesh, positions=new))
    got, _ = _motion(rrt, sc._handle, cams, size, None)
    assert M.same_bits(got, back) and not M.same_bits(back, want)
    sc.update_mesh_device(positions=torch.from_numpy(new).cuda())
    got, _ = _motion(rrt, sc._handle, cams, size, None)
    assert M.same_bits(got, want)
    # disabling gives the memory back and refuses the tracked source; the explicit one and a render go on
    frame = _render(rrt, sc).copy()
    sc.track_motion(False)
    assert sc.mesh_info() == dict(info0, has_transforms=0)
    _motion(rrt, sc._handle, cams, size, None, expect=L.ERR_INVALID_ARG)
    assert b"tracks motion" in lib.mipt_last_error()
    got, _ = _motion(rrt, sc._handle, cams, size, MW.expand(mesh))
    assert M.same_bits(got, want) and np.array_equal(_render(rrt, sc), frame)
    # and on again: transforms after a disable use the two tables that are left
    sc.track_motion()
    sc.set_transforms(_poses().reshape(-1, 4, 4))
    want = _model(orc, sc, ("three", "again"), cams, size, 0, 0, ARMS[0], MW.expand(mesh, positions=new))
    got, _ = _motion(rrt, sc._handle, cams, size, None)
    assert M.same_bits(got, want)
    sc.release()


def test_refusals_leave_the_scene_as_before(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc, prev, _ = _world(rrt, 1)
    size = (61, 37)
    w, h = size
    n = w * h
    want = _model(orc, sc, ("three", 1), [sc.camera], size, 0, 0, ARMS[0], prev)
    before = _render(rrt, sc).copy()
    table = _cam_table([sc.camera])
    d_buf = torch.full((n * 3 + 4,), POISON_I, dtype=torch.int32, device="cuda")
    d_prev = torch.from_numpy(prev.view(np.uint8).copy()).cuda()
    h_buf = np.full(n * 3 + 4, POISON_F, dtype=np.uint32)

    def opts(**kw):
        o = rrt.make_options(w, h, 1, 1)
        for k, v in kw.items():
            if k == "reserved":
                o.reserved[v] = 1
            else:
                setattr(o, k, v)
        return o

    def bufs(ptr, **kw):
        b = L.MiptMotionBuffers()
        b.prev_position = ptr
        for k, v in kw.items():
            if k == "reserved":
                b.reserved[v] = ptr
            else:
                setattr(b, k, v)
        return b

    option_cases = [
        (dict(width=0), "width"), (dict(samples=0), "samples"), (dict(max_ray_depth=0), "max_ray_depth"), (dict(seed_mode=3), "seed_mode"),
        (dict(samples=3), "MIPT_SEED_PIXEL_STREAM"), (dict(traversal=5), "traversal"), (dict(cull_margin=2.0), "cull_margin"),
        (dict(flags=L.FLAG_COUNT), "flags"), (dict(tile_world=4), "tile_world"), (dict(tile_rank=1), "tile_rank"),
        (dict(shading=L.SHADING_WGPU), "shading"), (dict(reserved=1), "reserved"), (dict(width=1 << 15, height=1 << 15), "below 2^32"),
    ]
    for device in (False, True):
        ptr = d_buf.data_ptr() if device else h_buf.ctypes.data
        tris_ptr = d_prev.data_ptr() if device else prev.ctypes.data
        f = lib.mipt_render_motion_device if device else lib.mipt_render_motion
        tail = [None, None] if device else [None]
        for kw, msg in option_cases:
            nv = 4 if "height" in kw else 1
            assert f(sc._handle, L.ptr(table), nv, C.byref(opts(**kw)), C.byref(bufs(ptr)), *tail) == L.ERR_INVALID_ARG, (kw, device)
            assert msg in lib.mipt_last_error().decode(), (kw, lib.mipt_last_error())
        for args, msg in [((None, L.ptr(table), 1, C.byref(opts()), C.byref(bufs(ptr))), "null scene"),
                          ((sc._handle, None, 1, C.byref(opts()), C.byref(bufs(ptr))), "cameras"),
                          ((sc._handle, L.ptr(table), 1, None, C.byref(bufs(ptr))), "opt"),
                          ((sc._handle, L.ptr(table), 1, C.byref(opts()), None), "buffers"),
                          ((sc._handle, L.ptr(table), 0, C.byref(opts()), C.byref(bufs(ptr))), "n_views"),
                          ((sc._handle, L.ptr(table), 1, C.byref(opts()), C.byref(bufs(None))), "null prev_position"),
                          ((sc._handle, L.ptr(table), 1, C.byref(opts()), C.byref(bufs(ptr, reserved0=1))), "reserved0"),
                          ((sc._handle, L.ptr(table), 1, C.byref(opts()), C.byref(bufs(ptr, reserved=4))), "reserved buffer pointers"),
                          ((sc._handle, L.ptr(table), 1, C.byref(opts()), C.byref(bufs(ptr, n_prev_tris=len(prev)))), "n_prev_tris"),
                          ((sc._handle, L.ptr(table), 1, C.byref(opts()), C.byref(bufs(ptr, prev_tris=tris_ptr, n_prev_tris=len(prev) - 1))), "n_prev_tris"),
                          ((sc._handle, L.ptr(table), 1, C.byref(opts()), C.byref(bufs(ptr, prev_tris=tris_ptr, n_prev_tris=len(prev) + 1))), "n_prev_tris")]:
            assert f(*args, *tail) == L.ERR_INVALID_ARG, (msg, device)
            assert msg in lib.mipt_last_error().decode(), (msg, lib.mipt_last_error())
    # the device entry: host memory, and pointers that are not 4-byte aligned
    f = lib.mipt_render_motion_device
    for b, msg in ((bufs(h_buf.ctypes.data), "prev_position is not device memory"),
                   (bufs(d_buf.data_ptr(), prev_tris=prev.ctypes.data, n_prev_tris=len(prev)), "prev_tris is not device memory"),
                   (bufs(d_buf.data_ptr() + 2), "prev_position must be 4-byte aligned"),
                   (bufs(d_buf.data_ptr(), prev_tris=d_prev.data_ptr() + 1, n_prev_tris=len(prev)), "prev_tris must be 4-byte aligned")):
        assert f(sc._handle, L.ptr(table), 1, C.byref(opts()), C.byref(b), None, None) == L.ERR_INVALID_ARG, msg
        assert msg in lib.mipt_last_error().decode(), (msg, lib.mipt_last_error())
    assert np.all(h_buf == POISON_F) and bool(torch.all(d_buf == POISON_I))   # no refused call wrote anything
    # the scene renders, queries and gives its previous positions as before
    assert np.array_equal(_render(rrt, sc), before)
    got, _ = _motion(rrt, sc._handle, [sc.camera], size, None)
    assert M.same_bits(got, want)
    rays = F.camera_rays(orc, sc, sc.camera.uniform, w, h, 0, pixels=np.arange(0, n, 37))[0]
    hits, _ = sc.query_closest(rays.view(np.float32).reshape(-1, 8))
    Th, u, v = _model_hits(orc, sc, ("three", 1), sc.camera.uniform, size, 0, 0, ARMS[0])
    sel = Th[::37] != Q.NONE
    assert sel.any() and F.same_bits(hits["u"][sel], u[::37][sel]) and F.same_bits(hits["v"][sel], v[::37][sel])
    sc.release()


# ---- render_sequence(motion=True): the calls made separately, and the temporal model fed prev_position ---------------------------------
def test_render_sequence_with_motion(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    size = (61, 37)
    w, h = size
    mesh, mats, texs, pose, block = MW.cornell_block()
    sc = rrt.Scene.from_mesh(materials=mats, textures=texs, **mesh)
    sc.camera = _camera(rrt, pose)
    sc.upload_from_mesh(0)
    n_parts = len(mesh["parts"])
    steps = [None, MW.block_pose(n_parts, block, (0.0, 0.0, 0.06), 3.0), MW.block_pose(n_parts, block, (0.02, 0.0, 0.15), 7.0)]
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=6, output_image_dimensions=size, output_image_path="/dev/null",
                                             seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED))
    path = [[sc.camera]] * 3
    with pytest.raises(ValueError):
        next(r.render_sequence(sc, path, motion=True))                         # not tracked yet
    stream = torch.cuda.current_stream().cuda_stream

    def run(motion):
        sc.set_transforms(None)
        frames = []
        seq = r.render_sequence(sc, path, denoise=False, motion=motion, max_history=16.0)
        for f in range(3):
            if steps[f] is not None:
                sc.set_transforms(steps[f].reshape(-1, 4, 4))
            fr = next(seq)
            torch.cuda.synchronize()
            keep = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in fr.items() if k != "features"}
            keep["features"] = {k: v.cpu().numpy() for k, v in fr["features"].items()}
            keep["history"] = keep["history"].view(np.uint32).copy()
            # the calls made separately, on the geometry of this frame
            sep, _ = r.render_features(sc, path[f], ("depth", "normal", "albedo", "position", "material"), device=True)
            for k in sep:
                assert np.array_equal(sep[k].cpu().numpy().view(np.uint32), keep["features"][k].view(np.uint32)), (f, k)
            if motion:
                alone, _ = r.render_motion(sc, path[f], device=True)
                assert M.same_bits(alone.cpu().numpy(), keep["prev_position"]), f
            else:
                assert "prev_position" not in keep
            frames.append(keep)
        return frames

    sc.track_motion()
    with_motion = run(True)
    without = run(False)
    cams = np.stack([sc.camera.uniform])
    for frames, motion in ((with_motion, True), (without, False)):
        history = None
        for f, fr in enumerate(frames):
            feat = fr["features"]
            position = fr["prev_position"] if motion else feat["position"]
            want = T.step(fr["noisy"], position, feat["normal"], feat["depth"], feat["material"].view(np.uint32), cams, history, feat["albedo"],
                          **dict(T.DEFAULTS, max_history=16.0))
            assert T.same_bits(fr["accumulated"], want["out"]), (motion, f)
            assert T.same_history(fr["history"], want["history"], 1, h, w), (motion, f)
            assert T.same_bits(fr["length"], want["length"]) and T.same_bits(fr["variance"], want["variance"]), (motion, f)
            history = want["history"]
    # frame 0 has no motion yet: the previous position is the position but for rounding; afterwards they differ on the block, and
    # only there, and the accumulated frames of the two sequences differ
    assert np.abs(with_motion[0]["prev_position"] - with_motion[0]["features"]["position"]).max() <= 1e-5
    block_mat = int(mesh["parts"][block[0]]["material_id"])
    on_block = with_motion[2]["features"]["material"].view(np.uint32) == block_mat
    moved = np.abs(with_motion[2]["prev_position"] - with_motion[2]["features"]["position"]).max(-1)
    assert on_block.sum() > 20 and moved[on_block].min() > 1e-3 and moved[~on_block].max() <= 1e-5
    assert not T.same_bits(with_motion[2]["accumulated"], without[2]["accumulated"])
    # motion=False is today's sequence: the same frames as the calls of the sequence without the argument
    sc.set_transforms(None)
    plain = [fr["accumulated"].cpu().numpy() for fr in r.render_sequence(sc, path[:2], denoise=False, max_history=16.0)]
    again = [fr["accumulated"].cpu().numpy() for fr in r.render_sequence(sc, path[:2], denoise=False, motion=False, max_history=16.0)]
    assert all(T.same_bits(a, b) for a, b in zip(plain, again))
    sc.release()
