"""GPU: mipt_render_features / mipt_render_features_device (csrc/first_hit.hip) against the model of tests/tools/features_model.py, which
tests/test_features_model.py holds to the oracle.  Every comparison is bit for bit on uint32 views (and, with MIPT_FLAG_COUNT, on the
six counters and `pixels`).  The frames are the smallest at which the kernel can go wrong -- ragged 8x8 tiles, less than one wave, one
pixel -- and each model frame is computed once and left unchanged."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import features_model as F  # noqa: E402
import launch_thresholds as LT  # noqa: E402
import mesh_model  # noqa: E402
import query_model as Q  # noqa: E402

pytestmark = pytest.mark.gpu

SAFE = 0.0078125
REF, CULL = 0, 1
ARMS = [(REF, 0.0), (CULL, 0.0), (CULL, SAFE)]
SIZES = [(61, 37), (8, 8), (1, 1)]
POISON_F, POISON_I = 0x7FA5A5A5, 0x25A5A5A5                     # what a word nobody wrote holds (host buffers / int32 tensors)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _make(kind):
    from rust_ray_tracing_amd import synth
    if kind == "quads":
        return _quads()
    kw = dict(n_target=2000, tex_size=32) if kind == "helmet" else {}
    return synth.make_scene(kind, **kw)


def _quads():
    """A few quads in front of the cornell camera with open sky around them: one seen from the front, one from behind (the same
    winding turned round), one with a base-colour AND an emission texture whose uv run past 1.  Vertex normals are neither unit nor
    equal, so their interpolation shows."""
    from rust_ray_tracing_amd import synth
    rng = np.random.default_rng(11)
    texs = [synth.value_noise_texture(rng, 16, (0.9, 0.6, 0.3), checker=True), synth.value_noise_texture(rng, 8, (0.2, 0.7, 0.9))]
    mats = [synth.material(base=(0.8, 0.3, 0.2), emission=(0.5, 0.25, 0.125)), synth.material(base=(0.1, 0.9, 0.4)),
            synth.material(base_tex=0, emission_tex=1)]
    a = synth.quad((0, 0.2, -1.8), (0, 1.8, -1.8), (0, 1.8, -0.2), (0, 0.2, -0.2), (1, 0, 0), 0)
    b = synth.quad((0, 0.2, 1.8), (0, 1.8, 1.8), (0, 1.8, 0.2), (0, 0.2, 0.2), (1, 0, 0), 1)
    c = synth.quad((-0.5, -1.8, -1.0), (-0.5, -0.2, -1.0), (-0.5, -0.2, 1.0), (-0.5, -1.8, 1.0), (1, 0, 0), 2, uv_scale=2.5)
    tris = np.concatenate([a, b, c])
    tris["vertices"]["normal"] += rng.uniform(-0.4, 0.4, tris["vertices"]["normal"].shape).astype(np.float32)
    return tris, mats, texs, synth.CORNELL_CAMERA


def _host_scene(rrt, kind):
    tris, mats, texs, cam = _make(kind)
    sc = rrt.Scene.from_arrays(tris, mats, texs)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    return sc


_scenes, _models, _rays = {}, {}, {}


def _scene(rrt, kind):
    if kind not in _scenes:
        _scenes[kind] = _host_scene(rrt, kind)
        _scenes[kind].upload(0)
    return _scenes[kind]


def _model(rrt, orc, kind, size, seed_mode, arm=ARMS[0], samples=1, sample_begin=0):
    """the model frame of a cached host-built scene's own camera: ({name: array}, counters), computed once and left unchanged"""
    key = (kind, size, seed_mode, arm, samples, sample_begin)
    if key not in _models:
        sc = _scene(rrt, kind)
        rays = _rays.setdefault((kind, size, seed_mode), {})
        _models[key] = F.frame(orc, sc, sc.camera.uniform, size[0], size[1], seed_mode, samples, sample_begin, arm[0] == CULL, arm[1], rays=rays)[:2]
    return _models[key]


# ---- one call of the C entry, with a sentinel word behind every output -------------------------------------------------------------
def _cam_table(cams):
    from rust_ray_tracing_amd import _lib as L
    return np.ascontiguousarray(np.stack([np.asarray(getattr(c, "uniform", c), dtype=L.CAMERA).reshape(()) for c in cams]))


def _features(rrt, handle, cams, size, seed_mode=0, arm=ARMS[0], samples=1, sample_begin=0, names=F.NAMES, device=False, count=True,
              stream=None, expect=0):
    """-> ({name: array [V,H,W(,k)]}, stats dict).  Every output is one word longer than the call needs; that word must keep its
    pattern."""
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    w, h = size
    n = len(cams) * w * h
    table = _cam_table(cams)
    opt = rrt.make_options(w, h, samples, 1, seed_mode=seed_mode, traversal=arm[0], flags=L.FLAG_COUNT if count else 0, sample_begin=sample_begin,
                           cull_margin=arm[1])
    bufs, st, store = L.MiptFeatureBuffers(), L.MiptStats(), {}
    if device:
        import torch
        for k in names:
            store[k] = torch.full((n * F.WIDTH[k] + 1,), POISON_I, dtype=torch.int32, device="cuda")
            setattr(bufs, k, store[k].data_ptr())
        rc = lib.mipt_render_features_device(handle, L.ptr(table), len(cams), C.byref(opt), C.byref(bufs), stream, C.byref(st))
        raw = {k: v.cpu().numpy().view(np.uint32) for k, v in store.items()}
        poison = POISON_I
    else:
        for k in names:
            store[k] = np.full(n * F.WIDTH[k] + 1, POISON_F, dtype=np.uint32)
            setattr(bufs, k, store[k].ctypes.data)
        rc = lib.mipt_render_features(handle, L.ptr(table), len(cams), C.byref(opt), C.byref(bufs), C.byref(st))
        raw, poison = store, POISON_F
    assert rc == expect, (rc, lib.mipt_last_error())
    out = {}
    for k in names:
        assert raw[k][-1] == poison, k                                         # nothing is written behind the last pixel
        a = raw[k][:-1] if k in F.UINT else raw[k][:-1].view(np.float32)
        out[k] = a.reshape((len(cams), h, w) + ((F.WIDTH[k],) if F.WIDTH[k] > 1 else ()))
    return out, st.as_dict()


def _same(got, want, names=F.NAMES, view=None):
    """names whose bits differ"""
    return [k for k in names if not F.same_bits(got[k] if view is None else got[k][view], want[k])]


def _same_counters(st, model):
    keys = F.COUNTERS + ("pixels",)
    return {k: st[k] for k in keys} == {k: model[k] for k in keys}


def _render(rrt, sc, handle=None):
    """a small frame of the scene through mipt_render: what must be the same before and after anything the feature pass does"""
    from rust_ray_tracing_amd import _lib as L
    hdr = np.zeros((12, 16, 3), dtype=np.float32)
    o = rrt.make_options(16, 12, 2, 3)
    L.check(rrt.load().mipt_render(handle if handle is not None else sc._handle, L.ptr(sc.camera.uniform), C.byref(o), L.ptr(hdr), None, None), "mipt_render")
    return hdr.view(np.uint32)


# ---- the frames: ragged tiles, less than a wave, one pixel; three arms, both seed modes, both entries ------------------------------
@pytest.mark.parametrize("arm", ARMS, ids=["ref", "cull0", "cullsafe"])
@pytest.mark.parametrize("seed_mode", [0, 1])
@pytest.mark.parametrize("kind", ["cornell", "helmet", "quads"])
def test_frames_against_the_model(rrt, orc, kind, seed_mode, arm):
    sc = _scene(rrt, kind)
    for size in SIZES:
        want, counters = _model(rrt, orc, kind, size, seed_mode, arm)
        if size == SIZES[0] and arm == ARMS[0]:
            prim = want["prim"]
            hit = prim != Q.NONE
            front = hit & ((prim & Q.FRONT) != 0)
            assert hit.any(), kind
            if kind == "quads":                                            # front hits, back hits, sky and both textures in one frame
                assert front.any() and (hit & ~front).any() and (~hit).any() and counters["texel_fetches"] >= 2
                assert np.any(want["uv"] > 1.0) and (want["material"] == 2).any()
            if kind == "helmet":
                assert (~hit).any() and counters["texel_fetches"] > 0
        for device in (False, True):
            got, st = _features(rrt, sc._handle, [sc.camera], size, seed_mode, arm, device=device, count=True)
            assert not _same(got, want, view=0), (kind, size, arm, device, _same(got, want, view=0))
            assert _same_counters(st, counters), (kind, size, arm, device, st, counters)
            assert st["kernel_ms"] > 0 and st["stack_overflows"] == 0 and st["tex_clamped"] == 0 and not any(st["diag"])
            got, st = _features(rrt, sc._handle, [sc.camera], size, seed_mode, arm, device=device, count=False)   # the production instantiation
            assert not _same(got, want, view=0), (kind, size, arm, device, _same(got, want, view=0))
            assert st["pixels"] == size[0] * size[1] and st["rays"] == 0 and st["tri_tests"] == 0 and st["texel_fetches"] == 0


# ---- PER_SAMPLE: several samples, a later first sample ------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_begin", [0, 5])
@pytest.mark.parametrize("samples", [1, 3])
def test_per_sample_means_and_first_sample(rrt, orc, samples, sample_begin):
    size = (19, 11)
    for kind in ("helmet", "quads"):
        sc = _scene(rrt, kind)
        for arm in (ARMS[0], ARMS[2]):
            want, counters = _model(rrt, orc, kind, size, 1, arm, samples, sample_begin)
            one, _ = _features(rrt, sc._handle, [sc.camera], size, 1, arm, 1, sample_begin)
            for device in (False, True):
                for count in (True, False):
                    got, st = _features(rrt, sc._handle, [sc.camera], size, 1, arm, samples, sample_begin, device=device, count=count)
                    assert not _same(got, want, view=0), (kind, arm, device, count, _same(got, want, view=0))
                    assert not _same(got, one, ("depth", "prim", "material", "position", "uv")), (kind, arm, device)
                    assert st["pixels"] == size[0] * size[1]
                    if count:
                        assert _same_counters(st, counters) and st["rays"] == samples * size[0] * size[1]
    if samples == 3:                                                           # the samples do differ: the mean is not the first sample
        assert _same(got, one, ("normal",)) or _same(got, one, ("albedo",))


# ---- buffer subsets ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_buffer_subsets_give_the_same_bits(rrt, orc, device):
    size = SIZES[0]
    sc = _scene(rrt, "quads")
    want, counters = _model(rrt, orc, "quads", size, 0)
    alls, st_all = _features(rrt, sc._handle, [sc.camera], size, device=device)
    assert not _same(alls, want, view=0)
    for k in F.NAMES:
        got, st = _features(rrt, sc._handle, [sc.camera], size, names=(k,), device=device)
        assert F.same_bits(got[k], alls[k]), k
        # a texture is fetched only for a buffer that is wanted
        fetches = {"albedo": (want["material"] == 2).sum(), "emission": (want["material"] == 2).sum()}.get(k, 0)
        assert st["texel_fetches"] == fetches and st["hits"] == counters["hits"] and st["pixels"] == counters["pixels"], (k, st)
    assert st_all["texel_fetches"] == 2 * (want["material"] == 2).sum()


def test_a_buffer_that_is_not_wanted_is_never_written(rrt):
    """All eight outputs are slices of ONE poisoned tensor; seven are passed, the eighth slice must keep its poison"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc = _scene(rrt, "quads")
    w, h = SIZES[0]
    n = w * h
    table = _cam_table([sc.camera])
    off, total = {}, 0
    for k in F.NAMES:
        off[k], total = total, total + n * F.WIDTH[k]
    for left_out in F.NAMES:
        t = torch.full((total,), POISON_I, dtype=torch.int32, device="cuda")
        bufs = L.MiptFeatureBuffers()
        for k in F.NAMES:
            if k != left_out:
                setattr(bufs, k, t.data_ptr() + 4 * off[k])
        opt = rrt.make_options(w, h, 1, 1)
        assert lib.mipt_render_features_device(sc._handle, L.ptr(table), 1, C.byref(opt), C.byref(bufs), None, None) == 0
        host = t.cpu().numpy()
        for k in F.NAMES:
            part = host[off[k]: off[k] + n * F.WIDTH[k]]
            if k == left_out:
                assert np.all(part == POISON_I), k
            else:
                assert not np.any(part == POISON_I), k                         # every word of a wanted buffer is written


# ---- views -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed_mode", [0, 1])
def test_views_equal_single_view_calls(rrt, orc, seed_mode):
    sc = _scene(rrt, "helmet")
    cam = sc.camera
    cams = [cam, rrt.Camera(position=(cam.position[0] + 0.3, cam.position[1] - 0.2, cam.position[2] + 0.1), pitch=cam.pitch + 7.0, yaw=cam.yaw - 11.0),
            rrt.Camera(position=(cam.position[0] - 0.4, cam.position[1] + 0.1, cam.position[2]), pitch=cam.pitch - 5.0, yaw=cam.yaw + 9.0)]
    for c in cams[1:]:
        c.update_view()
    size = (21, 13)                                                            # 3 x 2 tiles per view, ragged both ways
    samples = 1 + seed_mode
    singles = [_features(rrt, sc._handle, [c], size, seed_mode, ARMS[2], samples) for c in cams]
    want, counters = _model(rrt, orc, "helmet", size, seed_mode, ARMS[2], samples)
    assert not _same(singles[0][0], want, view=0) and _same_counters(singles[0][1], counters)
    assert _same(singles[1][0], singles[0][0], ("depth",)) and _same(singles[2][0], singles[1][0], ("depth",))   # three different views
    for device in (False, True):
        got, st = _features(rrt, sc._handle, cams, size, seed_mode, ARMS[2], samples, device=device)
        for v in range(3):
            assert not _same(got, {k: a[0] for k, a in singles[v][0].items()}, view=v), (v, device)
        for k in F.COUNTERS[:-1] + ("pixels",):
            assert st[k] == sum(s[1][k] for s in singles), k
        assert st["max_stack"] == max(s[1]["max_stack"] for s in singles)


# ---- more views than the launch holds lanes: every lane takes a second and a third pixel, of other views ---------------------------
# first_hit_kernel is persistent: n_cu x blocks_per_cu blocks of 256 lanes take work items (view, tile, pixel) from a queue, and every
# launch above fits into the lanes' first fetch.  These pass tests/tools/launch_thresholds.py's FULL_F -- more than twice the lanes in
# flight whatever the occupancy, a ragged tail -- with views of SIZES[0], the size test_frames_against_the_model holds to the model,
# and the four cameras of features_model.batch_cameras cycled with stride 3.  Every buffer of every view must equal the same entry
# called on its camera alone, bit for bit, and those four single frames must equal features_model.frame: views never see each other,
# so the two together cover every word.  tests/test_features_model.py shows that this work order refills waves
# whose other lanes are mid-traversal.
_big_models = {}


def _big_model(rrt, orc, cam_index, cams, seed_mode, samples, arm):
    key = (cam_index, seed_mode, samples, arm)
    if key not in _big_models:
        sc = _scene(rrt, "helmet")
        rays = _rays.setdefault(("helmet-batch", cam_index, seed_mode), {})
        _big_models[key] = F.frame(orc, sc, cams[cam_index].uniform, SIZES[0][0], SIZES[0][1], seed_mode, samples, 0, arm[0] == CULL, arm[1], rays=rays)[:2]
    return _big_models[key]


def _check_big_features(rrt, orc, seed_mode, samples, arm, names, runs, label):
    """runs: (device, count) of each batch call"""
    sc = _scene(rrt, "helmet")
    size = SIZES[0]
    cams = F.batch_cameras(rrt, sc.camera)
    n_cu = LT.device_n_cu()
    n = LT.views_for(LT.full_f(n_cu), *size)
    LT.check_full_f(n_cu, n * LT.view_work(*size))
    cycle = F.batch_cycle(n, len(cams))
    occurs = np.bincount(cycle, minlength=len(cams))
    t0 = time.perf_counter()
    singles = []
    for c in range(len(cams)):
        want, counters = _big_model(rrt, orc, c, cams, seed_mode, samples, arm)
        got, st = _features(rrt, sc._handle, [cams[c]], size, seed_mode, arm, samples, names=names)
        assert not _same(got, want, names, view=0), (label, c, _same(got, want, names, view=0))
        if names == F.NAMES:
            assert _same_counters(st, counters), (label, c, st, counters)
        singles.append((got, st))
    assert all(_same(singles[c][0], singles[0][0], ("depth",)) for c in range(1, len(cams)))   # four different views
    t_singles = time.perf_counter() - t0
    t_call = t_cmp = 0.0
    for device, count in runs:
        t0 = time.perf_counter()
        got, st = _features(rrt, sc._handle, [cams[c] for c in cycle], size, seed_mode, arm, samples, names=names, device=device, count=count)
        t_call += time.perf_counter() - t0
        t0 = time.perf_counter()
        for k in names:
            want = np.concatenate([s[0][k] for s in singles])[cycle]
            same = (np.ascontiguousarray(got[k]).view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)).reshape(n, -1).all(axis=1)
            assert same.all(), (label, k, device, count, int((~same).sum()), [(int(v), int(cycle[v])) for v in np.flatnonzero(~same)[:6]])
        assert st["pixels"] == n * size[0] * size[1] and st["stack_overflows"] == 0 and st["kernel_ms"] > 0
        if count:
            for k in F.COUNTERS[:-1]:
                assert st[k] == sum(int(occurs[c]) * singles[c][1][k] for c in range(len(cams))), (label, k, device)
            assert st["max_stack"] == max(s[1]["max_stack"] for s in singles)
        else:
            assert st["rays"] == 0 and st["tri_tests"] == 0 and st["texel_fetches"] == 0
        t_cmp += time.perf_counter() - t0
    print(f"{label}: {n} views of {size[0]}x{size[1]} = {n * LT.view_work(*size)} work items on {n_cu} CUs: models and singles {t_singles:.2f} s, "
          f"{len(runs)} batch calls {t_call:.2f} s, compare {t_cmp:.2f} s")


@pytest.mark.parametrize("arm", [ARMS[0], ARMS[2]], ids=["ref", "cullsafe"])
@pytest.mark.parametrize("seed_mode,samples", [(0, 1), (1, 3)], ids=["stream-1", "per-sample-3"])
def test_more_views_than_the_launch_holds_lanes(rrt, orc, seed_mode, samples, arm):
    """all eight buffers; with three samples a refilled lane restarts `sample` and the running sums in its new pixel's slots"""
    _check_big_features(rrt, orc, seed_mode, samples, arm, F.NAMES, [(False, True), (True, False), (False, False), (True, True)],
                        f"features-{'stream-1' if seed_mode == 0 else 'per-sample-3'}-{'ref' if arm[0] == REF else 'cullsafe'}")


@pytest.mark.parametrize("names", [("depth", "normal"), ("depth", "prim", "position")], ids=["depth-normal", "no-attributes"])
def test_more_views_than_the_launch_holds_lanes_buffer_subsets(rrt, orc, names):
    """depth and normal: the attribute record is read for the normal alone and no texel is fetched; depth, prim and position: want_attr
    is false and a finished lane reads no record at all -- on refilled lanes as on fresh ones"""
    _check_big_features(rrt, orc, 1, 3, ARMS[2], names, [(False, True), (True, False)], "features-" + "-".join(names))


# ---- scenes made three ways, then REFIT and REBUILD ----------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["upload", "upload_from_triangles", "from_mesh"])
def test_scene_variants_and_updates(rrt, orc, how):
    from rust_ray_tracing_amd import _lib as L
    tris, mats, texs, cam = _make("helmet")
    if how == "upload":
        sc = rrt.Scene.from_arrays(tris, mats, texs)
        sc.upload(0)
    elif how == "upload_from_triangles":
        sc = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
        sc.upload_from_triangles(0, fetch_bvh=True)
    else:
        mesh, _ = mesh_model.mesh_from_triangles(tris, 4)
        sc = rrt.Scene.from_mesh(materials=mats, textures=texs, **mesh)
        sc.upload_from_mesh(0, fetch_bvh=True)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    size = (23, 14)

    def check(tag):
        order = sc._tri_order
        if how != "upload" or tag == "rebuild":
            assert order is not None and not np.array_equal(order, np.arange(len(order)))
        for seed_mode, arm in ((0, ARMS[0]), (1, ARMS[2])):
            want, counters = F.frame(orc, sc, sc.camera.uniform, size[0], size[1], seed_mode, 1, 0, arm[0] == CULL, arm[1], tri_order=order)[:2]
            hit = want["prim"] != Q.NONE
            assert hit.any() and (~hit).any()
            if order is not None:                                              # prim is in the caller's order, not the tree's
                tree = F.frame(orc, sc, sc.camera.uniform, size[0], size[1], seed_mode, 1, 0, arm[0] == CULL, arm[1])[0]
                assert not F.same_bits(tree["prim"], want["prim"])
            for device in (False, True):
                got, st = _features(rrt, sc._handle, [sc.camera], size, seed_mode, arm, device=device)
                assert not _same(got, want, view=0), (how, tag, seed_mode, device, _same(got, want, view=0))
                assert _same_counters(st, counters), (how, tag, st, counters)
        return want

    first = check("created")
    if how == "from_mesh":
        n_parts = len(sc.mesh["parts"])
        xf = np.tile(np.eye(4, dtype=np.float32).reshape(16), (n_parts, 1))
        xf[:, 12:15] = np.random.default_rng(2).normal(0, 0.1, (n_parts, 3)).astype(np.float32)
        sc.set_transforms(xf, L.UPDATE_REFIT)
        refit = check("refit")
        xf[:, 12:15] *= np.float32(-0.5)
        sc.set_transforms(xf, L.UPDATE_REBUILD)
        rebuilt = check("rebuild")
    else:
        rng = np.random.default_rng(5)
        sc.tris["vertices"]["position"] += rng.uniform(-0.02, 0.02, sc.tris["vertices"]["position"].shape).astype(np.float32)
        sc.update_device(L.UPDATE_REFIT)
        refit = check("refit")
        sc.tris = np.ascontiguousarray(sc.tris[: len(sc.tris) - 37])                 # another triangle count, moved once more
        sc.tris["vertices"]["position"] += rng.uniform(-0.02, 0.02, sc.tris["vertices"]["position"].shape).astype(np.float32)
        if sc._tri_order is not None:                                          # update_device scatters through the order: keep it a permutation
            sc._tri_order = None
        sc.update_device(L.UPDATE_REBUILD)
        rebuilt = check("rebuild")
    assert not F.same_bits(first["depth"], refit["depth"]) and not F.same_bits(refit["depth"], rebuilt["depth"])


# ---- consistency without the model, on a larger frame ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed_mode", [0, 1])
def test_albedo_times_emission_is_the_depth_one_render(rrt, seed_mode):
    import torch
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth
    lib = rrt.load()
    if "atrium" not in _scenes:
        tris, mats, texs, cam = synth.make_scene("atrium", n_target=60000, tex_size=64)
        sc = rrt.Scene.from_arrays(tris, mats, texs)
        sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
        sc.upload(0)
        _scenes["atrium"] = sc
    sc = _scenes["atrium"]
    w, h = 256, 144
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=1, output_image_dimensions=(w, h), output_image_path="/dev/null", seed_mode=seed_mode,
                                             traversal=L.TRAVERSAL_CULLED))
    out, st = r.render_features(sc, features=F.NAMES, device=True)
    assert st["pixels"] == w * h and st["stack_overflows"] == 0
    hdr = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    o = rrt.make_options(w, h, 1, 1, seed_mode=seed_mode, traversal=L.TRAVERSAL_CULLED)
    assert lib.mipt_render_device(sc._handle, L.ptr(sc.camera.uniform), C.byref(o), hdr.data_ptr(), None, torch.cuda.current_stream().cuda_stream, None) == 0
    rad = (torch.zeros((), dtype=torch.float32, device="cuda") + out["albedo"][0] * out["emission"][0]) + torch.zeros((), dtype=torch.float32, device="cuda")
    assert torch.equal(rad.view(torch.int32), hdr.view(torch.int32))
    # depth / prim against query_closest on the rays rebuilt from the positions: as hit / miss masks only (the rebuilt directions
    # are not the kernel's bits)
    prim = out["prim"][0].reshape(-1).to(torch.int64) & 0xFFFFFFFF
    hit = prim != L.HIT_NONE
    assert 0 < int(hit.sum()) < w * h
    assert torch.equal(hit, out["depth"][0].reshape(-1) < 1e30) and torch.equal(hit, out["material"][0].reshape(-1) != -1)
    origin = torch.tensor(np.asarray(sc.camera.uniform["position"], dtype=np.float32), device="cuda").expand(w * h, 3).contiguous()
    d = out["position"][0].reshape(-1, 3) - origin
    d = d / d.norm(dim=1, keepdim=True)
    q, _ = sc.query_closest((origin[hit], d[hit].contiguous()))
    assert bool(q["hit"].all())                                              # (a miss has no position to rebuild a ray from)
    assert torch.all(out["position"][0].reshape(-1, 3)[~hit] == 0) and torch.all(out["albedo"][0].reshape(-1, 3)[~hit] == 1)


# ---- the traversal stack ------------------------------------------------------------------------------------------------------------
def test_deep_chain_spills_and_overflows(rrt, orc):
    from test_gpu_batch import _chain_bvh
    from rust_ray_tracing_amd import _lib as L
    sc = _chain_bvh(rrt, 40)                                                   # stack occupancy 40: 16 in LDS, the rest spilled
    sc.upload(0)
    size = (10, 6)                                                             # even: pixel (5, 3) looks straight down the chain
    want, counters = F.frame(orc, sc, sc.camera.uniform, size[0], size[1], 0)[:2]
    assert counters["max_stack"] > 16 and (want["prim"] != Q.NONE).any()
    for device in (False, True):
        for count in (True, False):
            got, st = _features(rrt, sc._handle, [sc.camera], size, device=device, count=count)
            assert not _same(got, want, view=0), (device, count, _same(got, want, view=0))
            assert st["stack_overflows"] == 0 and (not count or _same_counters(st, counters))
    deep = _chain_bvh(rrt, 120)                                                # deeper than the 64 entries: MIPT_ERR_STACK, buffers written
    deep.upload(0)
    for device in (False, True):
        got, st = _features(rrt, deep._handle, [deep.camera], size, device=device, expect=L.ERR_STACK)
        assert st["stack_overflows"] > 0 and st["pixels"] == size[0] * size[1] and "stack" in rrt.load().mipt_last_error().decode()
        for k in F.NAMES:
            assert not np.any(got[k].view(np.uint32) == (POISON_I if device else POISON_F)), k


def test_renders_queries_and_features_share_one_spill_buffer(rrt):
    """A one-block render, a five-block query (the slots must grow), a feature pass, the render again: each call's result and counters
    are those of the same call as the first on a fresh scene"""
    from test_gpu_batch import _chain_bvh
    from rust_ray_tracing_amd import _lib as L
    spilled = Q.chain_rays()[:70]
    big = np.resize(spilled, 4 * 256 + 1)

    def scene():
        sc = _chain_bvh(rrt, 40)
        sc.upload(0)
        return sc

    def render(sc):
        r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=3, output_image_dimensions=(8, 8), output_image_path="/dev/null"))
        hdr, _, st = r.render_buffers(sc, want_rgba8=False, flags=L.FLAG_COUNT)
        return [hdr.view(np.uint32).copy()], st

    def query(sc):
        raw, st = sc._query(False, big, None, REF, 0.0, True, None, None)
        return [raw.view(np.uint32).copy()], st

    def features(sc, size=(40, 30)):
        got, st = _features(rrt, sc._handle, [sc.camera], size)
        return [got[k].view(np.uint32) for k in F.NAMES], st

    def counters(st):
        return dict({k: v for k, v in st.items() if k != "kernel_ms"}, diag=st["diag"][:7])

    shared = scene()
    for i, call in enumerate([render, features, query, lambda sc: features(sc, (10, 6)), render]):
        want, want_st = call(scene())
        got, got_st = call(shared)
        assert want_st["max_stack"] > 16 and want_st["stack_overflows"] == 0, (i, want_st)   # the call spills
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), i
        assert counters(got_st) == counters(want_st), (i, got_st, want_st)


# ---- torch tensors on a side stream, a replica handle, the C++ mirror ------------------------------------------------------------------
def test_torch_tensors_on_a_side_stream(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    sc = _scene(rrt, "helmet")
    size = SIZES[0]
    want, counters = _model(rrt, orc, "helmet", size, 1, ARMS[2])
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=4, output_image_dimensions=size, output_image_path="/dev/null", seed_mode=1,
                                             traversal=L.TRAVERSAL_CULLED))
    host, st_h = r.render_features(sc, features=F.NAMES, flags=L.FLAG_COUNT)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = torch.ones((1 << 22,), device="cuda").cumsum(0)                 # work in front of the pass on the side stream
        dev, st_d = r.render_features(sc, features=F.NAMES, device=True, flags=L.FLAG_COUNT)
        dev2, _ = r.render_features(sc, cameras=[sc.camera, sc.camera.uniform], features=("normal", "prim"), device=True, stream=side)
    side.synchronize()
    assert busy[-1].item() == float(1 << 22)
    for k in F.NAMES:
        assert host[k].shape == want[k].shape[:0] + (1,) + want[k].shape and dev[k].is_cuda and tuple(dev[k].shape) == host[k].shape
        assert F.same_bits(host[k][0], want[k]) and F.same_bits(dev[k].cpu().numpy()[0], want[k]), k
    assert _same_counters(st_h, counters) and _same_counters(st_d, counters)
    assert set(dev2) == {"normal", "prim"} and tuple(dev2["normal"].shape) == (2, size[1], size[0], 3)
    for v in (0, 1):
        assert F.same_bits(dev2["normal"].cpu().numpy()[v], want["normal"]) and F.same_bits(dev2["prim"].cpu().numpy()[v], want["prim"])
    default, _ = r.render_features(sc)                                         # depth, normal, albedo of the scene's camera
    assert set(default) == {"depth", "normal", "albedo"} and F.same_bits(default["depth"][0], want["depth"])


def test_replica_handle_gives_the_same_buffers(rrt, orc):
    sc = _scene(rrt, "cornell")
    size = SIZES[0]
    want, counters = _model(rrt, orc, "cornell", size, 0, ARMS[2])
    multi = sc.upload_multi([0])
    replica = rrt.load().mipt_multi_scene(multi, 0)
    for device in (False, True):
        got, st = _features(rrt, replica, [sc.camera], size, 0, ARMS[2], device=device)
        assert not _same(got, want, view=0) and _same_counters(st, counters), device


def test_cpp_mirror_matches_the_python_binding(rrt, tmp_path):
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth
    obj = synth.write_cornell_obj(str(tmp_path))
    exe = str(tmp_path / "test_host_features")
    lib_dir = os.path.join(ROOT, "rust_ray_tracing_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_host_features.cpp"),
                           "-o", exe, "-L", lib_dir, "-l:libmipt.so", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    pos, pitch, yaw = synth.CORNELL_CAMERA
    out = subprocess.run([exe, "gpu", obj, str(tmp_path / "out.bin")] + [repr(float(x)) for x in pos] + [repr(float(pitch)), repr(float(yaw))],
                         capture_output=True, text=True)
    assert out.returncode == 0 and "gpu ok" in out.stdout, out.stdout + out.stderr
    sc = rrt.Scene.load(obj)                                                   # the same loader and BVH::build the C++ mirror calls
    sc.set_camera(rrt.Camera(position=pos, pitch=pitch, yaw=yaw))
    r = rrt.Renderer.new(rrt.RendererOptions(samples=2, max_ray_depth=3, output_image_dimensions=(24, 16), output_image_path="/dev/null", seed_mode=1,
                                             traversal=L.TRAVERSAL_REFERENCE))
    py, _ = r.render_features(sc, features=F.NAMES)
    want = b"".join(np.ascontiguousarray(py[k]).tobytes() for k in F.NAMES)
    assert (tmp_path / "out.bin").read_bytes() == want


# ---- errors: status, a message naming the field, and the scene as before ----------------------------------------------------------------
def test_errors_leave_the_scene_rendering_and_querying(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc = _scene(rrt, "cornell")
    size = SIZES[0]
    want, counters = _model(rrt, orc, "cornell", size, 0)
    before = _render(rrt, sc).copy()
    w, h = size
    n = w * h
    table = _cam_table([sc.camera])
    d_buf = torch.full((n * 3 + 4,), POISON_I, dtype=torch.int32, device="cuda")
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
        b = L.MiptFeatureBuffers()
        b.depth = ptr
        for k, v in kw.items():
            if k == "reserved":
                b.reserved[v] = ptr
            else:
                setattr(b, k, v)
        return b

    option_cases = [
        (dict(width=0), "width"), (dict(samples=0), "samples"), (dict(max_ray_depth=0), "max_ray_depth"), (dict(seed_mode=3), "seed_mode"),
        (dict(samples=3), "MIPT_SEED_PIXEL_STREAM"), (dict(traversal=5), "traversal"), (dict(cull_margin=2.0), "cull_margin"),
        (dict(flags=L.FLAG_TOUCHED | L.FLAG_COUNT), "flags"), (dict(tile_world=4), "tile_world"), (dict(tile_rank=1), "tile_rank"),
        (dict(shading=L.SHADING_WGPU), "shading"), (dict(reserved=1), "reserved"), (dict(width=1 << 15, height=1 << 15), "below 2^32"),
    ]
    for device in (False, True):
        ptr = d_buf.data_ptr() if device else h_buf.ctypes.data
        f = lib.mipt_render_features_device if device else lib.mipt_render_features
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
                          ((sc._handle, L.ptr(table), 1, C.byref(opts()), C.byref(bufs(None))), "no buffer wanted"),
                          ((sc._handle, L.ptr(table), 1, C.byref(opts()), C.byref(bufs(ptr, reserved=2))), "reserved buffer pointers")]:
            assert f(*args, *tail) == L.ERR_INVALID_ARG, (msg, device)
            assert msg in lib.mipt_last_error().decode(), (msg, lib.mipt_last_error())
    # the device entry: host memory, and a pointer that is not 4-byte aligned
    f = lib.mipt_render_features_device
    assert f(sc._handle, L.ptr(table), 1, C.byref(opts()), C.byref(bufs(h_buf.ctypes.data)), None, None) == L.ERR_INVALID_ARG
    assert "depth is not device memory" in lib.mipt_last_error().decode()
    assert f(sc._handle, L.ptr(table), 1, C.byref(opts()), C.byref(bufs(d_buf.data_ptr(), normal=h_buf.ctypes.data)), None, None) == L.ERR_INVALID_ARG
    assert "normal is not device memory" in lib.mipt_last_error().decode()
    assert f(sc._handle, L.ptr(table), 1, C.byref(opts()), C.byref(bufs(d_buf.data_ptr(), uv=d_buf.data_ptr() + 2)), None, None) == L.ERR_INVALID_ARG
    assert "uv must be 4-byte aligned" in lib.mipt_last_error().decode()
    assert np.all(h_buf == POISON_F) and bool(torch.all(d_buf == POISON_I))   # no refused call wrote anything
    # the scene renders, queries and gives its features as before
    assert np.array_equal(_render(rrt, sc), before)
    got, st = _features(rrt, sc._handle, [sc.camera], size)
    assert not _same(got, want, view=0) and _same_counters(st, counters)
    rays = F.camera_rays(orc, sc, sc.camera.uniform, w, h, 0, pixels=np.arange(0, n, 37))[0]
    hits, _ = sc.query_closest(rays.view(np.float32).reshape(-1, 8))
    assert F.same_bits(hits["t"], want["depth"].reshape(-1)[::37])
