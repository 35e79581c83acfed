"""CPU: the model of the first-hit feature buffers (tests/tools/features_model.py) is held to the oracle -- a depth-1 render is what
ray.rs:177,197-201 and cpu.rs:52,60 make of the first hit's albedo and emission, for hits and misses alike -- and the argument checks
of mipt_render_features / _device and of the C++ mirror's methods run before anything touches the scene or a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import features_model as F  # noqa: E402
import query_model as Q  # noqa: E402

W, H = 40, 24
ENTRIES = ("mipt_render_features", "mipt_render_features_device")


def _scene(rrt, kind):
    from rust_ray_tracing_amd import synth
    kw = dict(n_target=2000, tex_size=32) if kind == "helmet" else {}
    tris, mats, texs, cam = synth.make_scene(kind, **kw)
    sc = rrt.Scene.from_arrays(tris, mats, texs)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    return sc


_frames = {}


def _frame(rrt, orc, kind, seed_mode):
    """(Scene, model frame, counters, the oracle's recorded (tri, t)) -- computed once and left unchanged"""
    if (kind, seed_mode) not in _frames:
        sc = _scene(rrt, kind)
        _frames[kind, seed_mode] = (sc,) + F.frame(orc, sc, sc.camera.uniform, W, H, seed_mode)
    return _frames[kind, seed_mode]


@pytest.mark.parametrize("seed_mode", [0, 1])
@pytest.mark.parametrize("kind", ["cornell", "helmet"])
def test_model_radiance_is_the_oracles_depth_one_render(rrt, orc, kind, seed_mode):
    sc, out, counters, _ = _frame(rrt, orc, kind, seed_mode)
    hdr, _, st = orc.render(sc.tris, sc.bvh_nodes, sc.materials_array(), sc.textures, sc.camera.uniform, W, H, 1, 1, seed_mode=seed_mode,
                            want_rgba8=False)
    hit = out["prim"] != Q.NONE
    assert 0 < hit.sum() < hit.size or kind == "cornell"              # the helmet frame holds hits and sky
    assert hit.any()
    assert F.same_bits(F.radiance(out["albedo"], out["emission"]), hdr), (kind, seed_mode)
    for k in ("rays", "inner_steps", "tri_tests", "hits", "texel_fetches", "max_stack"):
        assert counters[k] == st[k], (k, counters[k], st[k])
    assert counters["pixels"] == W * H and counters["rays"] == W * H
    if kind == "helmet":
        assert counters["texel_fetches"] > 0
    # a miss is HitInfo::default and the sky
    miss = ~hit
    if miss.any():
        assert np.all(out["depth"][miss] == np.float32(1e30)) and np.all(out["material"][miss] == 0xFFFFFFFF)
        assert not out["position"][miss].any() and not out["uv"][miss].any() and not out["normal"][miss].any()
        assert np.all(out["albedo"][miss] == 1.0) and np.all(out["emission"][miss] == 1.0)


@pytest.mark.parametrize("seed_mode", [0, 1])
@pytest.mark.parametrize("kind", ["cornell", "helmet"])
def test_model_depth_and_triangle_are_the_oracles(rrt, orc, kind, seed_mode):
    sc, out, _, (rec_tri, rec_t) = _frame(rrt, orc, kind, seed_mode)
    assert F.same_bits(out["depth"].reshape(-1), rec_t)
    prim = out["prim"].reshape(-1)
    tree = np.where(prim == Q.NONE, Q.NONE, prim & 0x01FFFFFF).astype(np.uint32)     # host-built scene: the caller's order is the tree's
    assert np.array_equal(tree, rec_tri)
    hit = prim != Q.NONE
    assert np.array_equal(out["material"].reshape(-1)[hit], sc.tris["material_id"][tree[hit]])


def test_model_mean_over_samples(rrt, orc):
    """PER_SAMPLE: sample s of a call starting at sample_begin is the single-sample frame of sample number sample_begin + s, and the
    mean is +0, the samples in order, one division"""
    sc = _scene(rrt, "helmet")
    w, h = 9, 5
    singles = [F.frame(orc, sc, sc.camera.uniform, w, h, 1, 1, s)[0] for s in (5, 6, 7)]
    three, counters, _ = F.frame(orc, sc, sc.camera.uniform, w, h, 1, 3, 5)
    for k in ("depth", "prim", "material", "position", "uv"):
        assert F.same_bits(three[k], singles[0][k]), k
    for k in ("normal", "albedo", "emission"):
        # a single-sample frame holds (0 + v) / 1, which is v but for the sign of a zero
        acc = ((np.float32(0) + singles[0][k]) + singles[1][k]) + singles[2][k]
        assert F.same_bits(three[k], acc / np.float32(3)), k
    assert counters["rays"] == 3 * w * h
    assert not F.same_bits(singles[0]["position"], singles[1]["position"])           # the samples do differ
    first, _, _ = F.frame(orc, sc, sc.camera.uniform, w, h, 1, 1, 0)
    one, _, _ = F.frame(orc, sc, sc.camera.uniform, w, h, 1, 1, 1)
    assert all(F.same_bits(first[k], one[k]) for k in F.NAMES)                       # sample_begin 0 is sample 1


@pytest.mark.parametrize("arm", [(False, 0.0), (True, 0.0078125)], ids=["ref", "cullsafe"])
def test_batch_cameras_refill_waves_that_are_mid_traversal(rrt, orc, arm):
    """What makes tests/test_gpu_features.py::test_more_views_than_the_launch_holds_lanes reach first_hit_kernel's partial refill: the
    views of its four cameras hold sky pixels, over after the root's step, and hits of sixteen steps or more in the same tiles, and
    the kernel's scheduling rule (query_model.wave_refills at ray_query.hip's ratio 1/4, which first_hit.hip restates) fed their step
    counts in work-item order -- view, tile, pixel of the tile, the ragged edge skipped -- then hands a wave new pixels while other
    lanes are mid-traversal: with the wave alone on the queue, and with blocks at seeded random bases."""
    sc = _scene(rrt, "helmet")
    w, h = 61, 37                                                     # test_gpu_features.py SIZES[0]
    cams = F.batch_cameras(rrt, sc.camera)
    steps = [F.pixel_steps(orc, sc, c.uniform, w, h, 0, cull=arm[0], margin=arm[1]) for c in cams]
    for s in steps:
        assert s.min() >= 1 and (s <= Q.SHORT_MAX_STEPS).sum() > w * h // 8 and (s >= Q.LONG_MIN_STEPS).sum() > w * h // 20
        tiles = F.work_order_steps([s]).reshape(-1, 64)
        mixed = ((tiles >= Q.LONG_MIN_STEPS).any(axis=1) & ((tiles > 0) & (tiles <= Q.SHORT_MAX_STEPS)).any(axis=1)).sum()
        assert mixed >= 1, mixed                                      # a silhouette tile in every view
    cycle = F.batch_cycle(2 * len(cams))
    assert all(cycle[i] != cycle[i + 1] for i in range(len(cycle) - 1)) and set(cycle) == set(range(len(cams)))
    order = F.work_order_steps([steps[c] for c in cycle])
    assert len(order) == len(cycle) * 40 * 64 and (order == 0).sum() == len(cycle) * (40 * 64 - w * h)
    alone = Q.wave_refills(order, None, skips=True)
    assert alone > 0, "no refill into a partly busy wave with sequential bases"
    bases = np.random.default_rng(23).integers(0, len(order) - 64, 48)
    scattered = Q.wave_refills(order, bases, skips=True)
    assert scattered > 0, "no refill into a partly busy wave with random bases"
    # the rule without skips is the query kernel's own: an order with none gives the same count either way
    dense = order[order > 0]
    assert Q.wave_refills(dense, None) == Q.wave_refills(dense, None, skips=True)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_feature_symbols_and_struct_size(rrt):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    assert C.sizeof(L.MiptFeatureBuffers) == 96
    assert [n for n, _ in L.MiptFeatureBuffers._fields_] == list(F.NAMES) + ["reserved"]
    assert tuple(n for n, _, _ in L.FEATURES) == F.NAMES and {n: k for n, k, _ in L.FEATURES} == F.WIDTH
    for s in ENTRIES:
        assert s in L.EXPORTS and getattr(lib, s).restype is C.c_int
        assert len(getattr(lib, s).argtypes) == (7 if s.endswith("_device") else 6)
    src = open(os.path.join(ROOT, "rust_ray_tracing_amd", "csrc", "mipt_features.cpp")).read()
    assert "sizeof(MiptFeatureBuffers) == 96" in src                                 # the C side of the same claim
    assert lib.mipt_abi_version() == 4


def _opts(rrt, **kw):
    o = rrt.make_options(8, 4, 1, 1)
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


@pytest.mark.parametrize("which", ENTRIES)
def test_feature_argument_errors_without_a_device(rrt, which):
    """Refused with a message that names the field before the scene is touched: the scene argument is an opaque non-null handle the
    checks never dereference.  (Pointers that are not device memory of the scene's device need a scene: tests/test_gpu_features.py.)"""
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    device = which.endswith("_device")
    handle = C.c_void_p(0x1000)
    cams = np.zeros(4, dtype=L.CAMERA)
    store = np.zeros(2 * 8 * 4 * 3 + 4, dtype=np.float32)

    def bufs(**kw):
        b = L.MiptFeatureBuffers()
        for k, v in kw.items():
            if k == "reserved":
                b.reserved[v] = store.ctypes.data
            else:
                setattr(b, k, v)
        return b

    good = bufs(depth=store.ctypes.data, albedo=store.ctypes.data)
    nan = float("nan")
    cases = [
        ("null scene", None, cams, 2, _opts(rrt), good, "null scene, cameras, opt or buffers"),
        ("null cameras", handle, None, 2, _opts(rrt), good, "null scene, cameras, opt or buffers"),
        ("null opt", handle, cams, 2, None, good, "null scene, cameras, opt or buffers"),
        ("null buffers", handle, cams, 2, _opts(rrt), None, "null scene, cameras, opt or buffers"),
        ("no views", handle, cams, 0, _opts(rrt), good, "n_views"),
        ("no buffer wanted", handle, cams, 2, _opts(rrt), bufs(), "no buffer wanted"),
        ("reserved[0]", handle, cams, 2, _opts(rrt), bufs(depth=store.ctypes.data, reserved=0), "reserved buffer pointers"),
        ("reserved[3]", handle, cams, 2, _opts(rrt), bufs(depth=store.ctypes.data, reserved=3), "reserved buffer pointers"),
        ("width 0", handle, cams, 2, _opts(rrt, width=0), good, "width"),
        ("height 0", handle, cams, 2, _opts(rrt, height=0), good, "height"),
        ("samples 0", handle, cams, 2, _opts(rrt, samples=0), good, "samples"),
        ("depth 0", handle, cams, 2, _opts(rrt, max_ray_depth=0), good, "max_ray_depth"),
        ("seed mode", handle, cams, 2, _opts(rrt, seed_mode=2), good, "seed_mode"),
        ("two samples of the pixel stream", handle, cams, 2, _opts(rrt, samples=2), good, "only one sample is defined without path tracing"),
        ("traversal", handle, cams, 2, _opts(rrt, traversal=2), good, "traversal"),
        ("negative margin", handle, cams, 2, _opts(rrt, cull_margin=-0.5), good, "cull_margin"),
        ("NaN margin", handle, cams, 2, _opts(rrt, cull_margin=nan), good, "cull_margin"),
        ("SUM", handle, cams, 2, _opts(rrt, flags=L.FLAG_SUM), good, "flags"),
        ("COUNT | PACKED", handle, cams, 2, _opts(rrt, flags=L.FLAG_COUNT | L.FLAG_PACKED), good, "flags"),
        ("tile_world 2", handle, cams, 2, _opts(rrt, tile_world=2), good, "tile_world"),
        ("wgpu shading", handle, cams, 2, _opts(rrt, shading=L.SHADING_WGPU), good, "out of scope"),
        ("shading 7", handle, cams, 2, _opts(rrt, shading=7), good, "shading"),
        ("reserved option", handle, cams, 2, _opts(rrt, reserved=2), good, "reserved option fields"),
        ("2^32 pixels", handle, cams, 4, _opts(rrt, width=1 << 15, height=1 << 15), good, "below 2^32"),
        ("seed range", handle, cams, 1, _opts(rrt, width=1 << 16, height=1 << 15), good, "pixel seed"),
    ]
    if device:
        cases.append(("unaligned depth", handle, cams, 2, _opts(rrt), bufs(depth=store.ctypes.data + 2, albedo=store.ctypes.data), "depth must be 4-byte aligned"))
        cases.append(("unaligned emission", handle, cams, 2, _opts(rrt), bufs(emission=store.ctypes.data + 1), "emission must be 4-byte aligned"))
    for name, sc, cm, n, o, b, msg in cases:
        args = [sc, L.ptr(cm) if cm is not None else None, n, C.byref(o) if o is not None else None, C.byref(b) if b is not None else None]
        args += ([None] if device else []) + [None]
        assert getattr(lib, which)(*args) == L.ERR_INVALID_ARG, name
        err = lib.mipt_last_error().decode()
        assert msg in err and err.startswith(which + ":"), (name, err)
    assert not store.any()


def test_python_wrapper_rejects_bad_feature_lists_before_the_library(rrt):
    r = rrt.Renderer.new(rrt.RendererOptions(output_image_dimensions=(8, 4), output_image_path="/dev/null"))
    sc = rrt.Scene()                                             # never uploaded: the checks below come first
    for bad in ((), ("depth", "depth"), ("colour",), ("depth", "normals")):
        with pytest.raises(ValueError):
            r.render_features(sc, features=bad)
    with pytest.raises(ValueError):
        r.render_features(sc, cameras=[])


def test_cpp_feature_methods_check_arguments_without_a_device(built, tmp_path):
    exe = str(tmp_path / "test_host_features")
    lib_dir = os.path.join(ROOT, "rust_ray_tracing_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_host_features.cpp"),
                           "-o", exe, "-L", lib_dir, "-l:libmipt.so", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "cpu ok" in out.stdout, out.stdout + out.stderr
