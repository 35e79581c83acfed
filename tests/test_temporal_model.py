"""CPU: the model of the temporal accumulation (tests/tools/temporal_model.py) does what the contract of include/mipt.h promises -- a
frame's own positions reproject onto its own pixels through the oracle's camera, a static camera with constant radiance leaves the
frame unchanged while the history length counts up, a moving 1-spp sequence of the oracle comes out closer to the converged frame
than denoising alone, and the moved-camera inputs reach every branch -- and every argument check of mipt_temporal /
mipt_temporal_device / Renderer.temporal runs before any device work."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import denoise_model as D  # noqa: E402
import features_model as FM  # noqa: E402
import temporal_model as T  # noqa: E402

_atrium = {}


def _scene(rrt, orc):
    """the 20 k-triangle atrium with the oracle's BVH, built once"""
    if not _atrium:
        from rust_ray_tracing_amd import _lib as L
        from rust_ray_tracing_amd import synth
        tris, mats, texs, cam = synth.make_scene("atrium", n_target=20000, tex_size=64)
        sc = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
        t, nodes = orc.bvh_build(sc.tris)
        sc.tris, sc.bvh_nodes = t, nodes.view(L.NODE).reshape(-1)
        _atrium.update(scene=sc, pose=cam, guides={})
    return _atrium


def _camera(rrt, pose, dp=(0.0, 0.0, 0.0), dpitch=0.0, dyaw=0.0):
    c = rrt.Camera(position=tuple(float(pose[0][i]) + dp[i] for i in range(3)), pitch=pose[1] + dpitch, yaw=pose[2] + dyaw)
    c.update_view()
    return c.uniform


def _guides(rrt, orc, camera, w, h, seed_mode=1):
    """the first-hit buffers of the oracle for this camera (features_model.frame), computed once per input"""
    a = _scene(rrt, orc)
    key = (camera.tobytes(), w, h, seed_mode)
    if key not in a["guides"]:
        a["guides"][key] = FM.frame(orc, a["scene"], camera, w, h, seed_mode)[0]
    return a["guides"][key]


def _step(g, hdr, camera, history=None, albedo=True, **kw):
    return T.step(hdr, g["position"], g["normal"], g["depth"], g["material"], [camera], history, g["albedo"] if albedo else None, **kw)


# ---- reprojection against the oracle's camera --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed_mode", [0, 1])
@pytest.mark.parametrize("size", [(64, 36), (37, 61)], ids=["64x36", "37x61"])
def test_a_frame_reprojects_onto_itself(rrt, orc, size, seed_mode):
    """A frame's own first-hit positions through its own camera record: every hit pixel comes back at its own (column, row).  The
    camera ray carries the jitter of cpu.rs:38-42, at most 0.0005 in screen units = 0.00025 * H pixels (the same in x: the aspect
    cancels); 1e-3 pixel is left for the f32 arithmetic of the ray, the hit point and the projection.  The hit distance agrees with
    |position - C|: both carry a dozen f32 roundings of 2^-24 each, so 2e-6 relative bounds their difference."""
    w, h = size
    a = _scene(rrt, orc)
    cam = _camera(rrt, a["pose"])
    g = _guides(rrt, orc, cam, w, h, seed_mode)
    _, vz, fx, fy, d2 = T.project(g["position"], T.camera_record(cam), w, h)
    hit = g["depth"] < T.MISS
    assert hit.sum() > 0.5 * w * h and (vz[hit] > 0).all()
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    err = float(np.maximum(np.abs(fx - xs), np.abs(fy - ys))[hit].max())
    z = g["depth"][hit].astype(np.float64)
    rel = float((np.abs(d2[hit] - z * z) / d2[hit]).max())
    print(f"{w}x{h} seed mode {seed_mode}: largest reprojection error {err:.6f} pixels (bound {0.00025 * h + 1e-3:.5f}), |d2 - depth^2| / d2 <= {rel:.3g}")
    assert err <= 0.00025 * h + 1e-3
    assert rel <= 2e-6


# ---- a static camera -------------------------------------------------------------------------------------------------------------
def _exact_plane(w, h):
    """a camera whose record is the identity at the origin and the plane z = 1 seen through it: with W and H powers of two every
    operation of the projection is exact, so each pixel reprojects onto its own integer coordinates with one tap of weight 1"""
    cam = np.zeros((), dtype=[("look_at", "<f4", (4, 4)), ("position", "<f4", 3), ("_pad", "<f4")])
    cam["look_at"] = np.eye(4, dtype=np.float32)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    sx = (((xs / np.float32(w)) * 2) - 1) * np.float32(w / h)                     # cpu.rs:31-35
    sy = (((np.float32(h) - ys) / np.float32(h)) * 2) - 1
    position = np.stack([-sx, sy, np.ones_like(sx)], axis=-1).astype(np.float32)  # cpu.rs:44 with look_at = identity, t = 1
    depth = np.sqrt((position ** 2).sum(-1)).astype(np.float32)
    normal = np.zeros((h, w, 3), dtype=np.float32)
    normal[..., 2] = -1.0
    return cam, dict(position=position, normal=normal, depth=depth, material=np.full((h, w), 3, dtype=np.uint32), albedo=None)


def test_static_camera_constant_radiance_counts_the_history_up():
    w, h = 8, 4
    cam, g = _exact_plane(w, h)
    assert np.array_equal(T.camera_record(cam)[:12], np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]))
    rng = np.random.default_rng(5)
    hdr = (rng.random((h, w, 3)) * 3.0).astype(np.float32)                          # any radiance, the same every frame
    hist = None
    for f in range(8):
        r = _step(g, hdr, cam, hist, albedo=False, max_history=5.0)
        hist = r["history"]
        # the three other taps have weight 0; some lie outside the frame or fail the depth check, so the tap count varies
        assert (r["cls"] == T.FIRST).all() if f == 0 else (r["cls"] >= T.REUSED4).all()
        assert np.array_equal(r["out"].view(np.uint32), hdr.view(np.uint32)), f    # unchanged bit for bit
        assert (r["length"] == min(f + 1, 5)).all(), f
        assert (r["variance"] == 0).all()
        rec, p0, p1, p2 = T.unpack_history(hist, 1, h, w)
        assert np.array_equal(p0[0, ..., 3], r["length"]) and np.array_equal(p1[0, ..., 3], g["depth"]) and (p2[0, ..., 2] == 3).all()
        assert not p2[0, ..., 3].any() and not rec[0, 12:].any()


def test_static_camera_on_the_atrium_keeps_a_constant_frame(rrt, orc):
    """radiance 1.0 everywhere: sum(w * 1) is sum(w) bit for bit whatever the taps, so every pixel stays exactly 1.0, reused or reset"""
    w, h = 64, 36
    a = _scene(rrt, orc)
    cam = _camera(rrt, a["pose"])
    g = _guides(rrt, orc, cam, w, h)
    hdr = np.ones((h, w, 3), dtype=np.float32)
    hist, reused = None, 0
    for f in range(4):
        r = _step(g, hdr, cam, hist, albedo=False)
        hist = r["history"]
        assert np.array_equal(r["out"].view(np.uint32), hdr.view(np.uint32)), f
        # sum(w * len) / sum(w) of equal lengths is that length up to a few roundings of 2^-24 per frame
        assert (r["length"] <= (f + 1) * (1 + 1e-5)).all() and (r["length"] >= 1).all()
        reused = int((r["cls"] >= T.REUSED4).sum())
    assert reused > 0.8 * w * h and abs(float(r["length"].max()) - 4.0) <= 4e-5


# ---- quality and coverage on a moving camera --------------------------------------------------------------------------------------
def test_accumulation_beats_denoising_alone(rrt, orc):
    """The atrium at 64x36, depth 8, 1 spp, per-sample seeds with sample_begin = 1 + f, 8 frames of a camera that moves by
    (0.02, 0, 0.01) and yaws by 0.4 degrees per frame; the target is 1024 samples from 1000 at the last camera.  The exact model
    gives RMSE noisy 0.1867, accumulated 0.0759 (ratio 0.407), denoised only 0.0602, accumulated then denoised 0.0420 (ratio 0.698),
    2004-2036 of 2304 pixels reused per frame."""
    w, h = 64, 36
    a = _scene(rrt, orc)
    sc = a["scene"]
    hist, results = None, []
    for f in range(8):
        cam = _camera(rrt, a["pose"], dp=(0.02 * f, 0.0, 0.01 * f), dyaw=0.4 * f)
        args = (sc.tris, sc.bvh_nodes, sc.materials_array(), sc.textures, cam, w, h)
        noisy = orc.render(*args, 1, 8, seed_mode=1, sample_begin=1 + f, want_rgba8=False)[0]
        g = _guides(rrt, orc, cam, w, h)
        r = _step(g, noisy, cam, hist, **T.DEFAULTS)
        hist = r["history"]
        results.append(r)
        print(f"frame {f}: {int((r['cls'] >= T.REUSED4).sum())} of {w * h} pixels reused")
    target = orc.render(*args, 1024, 8, seed_mode=1, sample_begin=1000, want_rgba8=False)[0]
    den = lambda x: D.denoise(orc, x, g["normal"], g["depth"], g["albedo"], iterations=5, sigma_color=4.0, sigma_normal=0.5, sigma_depth=0.5)  # noqa: E731
    acc, acc_den, only_den = r["out"], den(r["out"]), den(noisy)
    e_noisy, e_acc, e_den, e_acc_den = (D.rmse(x, target) for x in (noisy, acc, only_den, acc_den))
    print(f"rmse noisy {e_noisy:.4f}, accumulated {e_acc:.4f} ({e_acc / e_noisy:.3f} x), denoised only {e_den:.4f}, accumulated then denoised "
          f"{e_acc_den:.4f} ({e_acc_den / e_den:.3f} x)")
    for x in (acc, acc_den, r["length"], r["variance"]):
        assert np.isfinite(x).all()
    assert e_acc <= 0.5 * e_noisy
    assert e_acc_den <= 0.8 * e_den


def test_the_moved_camera_reaches_every_class(rrt, orc):
    """the first frame from the camera of T.COVERAGE_MOVE, the second from the scene's: every class and rejection reason occurs"""
    w, h = 64, 36
    a = _scene(rrt, orc)
    before, now = _camera(rrt, a["pose"], **T.COVERAGE_MOVE), _camera(rrt, a["pose"])
    hdr = np.ones((h, w, 3), dtype=np.float32)
    first = _step(_guides(rrt, orc, before, w, h), hdr, before)
    second = _step(_guides(rrt, orc, now, w, h), hdr, now, first["history"])
    seen = T.classes_present([first, second])
    print({name: int((second["cls"] == k).sum()) for k, name in enumerate(T.CLASS_NAMES)})
    assert seen == T.ALL_CLASSES, T.ALL_CLASSES - seen


def test_special_values_take_the_reset_side():
    """NaN position, depth or record and an infinite position reset the pixel; a NaN in the history stays where the taps reach it"""
    w, h = 8, 4
    cam, g = _exact_plane(w, h)
    hdr = np.full((h, w, 3), 0.5, dtype=np.float32)
    h0 = _step(g, hdr, cam, albedo=False)["history"]
    g2 = {k: (v.copy() if v is not None else None) for k, v in g.items()}
    g2["position"][0, 0, 0] = np.nan
    g2["position"][0, 1, 2] = np.inf
    g2["depth"][0, 2] = np.nan
    g2["depth"][0, 3] = 1e30
    g2["material"][1, 0] = 0xFFFFFFFF
    g2["normal"][1, 1, 0] = np.nan
    r = _step(g2, hdr, cam, h0, albedo=False)
    assert r["cls"][0, 2] == T.MISSED and r["cls"][0, 3] == T.MISSED
    assert r["cls"][0, 0] in (T.BEHIND, T.OFF_FRAME) and r["cls"][0, 1] in (T.BEHIND, T.OFF_FRAME)
    assert r["cls"][1, 0] == T.THIN and r["rejects"][1, 0] == T.REJ_MATERIAL
    assert r["cls"][1, 1] == T.THIN and r["rejects"][1, 1] == T.REJ_NORMAL
    assert (r["length"][0, :4] == 1).all() and (r["length"][1, :2] == 1).all() and (r["cls"][2:] >= T.REUSED4).all() and (r["length"][2:] == 2).all()
    assert np.isfinite(r["out"]).all()
    _, p0, _, _ = T.unpack_history(h0, 1, h, w)
    p0[0, 3, 5, 0] = np.nan
    r = _step(g, hdr, cam, h0, albedo=False)
    assert np.isnan(r["out"][3, 5, 0]) and np.isfinite(r["out"]).sum() == r["out"].size - 1


# ---- the argument checks: before any device work, each message names its field -----------------------------------------------------
W, H, V = 6, 4, 2
N = W * H * V
WORDS = dict(hdr=3, position=3, normal=3, depth=1, material=1, albedo=3, out=3, length=1, variance=1)
HIST_BYTES = 64 * V + 48 * N


def _opt(L, **kw):
    o = L.MiptTemporalOptions()
    o.width, o.height, o.n_views = W, H, V
    o.alpha_min, o.max_history, o.normal_tol, o.depth_tol = 0.0, 32.0, 0.1, 0.1
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


class _Planes:
    """host planes for one call; two 16-byte aligned histories"""

    def __init__(self):
        self.a = {k: np.zeros(N * n + 4 + 3 * N, dtype=np.float32) for k, n in WORDS.items()}   # + 3 N words: a case that moves a pointer to a plane's end stays inside that plane's own allocation, whatever lies behind it on the heap
        for k in ("history_in", "history_out"):
            raw = np.zeros(HIST_BYTES // 4 + 8, dtype=np.float32)
            off = (-raw.ctypes.data % 16) // 4
            self.a[k] = raw[off: off + HIST_BYTES // 4]
            assert self.a[k].ctypes.data % 16 == 0

    def bufs(self, L, **kw):
        b = L.MiptTemporalBuffers()
        for k, a in self.a.items():
            setattr(b, k, a.ctypes.data)
        for k, v in kw.items():
            if k == "reserved":
                b.reserved[v] = self.a["hdr"].ctypes.data
            else:
                setattr(b, k, v)
        return b


def _cameras(rrt, n=V):
    from rust_ray_tracing_amd import _lib as L
    cams = np.zeros(n, dtype=L.CAMERA)
    for i in range(n):
        c = rrt.Camera(position=(0.5 * i, 1.0, -2.0), pitch=3.0 * i, yaw=20.0 + 7.0 * i)
        c.update_view()
        cams[i] = c.uniform
    return cams


def _calls(lib):
    """both entries with the same (opt, cameras, bufs) -> status"""
    return (("mipt_temporal", lambda o, c, b: lib.mipt_temporal(o, c, b, 0)),
            ("mipt_temporal_device", lambda o, c, b: lib.mipt_temporal_device(o, c, b, None)))


def test_struct_sizes_and_history_bytes(rrt):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    assert C.sizeof(L.MiptTemporalOptions) == 64 and C.sizeof(L.MiptTemporalBuffers) == 128
    assert lib.mipt_temporal_history_bytes(1920, 1080, 1) == 64 + 1920 * 1080 * 48
    assert lib.mipt_temporal_history_bytes(W, H, V) == HIST_BYTES == T.history_words(V, H, W) * 4
    assert lib.mipt_temporal_history_bytes(65535, 65535, 1) == 64 + 65535 * 65535 * 48
    assert lib.mipt_temporal_history_bytes(3, 2, 700) == 64 * 700 + 48 * 4200
    for bad in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (65536, 65536, 1), (1 << 15, 1 << 15, 4), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)):
        assert lib.mipt_temporal_history_bytes(*bad) == 0, bad


def test_argument_checks_of_both_entries(rrt):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    p = _Planes()
    cams = _cameras(rrt)
    inf, nan = float("inf"), float("nan")
    option_cases = [
        (dict(width=0), "width"), (dict(height=0), "height"), (dict(n_views=0), "n_views"),
        (dict(width=1 << 16, height=1 << 16, n_views=1), "below 2^32"),
        (dict(flags=1), "flags"), (dict(reserved=0), "reserved"), (dict(reserved=7), "reserved"),
        (dict(alpha_min=-0.01), "alpha_min"), (dict(alpha_min=1.5), "alpha_min"), (dict(alpha_min=nan), "alpha_min"),
        (dict(max_history=0.5), "max_history"), (dict(max_history=inf), "max_history"), (dict(max_history=nan), "max_history"),
        (dict(normal_tol=-1.0), "normal_tol"), (dict(normal_tol=inf), "normal_tol"), (dict(normal_tol=nan), "normal_tol"),
        (dict(depth_tol=-0.1), "depth_tol"), (dict(depth_tol=inf), "depth_tol"), (dict(depth_tol=nan), "depth_tol"),
    ]
    hdr = p.a["hdr"].ctypes.data
    hin, hout = p.a["history_in"].ctypes.data, p.a["history_out"].ctypes.data
    buffer_cases = [(dict(**{k: None}), f"null {k}") for k in ("hdr", "position", "normal", "depth", "material", "history_out", "out")] + [
        (dict(reserved=0), "reserved buffer pointers"), (dict(reserved=4), "reserved buffer pointers"),
        (dict(normal=hdr), "normal overlaps hdr"), (dict(albedo=hdr + 12 * N - 4), "albedo overlaps hdr"), (dict(out=hdr + 4), "out overlaps hdr"),
        (dict(out=p.a["albedo"].ctypes.data), "out overlaps albedo"), (dict(material=p.a["depth"].ctypes.data), "material overlaps depth"),
        (dict(history_out=hin), "history_out overlaps history_in"), (dict(history_out=hin + HIST_BYTES - 16), "history_out overlaps history_in"),
        (dict(history_in=hout + 64 * V), "history_out overlaps history_in"),
        (dict(out=hout + 16), "out overlaps history_out"), (dict(length=hin), "length overlaps history_in"),
        (dict(variance=p.a["length"].ctypes.data + 4 * N - 4), "variance overlaps length"), (dict(history_in=hdr), "history_in overlaps hdr"),
    ]
    for name, call in _calls(lib):
        for kw, msg in option_cases:
            assert call(C.byref(_opt(L, **kw)), L.ptr(cams), C.byref(p.bufs(L))) == L.ERR_INVALID_ARG, (name, kw)
            err = lib.mipt_last_error().decode()
            assert msg in err and err.startswith(name + ":"), (name, kw, err)
        for kw, msg in buffer_cases:
            assert call(C.byref(_opt(L)), L.ptr(cams), C.byref(p.bufs(L, **kw))) == L.ERR_INVALID_ARG, (name, kw)
            err = lib.mipt_last_error().decode()
            assert msg in err and err.startswith(name + ":"), (name, kw, err)
        assert call(None, L.ptr(cams), C.byref(p.bufs(L))) == L.ERR_INVALID_ARG and "opt" in lib.mipt_last_error().decode()
        assert call(C.byref(_opt(L)), None, C.byref(p.bufs(L))) == L.ERR_INVALID_ARG and "cameras" in lib.mipt_last_error().decode()
        assert call(C.byref(_opt(L)), L.ptr(cams), None) == L.ERR_INVALID_ARG and "buffers" in lib.mipt_last_error().decode()
        # a singular camera is named with its view
        for damage in ("zero", "rank", "nan", "huge"):
            bad = cams.copy()
            if damage == "zero":
                bad[1]["look_at"][:] = 0.0
            elif damage == "rank":
                bad[1]["look_at"][1] = bad[1]["look_at"][0]
            elif damage == "nan":
                bad[1]["look_at"][2][1] = nan
            else:
                bad[1]["look_at"][:3, :3] = np.eye(3, dtype=np.float32)
                bad[1]["look_at"][2, 2] = 1e-45                                                # det 1.4e-45 in binary64: B[2][2] = 7e44 is no f32
            assert T.camera_record(bad[1]) is None and T.camera_record(bad[0]) is not None
            assert call(C.byref(_opt(L)), L.ptr(bad), C.byref(p.bufs(L))) == L.ERR_INVALID_ARG, (name, damage)
            assert "cameras[1].look_at" in lib.mipt_last_error().decode(), (name, damage, lib.mipt_last_error())
    # the optional planes and the first frame get past the checks: to the device (the host entry) or the device-memory check
    for kw in (dict(albedo=None), dict(history_in=None), dict(length=None, variance=None), dict(out=hdr)):
        rc = lib.mipt_temporal(C.byref(_opt(L)), L.ptr(cams), C.byref(p.bufs(L, **kw)), 0)
        assert rc in (L.OK, L.ERR_HIP), (kw, rc, lib.mipt_last_error())
        assert lib.mipt_temporal_device(C.byref(_opt(L)), L.ptr(cams), C.byref(p.bufs(L, **kw)), None) == L.ERR_INVALID_ARG
        assert "hdr is not device memory" in lib.mipt_last_error().decode()


def test_device_entry_checks_alignment_and_memory(rrt):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    p = _Planes()
    cams = _cameras(rrt)
    f = lib.mipt_temporal_device
    o = _opt(L)
    for name in WORDS:
        bad = p.bufs(L, **{name: p.a[name].ctypes.data + 2})
        assert f(C.byref(o), L.ptr(cams), C.byref(bad), None) == L.ERR_INVALID_ARG
        assert f"{name} must be 4-byte aligned" in lib.mipt_last_error().decode(), (name, lib.mipt_last_error())
    for name in ("history_in", "history_out"):
        for off in (4, 8):
            raw = np.zeros(HIST_BYTES // 4 + 8, dtype=np.float32)
            base = raw.ctypes.data + (-raw.ctypes.data % 16)
            bad = p.bufs(L, **{name: base + off})
            assert f(C.byref(o), L.ptr(cams), C.byref(bad), None) == L.ERR_INVALID_ARG
            assert f"{name} must be 16-byte aligned" in lib.mipt_last_error().decode(), (name, lib.mipt_last_error())
    # host memory is not device memory: refused by name, with or without a device
    assert f(C.byref(o), L.ptr(cams), C.byref(p.bufs(L)), None) == L.ERR_INVALID_ARG
    assert "hdr is not device memory" in lib.mipt_last_error().decode()


def test_host_entry_fails_loudly_without_a_device(rrt):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path is exercised on the CPU-only box")
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    p = _Planes()
    cams = _cameras(rrt)
    assert lib.mipt_temporal(C.byref(_opt(L)), L.ptr(cams), C.byref(p.bufs(L)), 0) == L.ERR_HIP
    assert "hipSetDevice" in lib.mipt_last_error().decode()
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=1, output_image_dimensions=(W, H), output_image_path="x.png"))
    z3, z1 = np.zeros((H, W, 3), dtype=np.float32), np.zeros((H, W), dtype=np.float32)
    with pytest.raises(rrt.MiptError) as e:
        r.temporal(z3, dict(position=z3.copy(), normal=z3.copy(), depth=z1, material=np.zeros((H, W), dtype=np.uint32)), cams[:1])
    assert e.value.code == L.ERR_HIP


def test_renderer_temporal_checks_its_arguments(rrt):
    from rust_ray_tracing_amd import _lib as L
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=1, output_image_dimensions=(W, H), output_image_path="x.png"))
    cams = _cameras(rrt)
    hdr = np.zeros((V, H, W, 3), dtype=np.float32)
    z = np.zeros((V, H, W), dtype=np.float32)
    feats = dict(position=hdr.copy(), normal=hdr.copy(), depth=z, material=np.zeros((V, H, W), dtype=np.uint32), albedo=hdr.copy())
    for kw, msg in [(dict(hdr=np.zeros((H, W), dtype=np.float32)), "hdr"), (dict(hdr=hdr.astype(np.float64)), "hdr"), (dict(position=z), "position"),
                    (dict(position=None), "position"), (dict(normal=hdr[0]), "normal"), (dict(depth=hdr), "depth"), (dict(depth=None), "depth"),
                    (dict(material=z), "material"), (dict(material=None), "material"), (dict(albedo=hdr[:, :, :, :2]), "albedo"),
                    (dict(albedo=z.astype(np.float64)), "albedo")]:
        f = dict(feats, **{k: v for k, v in kw.items() if k != "hdr"})
        with pytest.raises(ValueError) as e:
            r.temporal(kw.get("hdr", hdr), f, cams)
        assert str(e.value).startswith(msg + ":"), (kw, str(e.value))
    with pytest.raises(ValueError) as e:
        r.temporal(hdr, feats, cams[:1])
    assert str(e.value).startswith("cameras:")
    with pytest.raises(ValueError) as e:
        r.temporal(hdr, feats, cams, history=np.zeros(5, dtype=np.uint32))
    assert str(e.value).startswith("history:")
    import torch
    with pytest.raises(ValueError) as e:
        r.temporal(hdr, dict(feats, normal=torch.zeros((V, H, W, 3))), cams)
    assert str(e.value).startswith("normal:")
    with pytest.raises(ValueError) as e:
        r.temporal(torch.zeros((V, H, W, 3)), feats, cams)                   # a host tensor
    assert str(e.value).startswith("hdr:")
    # what the library checks comes back as its status and message
    for kw, msg in [(dict(alpha_min=2.0), "alpha_min"), (dict(max_history=0.0), "max_history"), (dict(normal_tol=-1.0), "normal_tol"),
                    (dict(depth_tol=float("nan")), "depth_tol")]:
        with pytest.raises(rrt.MiptError) as e:
            r.temporal(hdr, feats, cams, **kw)
        assert e.value.code == L.ERR_INVALID_ARG and msg in str(e.value), (kw, str(e.value))
    bad = cams.copy()
    bad[0]["look_at"][:] = 0.0
    with pytest.raises(rrt.MiptError) as e:
        r.temporal(hdr, feats, bad)
    assert e.value.code == L.ERR_INVALID_ARG and "cameras[0].look_at" in str(e.value)
    # the pixel stream repeats its noise every frame: render_sequence refuses it before anything else
    with pytest.raises(ValueError) as e:
        next(r.render_sequence(None, [cams[:1]]))
    assert "SEED_PER_SAMPLE" in str(e.value)
