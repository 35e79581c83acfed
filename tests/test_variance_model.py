"""CPU: the model of the variance-guided a-trous filter (tests/tools/variance_model.py) has the properties the contract of
include/mipt.h promises -- a constant frame and a converged frame come back as they went in, the variance of a flat noisy frame
follows the closed form, special values take the side the header names, and on the atrium sequences the filter is no worse than the
fixed-bandwidth one -- and every argument check of mipt_denoise_variance / mipt_denoise_variance_device / Renderer.denoise_variance
runs before any device work."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import denoise_model as D  # noqa: E402
import features_model as FM  # noqa: E402
import temporal_model as T  # noqa: E402
import variance_model as VM  # noqa: E402

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guides", list(itertools.product((False, True), repeat=2)), ids=lambda g: "normal%d-depth%d" % g)
def test_a_constant_frame_stays_constant(orc, guides):
    """colour 1.0 and variance 0 on two 7x5 views, 8 iterations (steps up to 128: most taps fall outside): sum w*1 is sum w bit for
    bit whatever the guides make of the weights, so every pixel stays exactly 1.0 -- with the spatial estimate and without"""
    rng = np.random.default_rng(11)
    hdr = np.ones((2, 5, 7, 3), dtype=F)
    kw = {}
    if guides[0]:
        kw["normal"] = rng.standard_normal((2, 5, 7, 3)).astype(F)
    if guides[1]:
        kw["depth"] = (rng.random((2, 5, 7)) * 3.0).astype(F)
    length = rng.integers(1, 9, (2, 5, 7)).astype(F)                   # both sides of short_history = 4
    for sh in (0.0, 4.0):
        out, _ = VM.denoise_variance(orc, hdr, np.zeros((2, 5, 7), dtype=F), length, iterations=8, short_history=sh, **kw)
        assert np.array_equal(_bits(out), _bits(hdr)), (guides, sh)


def test_converged_pixels_come_back_as_they_went_in(orc):
    """variance 0 and a history of at least short_history: kl = 1 / 1e-8, so a luminance difference above 128e-8 clamps e to 128
    and every off-centre weight is expf(-128) = 0.  The frame comes back as (9/64 * c) / (9/64) per iteration: one rounding of the
    product and one of the quotient, which together leave at most one ulp -- and the same value again in the next iteration, since
    the quotient of the rounded product is a fixed point.  This is the convergence the fixed filter lacks: it changes the frame."""
    h, w = 9, 11
    rng = np.random.default_rng(3)
    grey = (0.05 + 0.01 * rng.permutation(h * w).reshape(h, w)).astype(F)   # luminances at least 0.01 apart
    hdr = (grey[..., None] * np.array([1.0, 0.9, 1.1], dtype=F)).astype(F)
    lum = VM.luminance(hdr)
    gaps = np.abs(lum.reshape(-1, 1) - lum.reshape(1, -1))[~np.eye(h * w, dtype=bool)]
    assert gaps.min() > 128e-8
    zero, long_ = np.zeros((h, w), dtype=F), np.full((h, w), 4.0, dtype=F)
    out, var = VM.denoise_variance(orc, hdr, zero, long_, iterations=5, short_history=4.0)
    ulps = np.abs(out.view(np.int32).astype(np.int64) - hdr.view(np.int32).astype(np.int64))
    print(f"converged frame: at most {int(ulps.max())} ulp from the input, {int((ulps > 0).sum())} of {ulps.size} values moved")
    assert ulps.max() <= 1
    assert not var.any()
    fixed = D.denoise(orc, hdr, iterations=5)
    assert D.rmse(fixed, hdr) > 0.01                                    # the fixed filter blurs the same frame


def test_variance_of_a_flat_frame_follows_the_closed_form(orc):
    """no guides, constant colour, variance 1, one iteration: every e is 0 and w = h[dy+2]*h[dx+2], so an interior pixel gets
    variance_out = sum(w^2) / (sum w)^2 = (sum h^2)^2 = (70/256)^2.  sv and wsum are 25 additions each, every one within 2^-24
    relative, and the products and the quotient add three more: 53 * 2^-24 bounds the relative error.  (With these dyadic weights
    every partial sum is in fact exact.)"""
    h, w = 9, 9
    hdr = np.full((h, w, 3), 0.75, dtype=F)
    out, var = VM.denoise_variance(orc, hdr, np.ones((h, w), dtype=F), np.full((h, w), 8.0, dtype=F), iterations=1, short_history=4.0)
    want = (70.0 / 256.0) ** 2
    inner = var[2:-2, 2:-2].astype(np.float64)
    err = float(np.abs(inner - want).max() / want)
    print(f"interior variance_out {float(var[4, 4])!r}, closed form {want!r}, relative error {err:.3g} (bound {53 * 2.0 ** -24:.3g})")
    assert err <= 53 * 2.0 ** -24
    assert np.array_equal(_bits(out), _bits(hdr))
    assert (var[0, 0] > var[4, 4]) and np.isfinite(var).all()           # a corner has 9 taps: less averaging


def test_special_values(orc):
    h, w = 8, 10
    rng = np.random.default_rng(21)
    hdr = (rng.random((h, w, 3)) * 2.0).astype(F)
    var = (rng.random((h, w)) * 0.1).astype(F)
    length = np.full((h, w), 9.0, dtype=F)
    base = VM.denoise_variance(orc, hdr, var, length)
    # a NaN (or negative) variance counts as 0
    v0, vn, vm = var.copy(), var.copy(), var.copy()
    v0[3, 4], vn[3, 4], vm[3, 4] = 0.0, np.nan, -2.0
    want = VM.denoise_variance(orc, hdr, v0, length)
    for got in (VM.denoise_variance(orc, hdr, vn, length), VM.denoise_variance(orc, hdr, vm, length)):
        assert VM.same_bits(got[0], want[0]) and VM.same_bits(got[1], want[1])
    assert np.isfinite(want[0]).all() and not VM.same_bits(want[0], base[0])
    # a NaN length takes the spatial estimate, with lc = 1
    l1, ln = length.copy(), length.copy()
    l1[2, 7], ln[2, 7] = 1.0, np.nan
    want, got = VM.denoise_variance(orc, hdr, var, l1), VM.denoise_variance(orc, hdr, var, ln)
    assert VM.same_bits(got[0], want[0]) and VM.same_bits(got[1], want[1]) and np.isfinite(got[0]).all()
    assert not VM.same_bits(got[0], base[0])
    # ... unless short_history is 0: then no pixel does
    want, got = VM.denoise_variance(orc, hdr, var, length, short_history=0.0), VM.denoise_variance(orc, hdr, var, ln, short_history=0.0)
    assert VM.same_bits(got[0], want[0]) and VM.same_bits(got[1], want[1])


@pytest.mark.parametrize("guide", ["normal", "depth"])
def test_an_edge_stops_the_estimate_and_the_filter(orc, guide):
    """two flat halves, 1.0 and 2.0, as a single frame without history (every pixel takes the spatial estimate): across the edge
    e clamps to 128 and the weight is 0, so each half sees only itself, its estimate is 0 and it comes back bit for bit"""
    h, w = 9, 12
    hdr = np.empty((h, w, 3), dtype=F)
    hdr[:, : w // 2], hdr[:, w // 2:] = 1.0, 2.0
    if guide == "normal":                                               # |dn|^2 = 2, kn = 400
        n = np.zeros((h, w, 3), dtype=F)
        n[:, : w // 2] = (0, 0, 1)
        n[:, w // 2:] = (1, 0, 0)
        kw = dict(normal=n, sigma_normal=0.05)
    else:                                                               # a hit at depth 1 beside a miss
        z = np.empty((h, w), dtype=F)
        z[:, : w // 2], z[:, w // 2:] = 1.0, 1e30
        kw = dict(depth=z)
    out, var = VM.denoise_variance(orc, hdr, iterations=5, **kw)
    assert np.array_equal(_bits(out), _bits(hdr))
    # the estimate's own roundings: l(1,1,1) is not exactly 1, so s2/ws and mu*mu differ by the roundings of their 25-term sums (25
    # for s2, twice 25 for mu*mu, a few for the products and quotients: 80 * 2^-24 relative to l^2 <= 4), times short_history / 1 = 4
    assert float(var.max()) <= 80 * 2.0 ** -24 * 4.0 * 4.0
    # without the guide the estimate sees the step and the halves mix
    plain, pvar = VM.denoise_variance(orc, hdr, iterations=5)
    assert not np.array_equal(_bits(plain), _bits(hdr)) and float(pvar.max()) > float(var.max())


# ---- quality on the atrium sequences -----------------------------------------------------------------------------------------------
_seq = {}


def _sequences(rrt, orc):
    """the 20 k-triangle atrium at 64x36, depth 8, 1 spp, per-sample seeds with sample_begin = 1 + f, temporal defaults: (a) the
    8-frame moving sequence of test_temporal_model.test_accumulation_beats_denoising_alone with its 1024-sample target, (b) 16
    frames of a static camera with a 4096-sample target from 100000, (c) the last noisy frame of (a) alone.  Computed once."""
    if _seq:
        return _seq
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth
    tris, mats, texs, pose = synth.make_scene("atrium", n_target=20000, tex_size=64)
    sc = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    t, nodes = orc.bvh_build(sc.tris)
    sc.tris, sc.bvh_nodes = t, nodes.view(L.NODE).reshape(-1)
    w, h = 64, 36

    def camera(dp=(0.0, 0.0, 0.0), dyaw=0.0):
        c = rrt.Camera(position=tuple(float(pose[0][i]) + dp[i] for i in range(3)), pitch=pose[1], yaw=pose[2] + dyaw)
        c.update_view()
        return c.uniform

    def run(frames, moving):
        hist = None
        for f in range(frames):
            cam = camera((0.02 * f, 0.0, 0.01 * f), 0.4 * f) if moving else camera()
            args = (sc.tris, sc.bvh_nodes, sc.materials_array(), sc.textures, cam, w, h)
            noisy = orc.render(*args, 1, 8, seed_mode=1, sample_begin=1 + f, want_rgba8=False)[0]
            g = FM.frame(orc, sc, cam, w, h, 1)[0]
            r = T.step(noisy, g["position"], g["normal"], g["depth"], g["material"], [cam], hist, g["albedo"], **T.DEFAULTS)
            hist = r["history"]
        return args, noisy, dict(normal=g["normal"], depth=g["depth"], albedo=g["albedo"]), r

    args, noisy, g, r = run(8, True)
    target = orc.render(*args, 1024, 8, seed_mode=1, sample_begin=1000, want_rgba8=False)[0]
    _seq["a"] = dict(hdr=r["out"], variance=r["variance"], length=r["length"], guides=g, target=target)
    _seq["c"] = dict(hdr=noisy, variance=None, length=None, guides=g, target=target)
    args, noisy, g, r = run(16, False)
    target = orc.render(*args, 4096, 8, seed_mode=1, sample_begin=100000, want_rgba8=False)[0]
    _seq["b"] = dict(hdr=r["out"], variance=r["variance"], length=r["length"], guides=g, target=target)
    return _seq


SWEEP = (2.0, 4.0, 8.0, 16.0)
DEFAULT_SIGMA = 16.0
# (b): the exact model gives guided / fixed = 0.01750 / 0.02384 = 0.734; a fifth more is 0.881, rounded up to one decimal
STATIC_RATIO = 0.9


def test_quality_against_the_fixed_filter_and_the_sigma_sweep(rrt, orc):
    """The exact model, RMSE against the converged frame, fixed filter (denoise_model defaults) | guided at sigma_luminance 2, 4, 8, 16:
      (a) 8 moving frames accumulated   0.0420 | 0.0456  0.0418  0.0401  0.0394
      (b) 16 static frames accumulated  0.0238 | 0.0222  0.0191  0.0178  0.0175
      (c) one noisy frame, no history   0.0602 | 0.0711  0.0609  0.0573  0.0558
    16 wins on all three, which makes it the default of Renderer.denoise_variance."""
    from rust_ray_tracing_amd import host
    import inspect
    assert inspect.signature(host.Renderer.denoise_variance).parameters["sigma_luminance"].default == DEFAULT_SIGMA == VM.DEFAULTS["sigma_luminance"]
    seq = _sequences(rrt, orc)
    fixed, guided = {}, {}
    for k in "abc":
        s = seq[k]
        fixed[k] = D.rmse(D.denoise(orc, s["hdr"], **s["guides"]), s["target"])
        for sigma in SWEEP:
            out, var = VM.denoise_variance(orc, s["hdr"], s["variance"], s["length"], sigma_luminance=sigma, **s["guides"])
            assert np.isfinite(out).all() and np.isfinite(var).all()
            guided[k, sigma] = D.rmse(out, s["target"])
        print(f"({k}) input {D.rmse(s['hdr'], s['target']):.4f}, fixed {fixed[k]:.4f}, guided at sigma_luminance "
              + ", ".join(f"{sigma:g}: {guided[k, sigma]:.4f}" for sigma in SWEEP))
    for k in "abc":
        print(f"({k}) rmse fixed {fixed[k]:.4f}, guided (sigma_luminance {DEFAULT_SIGMA:g}) {guided[k, DEFAULT_SIGMA]:.4f}, "
              f"ratio {guided[k, DEFAULT_SIGMA] / fixed[k]:.3f}")
    # the default is the value that wins or ties on all three
    for k in "abc":
        assert guided[k, DEFAULT_SIGMA] == min(guided[k, sigma] for sigma in SWEEP), (k, guided)
    assert guided["a", DEFAULT_SIGMA] <= fixed["a"]
    assert guided["c", DEFAULT_SIGMA] <= fixed["c"]
    assert guided["b", DEFAULT_SIGMA] <= STATIC_RATIO * fixed["b"]


# ---- the argument checks: before any device work, each message names its field -----------------------------------------------------
W, H, V = 6, 4, 2
N = W * H * V
WORDS = dict(hdr=3, normal=3, depth=1, albedo=3, variance=1, length=1, out=3, variance_out=1)


def _opt(L, **kw):
    o = L.MiptVarianceOptions()
    o.width, o.height, o.n_views, o.iterations = W, H, V, 5
    o.sigma_luminance, o.sigma_normal, o.sigma_depth, o.short_history = 16.0, 0.5, 0.5, 4.0
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


class _Planes:
    """host planes for one call; a 16-byte aligned workspace"""

    def __init__(self):
        self.a = {k: np.zeros(N * n + 4 + 3 * N, dtype=np.float32) for k, n in WORDS.items()}   # + 3 N words: a case that moves a pointer to a plane's end stays inside that plane's own allocation, whatever lies behind it on the heap
        raw = np.zeros(N * 12 + 8, dtype=np.float32)
        off = (-raw.ctypes.data % 16) // 4
        self.ws = raw[off: off + N * 12]
        assert self.ws.ctypes.data % 16 == 0

    def bufs(self, L, **kw):
        b = L.MiptVarianceBuffers()
        for k, a in self.a.items():
            setattr(b, k, a.ctypes.data)
        for k, v in kw.items():
            if k == "reserved":
                b.reserved[v] = self.a["hdr"].ctypes.data
            else:
                setattr(b, k, v)
        return b


def _calls(lib, p):
    """both entries with the same (opt, bufs) -> status"""
    return (("mipt_denoise_variance", lambda o, b: lib.mipt_denoise_variance(o, b, 0)),
            ("mipt_denoise_variance_device", lambda o, b: lib.mipt_denoise_variance_device(o, b, p.ws.ctypes.data, p.ws.nbytes, None)))


def test_struct_sizes_and_workspace_bytes(rrt):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    assert C.sizeof(L.MiptVarianceOptions) == 64 and C.sizeof(L.MiptVarianceBuffers) == 128
    assert L.MiptVarianceOptions.short_history.offset == 28 and L.MiptVarianceOptions.flags.offset == 32
    assert L.MiptVarianceBuffers.variance_out.offset == 56
    assert lib.mipt_denoise_variance_workspace_bytes(1920, 1080, 1) == 1920 * 1080 * 48
    assert lib.mipt_denoise_variance_workspace_bytes(W, H, V) == N * 48
    assert lib.mipt_denoise_variance_workspace_bytes(65535, 65535, 1) == 65535 * 65535 * 48
    assert lib.mipt_denoise_variance_workspace_bytes(3, 2, 700) == 4200 * 48
    for bad in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (65536, 65536, 1), (1 << 15, 1 << 15, 4), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)):
        assert lib.mipt_denoise_variance_workspace_bytes(*bad) == 0, bad
    assert lib.mipt_abi_version() == 4


def test_argument_checks_of_both_entries(rrt):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    p = _Planes()
    inf, nan = float("inf"), float("nan")
    option_cases = [
        (dict(width=0), "width"), (dict(height=0), "height"), (dict(n_views=0), "n_views"),
        (dict(width=1 << 15, height=1 << 15, n_views=4), "below 2^32"), (dict(width=1 << 16, height=1 << 16, n_views=1), "below 2^32"),
        (dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"),
        (dict(sigma_luminance=0.0), "sigma_luminance"), (dict(sigma_luminance=-1.0), "sigma_luminance"),
        (dict(sigma_luminance=inf), "sigma_luminance"), (dict(sigma_luminance=nan), "sigma_luminance"),
        (dict(short_history=-1.0), "short_history"), (dict(short_history=inf), "short_history"), (dict(short_history=nan), "short_history"),
        (dict(sigma_normal=0.0), "sigma_normal"), (dict(sigma_normal=nan), "sigma_normal"), (dict(sigma_normal=1e25), "sigma_normal"),
        (dict(sigma_depth=-0.5), "sigma_depth"), (dict(sigma_depth=inf), "sigma_depth"), (dict(sigma_depth=1e-25), "sigma_depth"),
        (dict(flags=1), "flags"), (dict(reserved=0), "reserved"), (dict(reserved=6), "reserved"),
    ]
    hdr = p.a["hdr"].ctypes.data
    at = lambda k, off=0: p.a[k].ctypes.data + off  # noqa: E731
    buffer_cases = [
        (dict(hdr=None), "null hdr"), (dict(out=None), "null out"), (dict(variance=None), "null variance"), (dict(length=None), "null length"),
        (dict(reserved=0), "reserved buffer pointers"), (dict(reserved=7), "reserved buffer pointers"),
        (dict(normal=hdr), "normal overlaps hdr"), (dict(albedo=hdr + 12 * N - 4), "albedo overlaps hdr"), (dict(out=hdr + 4), "out overlaps hdr"),
        (dict(out=at("albedo")), "out overlaps albedo"), (dict(depth=at("normal", 4 * N)), "depth overlaps normal"),
        (dict(variance=at("depth")), "variance overlaps depth"), (dict(length=at("variance", 4 * N - 4)), "length overlaps variance"),
        (dict(out=at("variance")), "out overlaps variance"), (dict(out=at("length")), "out overlaps length"),
        (dict(variance_out=hdr), "variance_out overlaps hdr"), (dict(variance_out=at("variance")), "variance_out overlaps variance"),
        (dict(variance_out=at("length", 4 * N - 4)), "variance_out overlaps length"), (dict(variance_out=at("out", 12 * N - 4)), "variance_out overlaps out"),
        (dict(variance_out=at("normal", 8)), "variance_out overlaps normal"),
    ]
    for name, call in _calls(lib, p):
        for kw, msg in option_cases:
            assert call(C.byref(_opt(L, **kw)), C.byref(p.bufs(L))) == L.ERR_INVALID_ARG, (name, kw)
            err = lib.mipt_last_error().decode()
            assert msg in err and err.startswith(name + ":"), (name, kw, err)
        for kw, msg in buffer_cases:
            assert call(C.byref(_opt(L)), C.byref(p.bufs(L, **kw))) == L.ERR_INVALID_ARG, (name, kw)
            err = lib.mipt_last_error().decode()
            assert msg in err and err.startswith(name + ":"), (name, kw, err)
        assert call(None, C.byref(p.bufs(L))) == L.ERR_INVALID_ARG and "opt" in lib.mipt_last_error().decode()
        assert call(C.byref(_opt(L)), None) == L.ERR_INVALID_ARG and "buffers" in lib.mipt_last_error().decode()
    # what may be absent, a sigma given for an absent guide, short_history 0 and out == hdr get past the checks: to the device (the
    # host entry) or the device-memory check (the device entry)
    for okw, bkw in ((dict(sigma_normal=nan), dict(normal=None)), (dict(sigma_depth=0.0), dict(depth=None)), ({}, dict(variance=None, length=None)),
                     ({}, dict(variance_out=None)), ({}, dict(albedo=None)), (dict(short_history=0.0), {}), ({}, dict(out=hdr))):
        rc = lib.mipt_denoise_variance(C.byref(_opt(L, **okw)), C.byref(p.bufs(L, **bkw)), 0)
        assert rc in (L.OK, L.ERR_HIP), (okw, bkw, rc, lib.mipt_last_error())
        assert lib.mipt_denoise_variance_device(C.byref(_opt(L, **okw)), C.byref(p.bufs(L, **bkw)), p.ws.ctypes.data, p.ws.nbytes, None) == L.ERR_INVALID_ARG
        assert "hdr is not device memory" in lib.mipt_last_error().decode()
    for a in p.a.values():
        assert not a.any()                                              # no refused call wrote anything (zeros filter to zeros)


def test_device_entry_checks_workspace_alignment_and_memory(rrt):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    p = _Planes()
    f = lib.mipt_denoise_variance_device
    o, b = _opt(L), p.bufs(L)
    ws, need = p.ws.ctypes.data, N * 48
    for args, msg in [((None, need), "null workspace"), ((ws, need - 1), "too small"), ((ws, 0), "too small"), ((ws + 4, need + 16), "workspace must be 16-byte aligned")]:
        assert f(C.byref(o), C.byref(b), *args, None) == L.ERR_INVALID_ARG, msg
        assert msg in lib.mipt_last_error().decode(), (msg, lib.mipt_last_error())
    for name in WORDS:
        bad = p.bufs(L, **{name: p.a[name].ctypes.data + 2})
        assert f(C.byref(o), C.byref(bad), ws, need, None) == L.ERR_INVALID_ARG
        assert f"{name} must be 4-byte aligned" in lib.mipt_last_error().decode(), (name, lib.mipt_last_error())
        inside = p.bufs(L, **{name: ws + 16 * N})
        assert f(C.byref(o), C.byref(inside), ws, need, None) == L.ERR_INVALID_ARG
        assert f"{name} overlaps the workspace" in lib.mipt_last_error().decode(), (name, lib.mipt_last_error())
    # host memory is not device memory: refused by name, with or without a device
    assert f(C.byref(o), C.byref(b), ws, need, None) == L.ERR_INVALID_ARG
    assert "hdr is not device memory" in lib.mipt_last_error().decode()


def test_host_entry_fails_loudly_without_a_device(rrt):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path is exercised on the CPU-only box")
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    p = _Planes()
    assert lib.mipt_denoise_variance(C.byref(_opt(L)), C.byref(p.bufs(L)), 0) == L.ERR_HIP
    assert "hipSetDevice" in lib.mipt_last_error().decode()
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=1, output_image_dimensions=(W, H), output_image_path="x.png"))
    with pytest.raises(rrt.MiptError) as e:
        r.denoise_variance(np.zeros((H, W, 3), dtype=np.float32))
    assert e.value.code == L.ERR_HIP


def test_renderer_denoise_variance_checks_its_arguments(rrt):
    from rust_ray_tracing_amd import _lib as L
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=1, output_image_dimensions=(W, H), output_image_path="x.png"))
    hdr = np.zeros((V, H, W, 3), dtype=np.float32)
    z = np.zeros((V, H, W), dtype=np.float32)
    for kw, msg in [(dict(hdr=np.zeros((H, W), dtype=np.float32)), "hdr"), (dict(hdr=np.zeros((H, W, 4), dtype=np.float32)), "hdr"),
                    (dict(hdr=hdr.astype(np.float64)), "hdr"), (dict(normal=z), "normal"), (dict(normal=hdr[0]), "normal"),
                    (dict(depth=hdr), "depth"), (dict(depth=z.astype(np.float64)), "depth"), (dict(albedo=hdr[:, :, :, :2]), "albedo"),
                    (dict(variance=hdr, length=z), "variance"), (dict(variance=z.astype(np.float64), length=z), "variance"),
                    (dict(variance=z, length=z[0]), "length"), (dict(variance=z, length=z.astype(np.int32)), "length")]:
        args = dict(dict(hdr=hdr), **kw)
        with pytest.raises(ValueError) as e:
            r.denoise_variance(**args)
        assert str(e.value).startswith(msg + ":"), (kw, str(e.value))
    import torch
    with pytest.raises(ValueError) as e:
        r.denoise_variance(hdr, variance=torch.zeros((V, H, W)), length=z)
    assert str(e.value).startswith("variance:")
    with pytest.raises(ValueError) as e:
        r.denoise_variance(torch.zeros((V, H, W, 3)))                   # a host tensor
    assert str(e.value).startswith("hdr:")
    # what the library checks comes back as its status and message
    for kw, msg in [(dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(sigma_luminance=0.0), "sigma_luminance"),
                    (dict(short_history=-1.0), "short_history"), (dict(variance=z), "null length"), (dict(length=z), "null variance"),
                    (dict(normal=hdr.copy(), sigma_normal=float("nan")), "sigma_normal"), (dict(depth=z, sigma_depth=-1.0), "sigma_depth")]:
        with pytest.raises(rrt.MiptError) as e:
            r.denoise_variance(hdr, **kw)
        assert e.value.code == L.ERR_INVALID_ARG and msg in str(e.value), (kw, str(e.value))
    # render_sequence takes True, False or "variance" and nothing else by name
    from rust_ray_tracing_amd import _lib as LL
    rs = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=1, output_image_dimensions=(W, H), output_image_path="x.png",
                                              seed_mode=LL.SEED_PER_SAMPLE))
    with pytest.raises(ValueError) as e:
        next(rs.render_sequence(None, [[None]], denoise="svgf"))
    assert "variance" in str(e.value)
    with pytest.raises(ValueError) as e:
        next(rs.render_sequence(None, [[None]], denoise="variance", sigma_color=4.0))
    assert "sigma_color" in str(e.value)
