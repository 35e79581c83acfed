"""CPU: the model of the guided upsampling (tests/tools/upsample_model.py) has the properties the contract of include/mipt.h
promises -- a constant frame stays constant, without guides it is plain bilinear, coinciding pixels come back bit for bit, material,
depth and normal edges keep each side's value where plain bilinear mixes them, albedo detail finer than the low frame comes back,
a pixel without an accepted tap falls back to plain bilinear with weight 0, special values take the side the header names, and on
the atrium a low frame upsampled with guides beats plain bilinear and a full frame of the same path budget -- and every argument
check of mipt_upsample / mipt_upsample_device / Renderer.upsample runs before any device work."""
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
import upsample_model as UM  # noqa: E402

F = np.float32
GUIDES = ("normal", "depth", "albedo", "material")
COMBOS = list(itertools.product((False, True), repeat=4))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _random_guides(rng, v, h, w, which, materials=3):
    g = {}
    if which[0]:
        g["normal"] = rng.standard_normal((v, h, w, 3)).astype(F)
    if which[1]:
        g["depth"] = (rng.random((v, h, w)) * 3.0).astype(F)
    if which[2]:
        g["albedo"] = rng.random((v, h, w, 3)).astype(F)
    if which[3]:
        g["material"] = rng.integers(0, materials, (v, h, w)).astype(np.uint32)
    return g


# ---- the model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", COMBOS, ids=lambda g: "n%dz%da%dm%d" % g)
def test_a_constant_frame_stays_constant(orc, which):
    """colour 1.0, no demodulation (an albedo guide would scale it: it is left out of both dicts): w*1 = w, so sum_ch and wsum add
    the same numbers in the same order and their quotient is exactly 1 -- and so are sb_ch and bsum where no tap was accepted"""
    rng = np.random.default_rng(5)
    v, h, w, k = 2, 4, 5, 3
    which = (which[0], which[1], False, which[3])
    lo, hi = _random_guides(rng, v, h, w, which), _random_guides(rng, v, h * k, w * k, which)
    out, weight, _ = UM.upsample(orc, np.ones((v, h, w, 3), dtype=F), k, lo, hi)
    assert np.array_equal(_bits(out), _bits(np.ones((v, h * k, w * k, 3), dtype=F)))
    if which[3]:
        assert (weight == 0).any() and (weight > 0).any()               # the fallback was on the way


@pytest.mark.parametrize("k", [2, 4, 8])
def test_without_guides_it_is_plain_bilinear(orc, k):
    """lo_hdr only, k a power of two: wx = rx/k and the products with the small integers of a ramp c = x are exact, so X/k comes
    back exactly; the last k-1 columns have no right neighbour and hold the last low value"""
    h, w = 3, 6
    lo = np.broadcast_to(np.arange(w, dtype=F)[None, :, None], (h, w, 3)).copy()
    out, weight, bil = UM.upsample(orc, lo, k)
    want = np.minimum(np.arange(w * k, dtype=np.float64) / k, w - 1).astype(F)
    assert np.array_equal(_bits(out), _bits(np.broadcast_to(want[None, :, None], (h * k, w * k, 3))))
    assert np.array_equal(_bits(out[:, -(k - 1):]), _bits(np.full((h * k, k - 1, 3), w - 1, dtype=F)))
    assert np.array_equal(_bits(out), _bits(bil))
    inner = weight[: -(k - 1), : -(k - 1)]                              # where all the taps with b > 0 exist, the weights sum to 1
    assert np.array_equal(_bits(inner), _bits(np.ones_like(inner)))


@pytest.mark.parametrize("k", [2, 3, 5])
def test_coinciding_pixels_come_back_bit_for_bit(orc, k):
    """X and Y multiples of k: one tap with b = 1; equal guides make e = 0 and expf(-0) = 1, so (1*c)/1 = c"""
    rng = np.random.default_rng(9)
    v, h, w = 2, 5, 7
    lo_hdr = (rng.random((v, h, w, 3)) * 4.0).astype(F)
    which = (True, True, False, True)
    hi = _random_guides(rng, v, h * k, w * k, which)
    lo = {n: np.ascontiguousarray(a[:, ::k, ::k]) for n, a in hi.items()}
    out, weight, _ = UM.upsample(orc, lo_hdr, k, lo, hi)
    assert np.array_equal(_bits(out[:, ::k, ::k]), _bits(lo_hdr))
    assert np.array_equal(_bits(weight[:, ::k, ::k]), _bits(np.ones((v, h, w), dtype=F)))


def _edge_case(guide, k=2, h=3, w=6, edge=5):
    """two low pixels columns 2 | 3 of colours 0 and 1 differ in `guide`; at full resolution the edge lies before column `edge`, an
    odd X between the two low pixels' own columns 2k and 3k"""
    lo_hdr = np.zeros((h, w, 3), dtype=F)
    lo_hdr[:, 3:] = 1.0
    H, W = h * k, w * k
    assert 2 * k < edge < 3 * k and edge % 2 == 1
    side_lo, side_hi = np.arange(w) >= 3, np.arange(W) >= edge

    def plane(side, n):
        if guide == "material":
            return np.broadcast_to(np.where(side, 7, 4).astype(np.uint32)[None, :], (n, len(side))).copy()
        if guide == "depth":
            return np.broadcast_to(np.where(side, 1e30, 1.0).astype(F)[None, :], (n, len(side))).copy()
        nrm = np.where(side[:, None], np.array([1, 0, 0], dtype=F), np.array([0, 0, 1], dtype=F))
        return np.broadcast_to(nrm[None], (n, len(side), 3)).copy()

    return lo_hdr, {guide: plane(side_lo, h)}, {guide: plane(side_hi, H)}, side_hi


@pytest.mark.parametrize("guide", ["material", "depth", "normal"])
def test_an_edge_keeps_each_side(orc, guide):
    """every full pixel takes exactly its own side's value (the other side's taps are rejected, or weigh expf(-128) = 0: a depth
    step 1 -> 1e30, |dn|^2 = 2 at sigma_normal 0.05 is e = 800); plain bilinear gives 0.5 at X = 5"""
    lo_hdr, lo, hi, side = _edge_case(guide)
    out, weight, bil = UM.upsample(orc, lo_hdr, 2, lo, hi, sigma_normal=0.05)
    want = np.broadcast_to(side.astype(F)[None, :, None], out.shape)
    assert np.array_equal(_bits(out), _bits(want)), out[0, :, 0]
    assert (weight > 0).all()
    assert bil[0, 5, 0] == F(0.5) and UM.upsample(orc, lo_hdr, 2)[0][0, 5, 0] == F(0.5)


def test_albedo_detail_finer_than_the_low_frame_comes_back(orc):
    """lo_hdr = lo_albedo * E and a one-pixel checker as the full-resolution albedo: every c_q = (a*E)/a is E within 1/2 ulp, a
    weighted mean of such values stays within their spread plus the mean's own roundings, and out = c * a_P adds one more: the
    bound asked for is 2 ulp of a_P * E"""
    rng = np.random.default_rng(13)
    h, w, k = 5, 6, 2
    E = F(1.75)
    lo_alb = (0.2 + 0.6 * rng.random((h, w, 3))).astype(F)
    lo_hdr = (lo_alb * E).astype(F)
    yy, xx = np.mgrid[0:h * k, 0:w * k]
    alb = np.where(((yy + xx) & 1)[..., None] == 1, F(0.9), F(0.1)).astype(F) * np.ones(3, dtype=F)
    out, _, _ = UM.upsample(orc, lo_hdr, k, dict(albedo=lo_alb), dict(albedo=alb))
    want = (alb.astype(np.float64) * float(E))
    ulp = np.spacing(want.astype(F)).astype(np.float64)
    err = np.abs(out.astype(np.float64) - want) / ulp
    print(f"albedo checker: at most {err.max():.2f} ulp from a_P * E")
    assert err.max() <= 2.0
    assert abs(float(out[0, 0, 0]) - float(out[0, 1, 0])) > 1.0          # the checker is there: 0.1*E beside 0.9*E


def test_a_pixel_without_an_accepted_tap_falls_back_to_plain_bilinear(orc):
    rng = np.random.default_rng(17)
    h, w, k = 4, 5, 2
    lo_hdr = rng.random((h, w, 3)).astype(F)
    lo_m = np.zeros((h, w), dtype=np.uint32)
    m = np.zeros((h * k, w * k), dtype=np.uint32)
    m[3, 5] = 9                                                         # four taps, none shares its material
    m[4, 4] = 9                                                         # one tap
    out, weight, bil = UM.upsample(orc, lo_hdr, k, dict(material=lo_m), dict(material=m))
    plain = UM.upsample(orc, lo_hdr, k)[0]
    assert weight[3, 5] == 0 and weight[4, 4] == 0 and np.count_nonzero(weight == 0) == 2
    assert np.array_equal(_bits(out), _bits(plain)) and np.array_equal(_bits(bil), _bits(plain))
    assert np.array_equal(_bits(out[4, 4]), _bits(lo_hdr[2, 2]))


def test_special_values(orc):
    rng = np.random.default_rng(21)
    h, w, k = 4, 5, 2
    lo_hdr = (rng.random((h, w, 3)) * 2.0).astype(F)
    lo = _random_guides(rng, 1, h, w, (True, True, True, False))
    hi = _random_guides(rng, 1, h * k, w * k, (True, True, True, False))
    lo, hi = {n: a[0] for n, a in lo.items()}, {n: a[0] for n, a in hi.items()}
    # a NaN (zero, negative) albedo equals the floor, at either resolution
    for res, at in (("lo", (2, 3, 1)), ("hi", (5, 4, 0))):
        variants = []
        for value in (1.0 / 256.0, np.nan, 0.0, -3.0):
            l2, h2 = {n: a.copy() for n, a in lo.items()}, {n: a.copy() for n, a in hi.items()}
            (l2 if res == "lo" else h2)["albedo"][at] = value
            variants.append(UM.upsample(orc, lo_hdr, k, l2, h2))
        for got in variants[1:]:
            assert UM.same_bits(got[0], variants[0][0]) and UM.same_bits(got[1], variants[0][1]), res
        assert np.isfinite(variants[0][0]).all()
    # a NaN normal gives its tap e = 128 and weight b * expf(-128) = 0: the tap adds +0 to every guided sum, which changes nothing,
    # so the frame equals the one where that tap's material is another
    l2 = {n: a.copy() for n, a in lo.items()}
    l2["normal"][1, 2, 1] = np.nan
    got = UM.upsample(orc, lo_hdr, k, l2, hi)
    lm, hm = dict(lo, material=np.zeros((h, w), dtype=np.uint32)), dict(hi, material=np.zeros((h * k, w * k), dtype=np.uint32))
    lm["material"][1, 2] = 5
    want = UM.upsample(orc, lo_hdr, k, lm, hm)
    assert UM.same_bits(got[0], want[0]) and UM.same_bits(got[1], want[1]) and np.isfinite(got[0]).all()
    assert got[1][2, 4] == 0                                            # the coinciding pixel has that tap alone: the fallback
    # a NaN normal at a full pixel rejects every tap of that pixel alone
    h2 = {n: a.copy() for n, a in hi.items()}
    h2["normal"][3, 3, 0] = np.nan
    got = UM.upsample(orc, lo_hdr, k, lo, h2)
    base = UM.upsample(orc, lo_hdr, k, lo, hi)
    assert got[1][3, 3] == 0 and np.count_nonzero(_bits(got[1]) != _bits(base[1])) == 1 and np.isfinite(got[0]).all()
    # NaN and inf radiance stay where the taps reach
    l3 = lo_hdr.copy()
    l3[0, 0, 0], l3[3, 4, 1] = np.nan, np.inf
    got = UM.upsample(orc, l3, k, lo, hi)
    assert np.isnan(got[0][0, 0, 0]) and np.isinf(got[0][6, 8, 1]) and np.isfinite(got[0][..., 2]).all()


# ---- quality on the atrium -----------------------------------------------------------------------------------------------------------
# the exact model gives guided / bilinear = 0.0453 / 0.0697 = 0.650; a fifth more is 0.780, rounded up to one decimal
BILINEAR_RATIO = 0.8


def test_quality_against_the_full_frame_and_plain_bilinear(rrt, orc):
    """The 20 k-triangle atrium of tests/test_denoise_model.py, its camera, depth 8 and 1024-sample target from seed 1000 at 64x36.
    The low frame is 32x18 at 4 spp -- the paths of 64x36 at 1 spp -- filtered by denoise_model.denoise at its defaults.  The exact
    model, RMSE against the target:
      full frame, 1 spp, unfiltered                         0.1910
      full frame, 1 spp, denoise_model.denoise              0.0547
      low frame, 4 spp, denoised, upsampled with guides     0.0453
      the same low frame, plain bilinear                    0.0697
    89 of the 2304 pixels (3.9 %) found no accepted tap and took the fallback."""
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth
    tris, mats, texs, cam = synth.make_scene("atrium", n_target=20000, tex_size=64)
    sc = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    t, nodes = orc.bvh_build(sc.tris)
    sc.tris, sc.bvh_nodes = t, nodes.view(L.NODE).reshape(-1)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    w, h, k = 64, 36, 2
    scene = (sc.tris, sc.bvh_nodes, sc.materials_array(), sc.textures, sc.camera.uniform)
    target = orc.render(*scene, w, h, 1024, 8, seed_mode=1, sample_begin=1000, want_rgba8=False)[0]
    hi = FM.frame(orc, sc, sc.camera.uniform, w, h, 0)[0]
    lo = FM.frame(orc, sc, sc.camera.uniform, w // k, h // k, 0)[0]
    full_noisy = orc.render(*scene, w, h, 1, 8, want_rgba8=False)[0]    # pixel-stream seeds, as test_it_denoises
    lo_noisy = orc.render(*scene, w // k, h // k, 4, 8, want_rgba8=False)[0]
    full = D.denoise(orc, full_noisy, hi["normal"], hi["depth"], hi["albedo"])
    lo_den = D.denoise(orc, lo_noisy, lo["normal"], lo["depth"], lo["albedo"])
    out, weight, _ = UM.upsample(orc, lo_den, k, lo, hi)
    plain = UM.upsample(orc, lo_den, k)[0]
    assert np.isfinite(out).all()
    r = dict(noisy=D.rmse(full_noisy, target), full=D.rmse(full, target), guided=D.rmse(out, target), bilinear=D.rmse(plain, target))
    fallback = int(np.count_nonzero(weight == 0))
    print(f"rmse full 1 spp {r['noisy']:.4f}, full 1 spp denoised {r['full']:.4f}, low 4 spp denoised + guided {r['guided']:.4f}, "
          f"+ plain bilinear {r['bilinear']:.4f}; guided / bilinear {r['guided'] / r['bilinear']:.3f}; "
          f"fallback {fallback} of {weight.size} pixels ({100.0 * fallback / weight.size:.1f} %)")
    assert r["guided"] <= r["full"]                                     # gate 1: the same number of paths
    assert r["guided"] <= r["bilinear"]                                 # gate 2
    assert r["guided"] <= BILINEAR_RATIO * r["bilinear"]                # gate 3
    assert fallback * 10 < weight.size


# ---- the argument checks: before any device work, each message names its field -----------------------------------------------------
W, H, V, K = 6, 4, 2, 2
N = W * H * V
NLO = N // (K * K)
WORDS = dict(lo_hdr=3, lo_normal=3, lo_depth=1, lo_albedo=3, lo_material=1, normal=3, depth=1, albedo=3, material=1, out=3, weight=1)


def _count(name):
    return NLO if name.startswith("lo_") else N


def _opt(L, **kw):
    o = L.MiptUpsampleOptions()
    o.width, o.height, o.n_views, o.scale = W, H, V, K
    o.sigma_normal, o.sigma_depth = 0.5, 0.5
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


class _Planes:
    """host planes for one call; a 16-byte aligned workspace"""

    def __init__(self):
        self.a = {k: np.zeros(_count(k) * n + 4 + 3 * N, dtype=np.float32) for k, n in WORDS.items()}   # + 3 N words: a case that moves a pointer to a plane's end stays inside that plane's own allocation, whatever lies behind it on the heap
        raw = np.zeros(NLO * 8 + 8, dtype=np.float32)
        off = (-raw.ctypes.data % 16) // 4
        self.ws = raw[off: off + NLO * 8]
        assert self.ws.ctypes.data % 16 == 0

    def bufs(self, L, **kw):
        b = L.MiptUpsampleBuffers()
        for k, a in self.a.items():
            setattr(b, k, a.ctypes.data)
        for k, v in kw.items():
            if k == "reserved":
                b.reserved[v] = self.a["lo_hdr"].ctypes.data
            else:
                setattr(b, k, v)
        return b


def _calls(lib, p):
    """both entries with the same (opt, bufs) -> status"""
    return (("mipt_upsample", lambda o, b: lib.mipt_upsample(o, b, 0)),
            ("mipt_upsample_device", lambda o, b: lib.mipt_upsample_device(o, b, p.ws.ctypes.data, p.ws.nbytes, None)))


def test_struct_sizes_offsets_and_workspace_bytes(rrt):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    assert C.sizeof(L.MiptUpsampleOptions) == 64 and C.sizeof(L.MiptUpsampleBuffers) == 128
    o = L.MiptUpsampleOptions
    assert [getattr(o, f).offset for f in ("width", "height", "n_views", "scale", "sigma_normal", "sigma_depth", "flags", "reserved")] == [0, 4, 8, 12, 16, 20, 24, 28]
    b = L.MiptUpsampleBuffers
    assert [getattr(b, f).offset for f in list(WORDS) + ["reserved"]] == [8 * i for i in range(12)]
    assert lib.mipt_upsample_workspace_bytes(1920, 1080, 1, 2) == 960 * 540 * 32
    assert lib.mipt_upsample_workspace_bytes(1920, 1080, 1, 4) == 480 * 270 * 32
    assert lib.mipt_upsample_workspace_bytes(W, H, V, K) == NLO * 32
    assert lib.mipt_upsample_workspace_bytes(6, 4, 700, 2) == 4200 * 32
    assert lib.mipt_upsample_workspace_bytes(65528, 65528, 1, 8) == 8191 * 8191 * 32
    for bad in ((0, 4, 1, 2), (4, 0, 1, 2), (4, 4, 0, 2), (65536, 65536, 1, 2), (1 << 15, 1 << 15, 4, 2), (4, 4, 1, 0), (4, 4, 1, 1),
                (9, 9, 1, 9), (6, 4, 1, 4), (4, 6, 1, 4), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 3)):
        assert lib.mipt_upsample_workspace_bytes(*bad) == 0, bad
    assert lib.mipt_abi_version() == 4


def test_argument_checks_of_both_entries(rrt, orc):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    p = _Planes()
    inf, nan = float("inf"), float("nan")
    option_cases = [
        (dict(width=0), "width"), (dict(height=0), "height"), (dict(n_views=0), "n_views"),
        (dict(width=1 << 15, height=1 << 15, n_views=4), "below 2^32"), (dict(width=1 << 16, height=1 << 16, n_views=1), "below 2^32"),
        (dict(scale=0), "scale"), (dict(scale=1), "scale"), (dict(scale=9), "scale"),
        (dict(width=7), "width 7 is not a multiple of scale"), (dict(height=5), "height 5 is not a multiple of scale"),
        (dict(scale=4), "width 6 is not a multiple of scale"), (dict(width=8, scale=4, height=6), "height 6 is not a multiple of scale"),
        (dict(sigma_normal=0.0), "sigma_normal"), (dict(sigma_normal=nan), "sigma_normal"), (dict(sigma_normal=1e25), "sigma_normal"),
        (dict(sigma_depth=-0.5), "sigma_depth"), (dict(sigma_depth=inf), "sigma_depth"), (dict(sigma_depth=1e-25), "sigma_depth"),
        (dict(flags=1), "flags"), (dict(reserved=0), "reserved"), (dict(reserved=8), "reserved"),
    ]
    at = lambda k, off=0: p.a[k].ctypes.data + off  # noqa: E731
    buffer_cases = [
        (dict(lo_hdr=None), "null lo_hdr"), (dict(out=None), "null out"),
        (dict(lo_normal=None), "null lo_normal"), (dict(normal=None), "null normal"), (dict(lo_depth=None), "null lo_depth"),
        (dict(depth=None), "null depth"), (dict(lo_albedo=None), "null lo_albedo"), (dict(albedo=None), "null albedo"),
        (dict(lo_material=None), "null lo_material"), (dict(material=None), "null material"),
        (dict(reserved=0), "reserved buffer pointers"), (dict(reserved=4), "reserved buffer pointers"),
        (dict(lo_normal=at("lo_hdr")), "lo_normal overlaps lo_hdr"), (dict(lo_albedo=at("lo_hdr", 4)), "lo_albedo overlaps lo_hdr"),
        (dict(out=at("lo_hdr")), "out overlaps lo_hdr"), (dict(out=at("albedo")), "out overlaps albedo"),
        (dict(lo_depth=at("lo_normal", 4 * NLO)), "lo_depth overlaps lo_normal"), (dict(lo_material=at("lo_depth")), "lo_material overlaps lo_depth"),
        (dict(lo_material=at("normal", 8)), "normal overlaps lo_material"), (dict(depth=at("normal", 8)), "depth overlaps normal"),
        (dict(depth=at("albedo", 8 * N - 4)), "albedo overlaps depth"), (dict(material=at("albedo")), "material overlaps albedo"),
        (dict(material=at("out", 4)), "out overlaps material"), (dict(weight=at("out", 8 * N)), "weight overlaps out"),
        (dict(weight=at("lo_hdr")), "weight overlaps lo_hdr"), (dict(weight=at("normal", 4)), "weight overlaps normal"),
        (dict(lo_albedo=at("out", 12 * N - 4)), "out overlaps lo_albedo"),
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
    # what may be absent and a sigma given for an absent guide get past the checks: to the device (the host entry) or the
    # device-memory check (the device entry).  These calls get planes of their own: where a device exists the host entry runs, and
    # zeros upsample to zeros in `out` but not in `weight`, which is the sum of the accepted taps' weights -- the model's, bit for bit
    zeros = np.zeros((V, H // K, W // K, 3), dtype=F)
    guide_planes = lambda h, w: dict(normal=np.zeros((V, h, w, 3), dtype=F), depth=np.zeros((V, h, w), dtype=F),  # noqa: E731
                                     albedo=np.zeros((V, h, w, 3), dtype=F), material=np.zeros((V, h, w), dtype=np.uint32))
    for okw, bkw in ((dict(sigma_normal=nan), dict(lo_normal=None, normal=None)), (dict(sigma_depth=0.0), dict(lo_depth=None, depth=None)),
                     ({}, dict(lo_albedo=None, albedo=None)), ({}, dict(lo_material=None, material=None)), ({}, dict(weight=None)),
                     ({}, {k: None for k in WORDS if k not in ("lo_hdr", "out")})):
        q = _Planes()
        rc = lib.mipt_upsample(C.byref(_opt(L, **okw)), C.byref(q.bufs(L, **bkw)), 0)
        assert rc in (L.OK, L.ERR_HIP), (okw, bkw, rc, lib.mipt_last_error())
        assert lib.mipt_upsample_device(C.byref(_opt(L, **okw)), C.byref(q.bufs(L, **bkw)), q.ws.ctypes.data, q.ws.nbytes, None) == L.ERR_INVALID_ARG
        assert "lo_hdr is not device memory" in lib.mipt_last_error().decode()
        for k, a in q.a.items():
            if k != "weight":
                assert not a.any(), (okw, bkw, k)                       # inputs untouched, out all zero, nothing behind a plane
        weight = q.a["weight"]
        if rc == L.OK and "weight" not in bkw:
            passed = [g for g in GUIDES if g not in bkw]
            lo_g, hi_g = guide_planes(H // K, W // K), guide_planes(H, W)
            want = UM.upsample(orc, zeros, K, {g: lo_g[g] for g in passed}, {g: hi_g[g] for g in passed})[1]
            assert (want > 0).all() and np.array_equal(_bits(weight[: N]), _bits(want.reshape(-1))), (okw, bkw)
            assert not weight[N:].any()
        else:
            assert not weight.any(), (okw, bkw)                         # no device, or no weight plane passed: not written
    for a in p.a.values():
        assert not a.any()                                              # no refused call wrote anything


def test_device_entry_checks_workspace_alignment_and_memory(rrt):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    p = _Planes()
    f = lib.mipt_upsample_device
    o, b = _opt(L), p.bufs(L)
    ws, need = p.ws.ctypes.data, NLO * 32
    for args, msg in [((None, need), "null workspace"), ((ws, need - 1), "too small"), ((ws, 0), "too small"), ((ws + 4, need + 16), "workspace must be 16-byte aligned")]:
        assert f(C.byref(o), C.byref(b), *args, None) == L.ERR_INVALID_ARG, msg
        assert msg in lib.mipt_last_error().decode(), (msg, lib.mipt_last_error())
    for name in WORDS:
        bad = p.bufs(L, **{name: p.a[name].ctypes.data + 2})
        assert f(C.byref(o), C.byref(bad), ws, need, None) == L.ERR_INVALID_ARG
        assert f"{name} must be 4-byte aligned" in lib.mipt_last_error().decode(), (name, lib.mipt_last_error())
        inside = p.bufs(L, **{name: ws + need - 4})
        assert f(C.byref(o), C.byref(inside), ws, need, None) == L.ERR_INVALID_ARG
        assert f"{name} overlaps the workspace" in lib.mipt_last_error().decode(), (name, lib.mipt_last_error())
    # host memory is not device memory: refused by name, with or without a device
    assert f(C.byref(o), C.byref(b), ws, need, None) == L.ERR_INVALID_ARG
    assert "lo_hdr is not device memory" in lib.mipt_last_error().decode()


def test_host_entry_fails_loudly_without_a_device(rrt):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path is exercised on the CPU-only box")
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    p = _Planes()
    assert lib.mipt_upsample(C.byref(_opt(L)), C.byref(p.bufs(L)), 0) == L.ERR_HIP
    assert "hipSetDevice" in lib.mipt_last_error().decode()
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=1, output_image_dimensions=(W, H), output_image_path="x.png"))
    with pytest.raises(rrt.MiptError) as e:
        r.upsample(np.zeros((H // K, W // K, 3), dtype=np.float32), None, None, K)
    assert e.value.code == L.ERR_HIP


def test_renderer_upsample_checks_its_arguments(rrt):
    from rust_ray_tracing_amd import _lib as L
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=1, output_image_dimensions=(W, H), output_image_path="x.png"))
    h, w = H // K, W // K
    lo_hdr = np.zeros((V, h, w, 3), dtype=np.float32)
    lz, z = np.zeros((V, h, w), dtype=np.float32), np.zeros((V, H, W), dtype=np.float32)
    l3, f3 = np.zeros((V, h, w, 3), dtype=np.float32), np.zeros((V, H, W, 3), dtype=np.float32)
    lm, m = np.zeros((V, h, w), dtype=np.uint32), np.zeros((V, H, W), dtype=np.uint32)
    cases = [
        (dict(lo_hdr=np.zeros((h, w), dtype=np.float32)), "lo_hdr"), (dict(lo_hdr=np.zeros((h, w, 4), dtype=np.float32)), "lo_hdr"),
        (dict(lo_hdr=lo_hdr.astype(np.float64)), "lo_hdr"),
        (dict(scale=1), "scale"), (dict(scale=9), "scale"), (dict(scale=2.0), "scale"), (dict(scale=True), "scale"),
        (dict(lo_guides=[l3]), "lo_guides"), (dict(guides=(f3,)), "guides"),
        (dict(lo_guides=dict(normal=l3)), "normal"), (dict(guides=dict(normal=f3)), "lo_normal"),
        (dict(lo_guides=dict(material=lm), guides=dict(depth=z)), "lo_depth"),
        (dict(lo_guides=dict(normal=f3), guides=dict(normal=f3)), "lo_normal"), (dict(lo_guides=dict(normal=l3), guides=dict(normal=l3)), "normal"),
        (dict(lo_guides=dict(depth=lz), guides=dict(depth=z.astype(np.float64))), "depth"),
        (dict(lo_guides=dict(depth=l3), guides=dict(depth=z)), "lo_depth"),
        (dict(lo_guides=dict(albedo=l3), guides=dict(albedo=f3[0])), "albedo"),
        (dict(lo_guides=dict(material=lm.astype(np.float32)), guides=dict(material=m)), "lo_material"),
        (dict(lo_guides=dict(material=lm), guides=dict(material=m.astype(np.int32))), "material"),
    ]
    for kw, msg in cases:
        args = dict(dict(lo_hdr=lo_hdr, lo_guides=None, guides=None, scale=K), **kw)
        with pytest.raises(ValueError) as e:
            r.upsample(**args)
        assert str(e.value).startswith(msg + ":"), (kw, str(e.value))
    import torch
    with pytest.raises(ValueError) as e:
        r.upsample(lo_hdr, dict(depth=torch.zeros((V, h, w))), dict(depth=z), K)
    assert str(e.value).startswith("lo_depth:")
    with pytest.raises(ValueError) as e:
        r.upsample(torch.zeros((V, h, w, 3)), None, None, K)            # a host tensor
    assert str(e.value).startswith("lo_hdr:")
    # what the library checks comes back as its status and message; keys the filter does not use are ignored
    for kw, msg in [(dict(lo_guides=dict(normal=l3, position=l3), guides=dict(normal=f3), sigma_normal=float("nan")), "sigma_normal"),
                    (dict(lo_guides=dict(depth=lz), guides=dict(depth=z), sigma_depth=-1.0), "sigma_depth")]:
        args = dict(dict(lo_hdr=lo_hdr, lo_guides=None, guides=None, scale=K), **kw)
        with pytest.raises(rrt.MiptError) as e:
            r.upsample(**args)
        assert e.value.code == L.ERR_INVALID_ARG and msg in str(e.value), (kw, str(e.value))
    # render_denoised and render_sequence refuse a frame that is no multiple of k, and a k that is none, before any device work
    for dims, k, msg in (((7, 4), 2, "multiples"), ((6, 5), 2, "multiples"), ((6, 4), 4, "multiples"), ((6, 4), 1, "2 ... 8"), ((18, 18), 9, "2 ... 8"),
                         ((6, 4), 2.0, "2 ... 8")):
        rs = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=1, output_image_dimensions=dims, output_image_path="x.png",
                                                  seed_mode=L.SEED_PER_SAMPLE))
        with pytest.raises(ValueError) as e:
            rs.render_denoised(None, [None], upsample=k)
        assert msg in str(e.value) and "render_denoised" in str(e.value), (dims, k, str(e.value))
        with pytest.raises(ValueError) as e:
            next(rs.render_sequence(None, [[None]], denoise="variance", upsample=k))
        assert msg in str(e.value) and "render_sequence" in str(e.value), (dims, k, str(e.value))
