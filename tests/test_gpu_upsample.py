"""GPU: mipt_upsample / mipt_upsample_device (csrc/upsample.hip) against the model of tests/tools/upsample_model.py, which
tests/test_upsample_model.py holds to the contract's properties.  Every comparison is bit for bit on uint32 views (a NaN equals a
NaN: its sign and payload are the implementation's), for `out` and for `weight`.  The (low size, k) pairs are the smallest at which
the kernels can go wrong: the smallest frame, exactly one 64x4 tile, one lane short of and one lane past the tile row, the largest
k, more than one block both ways.  Each model frame is computed once per input."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import temporal_model as T  # noqa: E402
import upsample_model as UM  # noqa: E402
import variance_model as VM  # noqa: E402

pytestmark = pytest.mark.gpu

# (low size, k): full size, why
CASES = [((1, 1), 2),      # 2x2: the smallest frame
         ((3, 2), 2),      # 6x4
         ((5, 5), 3),      # 15x15
         ((16, 1), 4),     # 64x4: exactly one tile
         ((21, 2), 3),     # 63x6: one lane short of the tile row
         ((13, 3), 5),     # 65x15: one lane past the tile row
         ((17, 2), 4),     # 68x8
         ((8, 5), 8),      # 64x40: the largest k
         ((61, 37), 2)]    # 122x74: more than one block both ways
GUIDES = ("normal", "depth", "albedo", "material")
COMBOS = [tuple(g for g, on in zip(GUIDES, bits) if on) for bits in itertools.product((0, 1), repeat=4)]     # all sixteen
GWORDS = dict(normal=3, depth=1, albedo=3, material=1)
FIELDS = ("lo_hdr", "lo_normal", "lo_depth", "lo_albedo", "lo_material", "normal", "depth", "albedo", "material", "out", "weight")
POISON_F, POISON_I = 0x7FA5A5A5, 0x25A5A5A5                     # what a word nobody wrote holds (host buffers / int32 tensors)
ARGS = dict(sigma_normal=0.5, sigma_depth=0.5)
OTHER_MATERIAL = 77


def _words(field):
    return 3 if field in ("lo_hdr", "out") else 1 if field == "weight" else GWORDS[field.replace("lo_", "")]


def _fields(lo_size, k, views, seed=0):
    """random planes: lo_* [V,h,w(,c)] and the guides at [V,h*k,w*k(,c)].  Radiance in [0, 4); the full-resolution guides are the low
    ones repeated k times plus their own detail, so that the weights are neither all 1 nor all 0: normals of length about 1 in a few
    directions, depths in smooth patches with misses (1e30) beside hits, albedo in (0, 1] with detail finer than the low frame, and
    material ids in patches of 2x2 low pixels, one full pixel in eight of another material that no tap shares"""
    w, h = lo_size
    rng = np.random.default_rng(9000 * w + 10 * h + 100 * k + views + seed)
    rep = lambda a: np.repeat(np.repeat(a, k, axis=1), k, axis=2)  # noqa: E731
    H, W = h * k, w * k
    lo_hdr = (rng.random((views, h, w, 3)) ** 2 * 4.0).astype(np.float32)
    dirs = np.array([(0, 0, 1), (0, 1, 0), (0.6, 0, 0.8), (-1, 0, 0)], dtype=np.float32)
    lo_normal = (dirs[rng.integers(0, 4, (views, h, w)) * (rng.random((views, h, w)) < 0.3)] + rng.normal(0, 0.05, (views, h, w, 3))).astype(np.float32)
    normal = (rep(lo_normal) + rng.normal(0, 0.1, (views, H, W, 3))).astype(np.float32)
    lo_depth = (2.0 + 0.01 * np.arange(w)[None, None, :] + rng.random((views, h, w)) * 0.3).astype(np.float32)
    depth = (rep(lo_depth) + rng.normal(0, 0.1, (views, H, W))).astype(np.float32)
    lo_depth[rng.random((views, h, w)) < 0.15] = np.float32(1e30)
    depth[rng.random((views, H, W)) < 0.15] = np.float32(1e30)
    lo_albedo = (0.02 + 0.98 * rng.random((views, h, w, 3))).astype(np.float32)
    albedo = (0.02 + 0.98 * rng.random((views, H, W, 3))).astype(np.float32)
    patches = rng.integers(0, 3, (views, (h + 1) // 2, (w + 1) // 2)).astype(np.uint32)
    lo_material = np.ascontiguousarray(np.repeat(np.repeat(patches, 2, axis=1), 2, axis=2)[:, :h, :w])
    material = rep(lo_material).copy()
    material[rng.random((views, H, W)) < 0.125] = OTHER_MATERIAL
    return dict(lo_hdr=lo_hdr, lo_normal=lo_normal, lo_depth=lo_depth, lo_albedo=lo_albedo, lo_material=lo_material,
                normal=np.ascontiguousarray(normal), depth=depth, albedo=albedo, material=np.ascontiguousarray(material), scale=k)


def _passed(combo):
    return ("lo_hdr",) + tuple("lo_" + g for g in combo) + tuple(combo)


def _opt(L, planes, **args):
    v, h, w = planes["lo_depth"].shape
    k = planes["scale"]
    o = L.MiptUpsampleOptions()
    o.width, o.height, o.n_views, o.scale = w * k, h * k, v, k
    a = dict(ARGS, **args)
    o.sigma_normal, o.sigma_depth = a["sigma_normal"], a["sigma_depth"]
    return o


def _u32(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def _host(rrt, planes, combo, want_weight=True, **args):
    """mipt_upsample on copies of the planes, a sentinel word behind every plane -> (out [V,H,W,3], weight [V,H,W] or None)"""
    from rust_ray_tracing_amd import _lib as L
    v, H, W = planes["depth"].shape
    n = v * H * W
    b, keep = L.MiptUpsampleBuffers(), {}
    for f in _passed(combo):
        keep[f] = np.concatenate([_u32(planes[f]), [POISON_F]]).astype(np.uint32)
        setattr(b, f, keep[f].ctypes.data)
    out = np.full(n * 3 + 1, POISON_F, dtype=np.uint32)
    wt = np.full(n + 1, POISON_F, dtype=np.uint32)
    b.out = out.ctypes.data
    if want_weight:
        b.weight = wt.ctypes.data
    rc = rrt.load().mipt_upsample(C.byref(_opt(L, planes, **args)), C.byref(b), 0)
    assert rc == 0, (rc, rrt.load().mipt_last_error())
    for f, a in keep.items():
        assert a[-1] == POISON_F, f
        assert np.array_equal(a[:-1], _u32(planes[f])), f                   # an input is not written
    assert out[-1] == POISON_F and wt[-1] == POISON_F and (want_weight or np.all(wt == POISON_F))
    return out[:-1].view(np.float32).reshape(v, H, W, 3), (wt[:-1].view(np.float32).reshape(v, H, W) if want_weight else None)


def _device(rrt, planes, combo, want_weight=True, stream=None, **args):
    """mipt_upsample_device: all eleven planes are slices of one tensor, a plane that is not passed holds poison and must keep it; a
    sentinel word behind every plane and behind the workspace's declared size -> (out [V,H,W,3], weight [V,H,W] or None)"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    v, H, W = planes["depth"].shape
    k = planes["scale"]
    n, n_lo = v * H * W, v * H * W // (k * k)
    count = lambda f: n_lo if f.startswith("lo_") else n  # noqa: E731
    off, total = {}, 0
    for f in FIELDS:
        off[f], total = total, total + count(f) * _words(f) + 1
    host = np.full(total, POISON_I, dtype=np.uint32)
    for f in _passed(combo):
        host[off[f]: off[f] + count(f) * _words(f)] = _u32(planes[f])
    before = host.copy()
    t = torch.from_numpy(host.view(np.int32)).cuda()
    need = int(lib.mipt_upsample_workspace_bytes(W, H, v, k))
    assert need == n_lo * 32
    ws = torch.full((need // 4 + 4,), POISON_I, dtype=torch.int32, device="cuda")
    b = L.MiptUpsampleBuffers()
    for f in _passed(combo):
        setattr(b, f, t.data_ptr() + 4 * off[f])
    b.out = t.data_ptr() + 4 * off["out"]
    if want_weight:
        b.weight = t.data_ptr() + 4 * off["weight"]
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()                                                # the fills above ran on torch's current stream, which need not be `stream`
    rc = lib.mipt_upsample_device(C.byref(_opt(L, planes, **args)), C.byref(b), ws.data_ptr(), need, stream)
    assert rc == 0, (rc, lib.mipt_last_error())
    torch.cuda.synchronize()
    got = t.cpu().numpy().view(np.uint32)
    written = ("out",) + (("weight",) if want_weight else ())
    for f in FIELDS:
        lo, hi = off[f], off[f] + count(f) * _words(f)
        assert got[hi] == POISON_I, f                                      # nothing is written behind a plane
        if f not in written:
            assert np.array_equal(got[lo:hi], before[lo:hi]), f            # inputs, and a plane that was not passed, are untouched
    assert bool(torch.all(ws[need // 4:] == POISON_I))                      # nor behind the workspace's declared size
    if not any(g in combo for g in ("normal", "depth")):
        assert bool(torch.all(ws[n_lo * 4: need // 4] == POISON_I))         # plane 1 is written only when a normal or depth guide exists
    lo, lw = off["out"], off["weight"]
    return got[lo: lo + n * 3].view(np.float32).reshape(v, H, W, 3), (got[lw: lw + n].view(np.float32).reshape(v, H, W) if want_weight else None)


def _model(orc, planes, combo, **args):
    out, weight, _ = UM.upsample(orc, planes["lo_hdr"], planes["scale"], {g: planes["lo_" + g] for g in combo}, {g: planes[g] for g in combo},
                                 **dict(ARGS, **args))
    return out, weight


def _same(got, want):
    return UM.same_bits(got[0], want[0]) and (got[1] is None or UM.same_bits(got[1], want[1]))


def _differ(got, want):
    return (int((got[0].view(np.uint32) != want[0].view(np.uint32)).sum()),
            None if got[1] is None else int((got[1].view(np.uint32) != want[1].view(np.uint32)).sum()))


# ---- sizes x views x guide combinations x entries x with and without weight ------------------------------------------------------------
@pytest.mark.parametrize("views", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=[f"{w}x{h}-k{k}" for (w, h), k in CASES])
def test_random_fields_against_the_model(rrt, orc, case, views):
    lo_size, k = case
    planes = _fields(lo_size, k, views)
    for combo in COMBOS:
        want = _model(orc, planes, combo)
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
        for entry in (_host, _device):
            for want_weight in (True, False):
                got = entry(rrt, planes, combo, want_weight=want_weight)
                assert _same(got, want), (case, views, combo, entry.__name__, want_weight, _differ(got, want))


def test_within_one_wave_some_pixels_have_no_accepted_tap_and_some_all_four(rrt, orc):
    planes = _fields((61, 37), 2, 1, seed=1)
    lo_m, m = planes["lo_material"][0], planes["material"][0]
    row = 1                                                             # an odd row: ry = 1, so odd columns have four taps
    xs = np.arange(1, 64, 2)
    four = [(m[row, x] == lo_m[row // 2: row // 2 + 2, x // 2: x // 2 + 2]).all() for x in xs]
    assert any(four) and (m[row, :64] == OTHER_MATERIAL).any()
    for combo in (("material",), GUIDES):
        want = _model(orc, planes, combo)
        assert (want[1][0, row, :64] == 0).any() and (want[1][0, row, :64] > 0).any()
        for entry in (_host, _device):
            got = entry(rrt, planes, combo)
            assert _same(got, want), (combo, entry.__name__, _differ(got, want))


def test_special_values(rrt, orc):
    """zero, negative and NaN albedo at both resolutions, +-inf and NaN radiance, a NaN normal at both, misses beside hits: the NaN
    rule of the header, and the sides its comparisons name"""
    planes = _fields((61, 37), 2, 1, seed=2)
    planes["lo_hdr"][0, 5, 7, 1] = np.inf
    planes["lo_hdr"][0, 30, 50] = np.nan
    planes["lo_hdr"][0, 20, 3, 2] = -np.inf
    planes["lo_albedo"][0, 10, 10] = 0.0
    planes["lo_albedo"][0, 11, 40, 0] = np.nan
    planes["lo_albedo"][0, 12, 41, 2] = -0.5
    planes["lo_albedo"][0, 2, 2] = np.float32(1.0 / 256.0)                  # the floor itself: the comparison is strict
    planes["albedo"][0, 21, 21] = 0.0
    planes["albedo"][0, 22, 81, 0] = np.nan
    planes["albedo"][0, 25, 83, 2] = -0.5
    planes["albedo"][0, 4, 4] = np.float32(1.0 / 256.0)
    planes["lo_normal"][0, 25, 25, 0] = np.nan
    planes["normal"][0, 60, 100, 2] = np.nan
    planes["lo_depth"][0, 15:20, 30:35] = 1e30
    planes["lo_depth"][0, 17, 32] = 3.0                                     # one hit in a patch of misses
    planes["depth"][0, 30:40, 60:70] = 1e30
    planes["depth"][0, 35, 65] = 3.0
    planes["depth"][0, 50, 20] = np.nan
    for combo in COMBOS:
        want = _model(orc, planes, combo)
        assert np.isnan(want[0]).any() and np.isfinite(want[0]).sum() > want[0].size // 2
        for entry in (_host, _device):
            got = entry(rrt, planes, combo)
            assert _same(got, want), (combo, entry.__name__, _differ(got, want))
    # a NaN or zero albedo and a NaN normal alone leave everything finite
    clean = _fields((61, 37), 2, 1, seed=2)
    clean["lo_albedo"][0, 10, 10] = 0.0
    clean["albedo"][0, 22, 81, 0] = np.nan
    clean["lo_normal"][0, 25, 25, 0] = np.nan
    clean["normal"][0, 60, 100, 2] = np.nan
    want = _model(orc, clean, GUIDES)
    assert np.isfinite(want[0]).all() and want[1][0, 60, 100] == 0 and _same(_device(rrt, clean, GUIDES), want)


def test_options_reach_the_kernel(rrt, orc):
    planes = _fields((61, 37), 2, 1, seed=3)
    base = _model(orc, planes, GUIDES)
    for args in (dict(sigma_normal=2.5), dict(sigma_depth=7.0), dict(sigma_normal=1e4, sigma_depth=1e-4), dict(sigma_normal=0.05, sigma_depth=30.0)):
        want = _model(orc, planes, GUIDES, **args)
        assert not UM.same_bits(want[0], base[0]), args
        for entry in (_host, _device):
            got = entry(rrt, planes, GUIDES, **args)
            assert _same(got, want), (args, entry.__name__, _differ(got, want))


def test_many_tiny_views(rrt, orc):
    """700 views of 3x2 at k = 2 walk the (view, tile) decode far past one block"""
    planes = _fields((3, 2), 2, 700, seed=4)
    want = _model(orc, planes, GUIDES)
    assert _same(_device(rrt, planes, GUIDES), want)
    alone = _model(orc, {f: (a[5:6] if f != "scale" else a) for f, a in planes.items()}, GUIDES)
    assert UM.same_bits(want[0][5], alone[0][0]) and UM.same_bits(want[1][5], alone[1][0])     # views never see each other


CAP = 1 << 20                                                   # kFrameMaxGrid (csrc/tile_shape.h): workgroups per launch, one 64x4 tile per trip


def test_more_tiles_than_the_grid_holds(rrt, orc):
    """2^20 + 700 views of 2x2 pixels from 1x1 at k = 2 are as many tiles at both resolutions: 700 workgroups of the pack and of the
    upsampling kernel take a second trip, and the (view, tile) decode runs past 2^20.  Both outputs start as poison.  Views never
    see each other (test_many_tiny_views), so the model on a subset of the views -- the first and last 8, both sides of the first
    tile of the second trip, 2000 seeded others -- and every view against the same call made in chunks of 2^19 views -- below the
    cap, the path the tests above hold to the model -- cover every word of out and weight."""
    views = CAP + 700
    planes = _fields((1, 1), 2, views, seed=7)
    cut = lambda sl: {f: (a[sl] if f != "scale" else a) for f, a in planes.items()}  # noqa: E731
    got = _device(rrt, planes, GUIDES)
    assert not (got[0].view(np.uint32) == POISON_I).any() and not (got[1].view(np.uint32) == POISON_I).any()
    rng = np.random.default_rng(views)
    idx = np.unique(np.concatenate([np.arange(8), np.arange(views - 8, views), np.arange(CAP - 8, CAP + 8), rng.choice(views, 2000, replace=False)]))
    want = _model(orc, cut(idx), GUIDES)
    assert (want[1] > 0).any() and (want[1] == 0).any()                     # accepted taps and pixels without one
    assert _same((got[0][idx], got[1][idx]), want), _differ((got[0][idx], got[1][idx]), want)
    for lo in range(0, views, CAP // 2):
        part = _device(rrt, cut(slice(lo, lo + CAP // 2)), GUIDES)
        for g, p in zip(got, part):
            assert np.array_equal(g[lo: lo + CAP // 2].view(np.uint32), p.view(np.uint32)), lo


def _dicts(planes, conv):
    return {g: conv(planes["lo_" + g]) for g in GUIDES}, {g: conv(planes[g]) for g in GUIDES}


def test_torch_tensors_on_a_side_stream(rrt, orc):
    import torch
    planes = _fields((13, 3), 5, 3, seed=5)
    want = _model(orc, planes, GUIDES)
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=1, output_image_dimensions=(65, 15), output_image_path="/dev/null"))
    conv = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()  # noqa: E731
    lo_hdr = conv(planes["lo_hdr"])
    lo, hi = _dicts(planes, conv)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = torch.ones((1 << 22,), device="cuda").cumsum(0)               # work in front of the passes on the side stream
        a = r.upsample(lo_hdr, lo, hi, 5)                                    # torch's current stream
    b, bw = r.upsample(lo_hdr, lo, hi, 5, stream=side, want_weight=True)     # the one given
    c = _device(rrt, planes, GUIDES, stream=side.cuda_stream)
    side.synchronize()
    assert busy[-1].item() == float(1 << 22)
    assert a.is_cuda and tuple(a.shape) == (3, 15, 65, 3) and tuple(bw.shape) == (3, 15, 65)
    assert UM.same_bits(a.cpu().numpy(), want[0]) and _same((b.cpu().numpy(), bw.cpu().numpy()), want) and _same(c, want)
    for g in GUIDES:
        assert np.array_equal(_u32(lo[g].cpu().numpy()), _u32(planes["lo_" + g])) and np.array_equal(_u32(hi[g].cpu().numpy()), _u32(planes[g])), g
    # numpy arrays and a single view through the host entry; other sigmas and a subset of the guides
    nlo, nhi = _dicts(planes, lambda a: a[1])
    got = r.upsample(planes["lo_hdr"][1], nlo, nhi, 5, want_weight=True)
    assert isinstance(got[0], np.ndarray) and got[0].shape == (15, 65, 3) and got[1].shape == (15, 65)
    assert UM.same_bits(got[0], want[0][1]) and UM.same_bits(got[1], want[1][1])
    sub = ("depth", "material")
    got = r.upsample(planes["lo_hdr"], {g: planes["lo_" + g] for g in sub}, {g: planes[g] for g in sub}, 5, sigma_depth=0.1)
    assert UM.same_bits(got, _model(orc, planes, sub, sigma_depth=0.1)[0])


# ---- real frames: the buffers the render, the feature pass, the temporal step and the filter leave in HBM ---------------------------
_scenes = {}


def _scene(rrt, kind):
    if kind not in _scenes:
        from rust_ray_tracing_amd import synth
        kw = dict(n_target=20000, tex_size=64) if kind == "atrium" else {}
        tris, mats, texs, cam = synth.make_scene(kind, **kw)
        sc = rrt.Scene.from_arrays(tris, mats, texs)
        sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
        sc.upload(0)
        _scenes[kind] = sc
    return _scenes[kind]


def _moved(rrt, cam, dp=(0.0, 0.0, 0.0), dpitch=0.0, dyaw=0.0):
    c = rrt.Camera(position=tuple(float(cam.position[i]) + dp[i] for i in range(3)), pitch=cam.pitch + dpitch, yaw=cam.yaw + dyaw)
    c.update_view()
    return c


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _eq(a, b):
    return np.array_equal(_u32(a), _u32(b))


def _as_planes(lo_hdr, lo, hi, k):
    p = dict(lo_hdr=lo_hdr, scale=k)
    for g in GUIDES:
        p["lo_" + g], p[g] = lo[g].view(np.uint32) if g == "material" else lo[g], hi[g].view(np.uint32) if g == "material" else hi[g]
    return p


def _renderer(rrt, size, spp, **kw):
    from rust_ray_tracing_amd import _lib as L
    return rrt.Renderer.new(rrt.RendererOptions(samples=spp, max_ray_depth=8, output_image_dimensions=size, output_image_path="/dev/null",
                                                traversal=L.TRAVERSAL_CULLED, **kw))


@pytest.mark.parametrize("kind,size", [("cornell", (122, 74)), ("atrium", (64, 36))])
def test_render_denoised_with_upsampling(rrt, orc, kind, size):
    """render_denoised(upsample=2) is render_denoised at half the size, one full-resolution feature pass and mipt_upsample_device --
    the same stages called separately, and the model applied to the buffers the GPU produced; upsample=None is the call without it"""
    import torch
    sc = _scene(rrt, kind)
    w, h = size
    cams = [_moved(rrt, sc.camera), _moved(rrt, sc.camera, dp=(0.3, -0.2, 0.1), dpitch=7.0, dyaw=-11.0)]
    r, r_low = _renderer(rrt, size, 2), _renderer(rrt, (w // 2, h // 2), 2)
    for variance in (False, True):
        full, den, noisy, feat, feat_full, stats = r.render_denoised(sc, cams, variance=variance, upsample=2)
        torch.cuda.synchronize()
        assert tuple(full.shape) == (2, h, w, 3) and tuple(den.shape) == tuple(noisy.shape) == (2, h // 2, w // 2, 3)
        assert sorted(feat) == sorted(feat_full) == sorted(GUIDES) and tuple(feat_full["depth"].shape) == (2, h, w)
        den2, noisy2, feat2, _ = r_low.render_denoised(sc, cams, variance=variance)
        ff2, _ = _renderer(rrt, size, 1).render_features(sc, cams, GUIDES, device=True)
        torch.cuda.synchronize()
        assert _eq(den.cpu().numpy(), den2.cpu().numpy()) and _eq(noisy.cpu().numpy(), noisy2.cpu().numpy())
        for g in ("depth", "normal", "albedo"):
            assert _eq(feat[g].cpu().numpy(), feat2[g].cpu().numpy()), g
        for g in GUIDES:
            assert _eq(feat_full[g].cpu().numpy(), ff2[g].cpu().numpy()), g
        planes = _as_planes(den.cpu().numpy(), _np(feat), _np(feat_full), 2)
        want = _model(orc, planes, GUIDES)
        assert UM.same_bits(full.cpu().numpy(), want[0]) and _same(_device(rrt, planes, GUIDES), want)
        assert np.isfinite(want[0]).all() and (want[1] > 0).any()
    # its own sigmas pass through, the filter's too
    full3 = r.render_denoised(sc, cams, upsample=2, iterations=3, upsample_sigma_normal=0.1, upsample_sigma_depth=2.0)[0]
    den3, _, feat3, _ = r_low.render_denoised(sc, cams, iterations=3)
    torch.cuda.synchronize()
    planes = _as_planes(den3.cpu().numpy(), dict(_np(feat3), material=planes["lo_material"]), _np(feat_full), 2)
    assert UM.same_bits(full3.cpu().numpy(), _model(orc, planes, GUIDES, sigma_normal=0.1, sigma_depth=2.0)[0])
    # upsample=None: the four values of the call without it
    a, b = r.render_denoised(sc, cams, upsample=None), r.render_denoised(sc, cams)
    torch.cuda.synchronize()
    assert len(a) == len(b) == 4 and tuple(a[0].shape) == (2, h, w, 3) and sorted(a[2]) == ["albedo", "depth", "normal"]
    assert _eq(a[0].cpu().numpy(), b[0].cpu().numpy()) and _eq(a[1].cpu().numpy(), b[1].cpu().numpy())
    with pytest.raises(ValueError):
        r.render_denoised(sc, cams, upsample=4 if kind == "cornell" else 5)  # 122 and 36 are no multiples


@pytest.mark.parametrize("kind,size", [("cornell", (122, 74)), ("atrium", (64, 36))])
def test_render_sequence_with_upsampling(rrt, orc, kind, size):
    """render_sequence(upsample=2, denoise="variance") over 3 frames: every key keeps its meaning at half the size -- the sequence a
    renderer of that size yields -- and out_full is mipt_upsample_device, and the model, applied to `out` and the two feature dicts"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    sc = _scene(rrt, kind)
    w, h = size
    path = [[_moved(rrt, sc.camera, **T.COVERAGE_MOVE)], [_moved(rrt, sc.camera)], [_moved(rrt, sc.camera, dp=(0.02, 0.0, 0.01), dyaw=0.4)]]
    r = _renderer(rrt, size, 1, seed_mode=L.SEED_PER_SAMPLE)
    r_low = _renderer(rrt, (w // 2, h // 2), 1, seed_mode=L.SEED_PER_SAMPLE)
    r_feat = _renderer(rrt, size, 1, seed_mode=L.SEED_PER_SAMPLE)
    keys = ("out", "accumulated", "noisy", "length", "variance")

    def collect(rr, **kw):
        frames = []
        for fr in rr.render_sequence(sc, path, denoise="variance", max_history=16.0, **kw):
            torch.cuda.synchronize()
            frames.append({k: fr[k].cpu().numpy() for k in keys + (("out_full",) if "out_full" in fr else ())})
            frames[-1]["features"] = _np(fr["features"])
            if "features_full" in fr:
                frames[-1]["features_full"] = _np(fr["features_full"])
        return frames

    up, low, none = collect(r, upsample=2), collect(r_low), collect(r, upsample=None)
    assert len(up) == len(low) == len(none) == 3
    for f in range(3):
        for k in keys:
            assert _eq(up[f][k], low[f][k]), (f, k)
        assert sorted(up[f]["features"]) == sorted(low[f]["features"])
        for k, a in low[f]["features"].items():
            assert _eq(up[f]["features"][k], a), (f, k)
        assert "out_full" not in low[f] and "out_full" not in none[f] and "features_full" not in none[f]
        assert tuple(none[f]["out"].shape) == (1, h, w, 3) and tuple(up[f]["out"].shape) == (1, h // 2, w // 2, 3)
        assert tuple(up[f]["out_full"].shape) == (1, h, w, 3) and sorted(up[f]["features_full"]) == sorted(GUIDES)
        ff, _ = r_feat.render_features(sc, path[f], GUIDES, device=True)
        for g in GUIDES:
            assert _eq(up[f]["features_full"][g], ff[g].cpu().numpy()), (f, g)
        planes = _as_planes(up[f]["out"], up[f]["features"], up[f]["features_full"], 2)
        want = _model(orc, planes, GUIDES)
        assert UM.same_bits(up[f]["out_full"], want[0]), f
        assert _same(_device(rrt, planes, GUIDES), want), f
        # the low frame is the variance filter's, as before
        feat = up[f]["features"]
        assert VM.same_bits(up[f]["out"], VM.denoise_variance(orc, up[f]["accumulated"], up[f]["variance"], up[f]["length"], feat["normal"], feat["depth"],
                                                              feat["albedo"], **VM.DEFAULTS)[0]), f
    # upsample=None is the sequence without the argument
    plain = []
    for fr in r.render_sequence(sc, path, denoise="variance", max_history=16.0):
        torch.cuda.synchronize()
        plain.append(fr["out"].cpu().numpy())
    assert all(_eq(plain[f], none[f]["out"]) for f in range(3))
    # its own sigmas pass through; anything else unknown is refused by name, and so is a size that is no multiple
    fr = next(r.render_sequence(sc, path[:1], denoise="variance", max_history=16.0, upsample=2, upsample_sigma_normal=0.1))
    torch.cuda.synchronize()
    planes = _as_planes(up[0]["out"], up[0]["features"], up[0]["features_full"], 2)
    assert UM.same_bits(fr["out_full"].cpu().numpy(), _model(orc, planes, GUIDES, sigma_normal=0.1)[0])
    with pytest.raises(ValueError):
        next(r.render_sequence(sc, path[:1], denoise="variance", upsample=2, upsample_sigma_color=1.0))
    with pytest.raises(ValueError):
        next(r.render_sequence(sc, path[:1], denoise="variance", upsample=4 if kind == "cornell" else 5))


# ---- refusals: status, a message naming the field, nothing written, and everything works as before ------------------------------------
def test_refusals_leave_everything_as_before(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc = _scene(rrt, "cornell")
    hdr0 = np.zeros((12, 16, 3), dtype=np.float32)
    ro = rrt.make_options(16, 12, 2, 3)
    L.check(lib.mipt_render(sc._handle, L.ptr(sc.camera.uniform), C.byref(ro), L.ptr(hdr0), None, None), "mipt_render")
    lo_size, k, views = (17, 2), 4, 1
    planes = _fields(lo_size, k, views, seed=6)
    want = _model(orc, planes, GUIDES)
    assert _same(_device(rrt, planes, GUIDES), want)
    n_lo = lo_size[0] * lo_size[1]
    n = n_lo * k * k
    need = n_lo * 32
    t = torch.full((n * 12 + n_lo * 12 + 64,), POISON_I, dtype=torch.int32, device="cuda")
    ws = torch.full((need // 4 + 4,), POISON_I, dtype=torch.int32, device="cuda")
    host = np.full(n * 3, POISON_F, dtype=np.uint32)
    base = t.data_ptr()
    ptr, at = {}, 0
    for f in FIELDS:                                                         # 16 bytes between planes
        ptr[f], at = base + at, at + 4 * (n_lo if f.startswith("lo_") else n) * _words(f) + 16

    def bufs(**kw):
        b = L.MiptUpsampleBuffers()
        for f, v in dict(ptr, **kw).items():
            if f == "reserved":
                b.reserved[v] = base
            else:
                setattr(b, f, v)
        return b

    def opt(**kw):
        o = _opt(L, planes)
        for f, v in kw.items():
            if f == "reserved":
                o.reserved[v] = 1
            else:
                setattr(o, f, v)
        return o

    def refused(msg, o=None, b=None, workspace=None, nbytes=need):
        o = opt() if o is None else o
        b = bufs() if b is None else b
        rc = lib.mipt_upsample_device(C.byref(o) if o != "null" else None, C.byref(b) if b != "null" else None,
                                      ws.data_ptr() if workspace is None else workspace, nbytes, None)
        err = lib.mipt_last_error().decode()
        assert rc == L.ERR_INVALID_ARG and msg in err and err.startswith("mipt_upsample_device:"), (msg, rc, err)

    inf, nan = float("inf"), float("nan")
    refused("opt", o="null")
    refused("buffers", b="null")
    refused("null lo_hdr", b=bufs(lo_hdr=None))
    refused("null out", b=bufs(out=None))
    for g in GUIDES:
        refused("null lo_" + g, b=bufs(**{"lo_" + g: None}))
        refused("null " + g, b=bufs(**{g: None}))
    for kw, msg in [(dict(width=0), "width"), (dict(height=0), "height"), (dict(n_views=0), "n_views"), (dict(width=1 << 16, height=1 << 16), "below 2^32"),
                    (dict(scale=1), "scale"), (dict(scale=9), "scale"), (dict(width=70), "width 70 is not a multiple"), (dict(height=6), "height 6 is not a multiple"),
                    (dict(scale=3), "is not a multiple"), (dict(sigma_normal=inf), "sigma_normal"), (dict(sigma_normal=nan), "sigma_normal"),
                    (dict(sigma_depth=-1.0), "sigma_depth"), (dict(sigma_depth=1e-25), "sigma_depth"), (dict(flags=2), "flags"), (dict(reserved=3), "reserved")]:
        refused(msg, o=opt(**kw))
    refused("reserved buffer pointers", b=bufs(reserved=1))
    refused("lo_normal overlaps lo_hdr", b=bufs(lo_normal=base + 4))
    refused("out overlaps albedo", b=bufs(out=ptr["albedo"]))
    refused("out overlaps lo_hdr", b=bufs(out=base, lo_normal=None, normal=None, lo_depth=None, depth=None, lo_albedo=None, albedo=None,
                                          lo_material=None, material=None, weight=None))
    refused("weight overlaps out", b=bufs(weight=ptr["out"] + 8))
    refused("weight overlaps material", b=bufs(weight=ptr["material"]))
    refused("normal overlaps lo_material", b=bufs(lo_material=ptr["normal"] + 12 * n - 4))
    refused("depth overlaps lo_depth", b=bufs(lo_depth=ptr["depth"] + 4))
    refused("null workspace", workspace=0)
    refused("too small", nbytes=need - 16)
    refused("workspace must be 16-byte aligned", workspace=ws.data_ptr() + 8)
    refused("depth must be 4-byte aligned", b=bufs(depth=ptr["depth"] + 1))
    refused("lo_material must be 4-byte aligned", b=bufs(lo_material=ptr["lo_material"] + 2))
    refused("weight must be 4-byte aligned", b=bufs(weight=ptr["weight"] + 2))
    refused("lo_depth overlaps the workspace", b=bufs(lo_depth=ws.data_ptr() + 16 * n_lo))
    refused("weight overlaps the workspace", b=bufs(weight=ws.data_ptr() + need - 4))
    assert base % 16 == 0
    refused("lo_hdr overlaps the workspace", workspace=base)
    refused("albedo is not device memory of lo_hdr's device", b=bufs(albedo=host.ctypes.data))
    refused("weight is not device memory of lo_hdr's device", b=bufs(weight=host.ctypes.data))
    refused("workspace is not device memory of lo_hdr's device", workspace=(host.ctypes.data + 15) & ~15, nbytes=1 << 40)
    refused("lo_hdr is not device memory", b=bufs(lo_hdr=host.ctypes.data))
    assert bool(torch.all(t == POISON_I)) and bool(torch.all(ws == POISON_I)) and np.all(host == POISON_F)      # no refused call wrote anything
    # the host entry refuses the same way
    b = L.MiptUpsampleBuffers()
    b.lo_hdr, b.out = host.ctypes.data, host.ctypes.data + 4
    assert lib.mipt_upsample(C.byref(opt()), C.byref(b), 0) == L.ERR_INVALID_ARG and "out overlaps lo_hdr" in lib.mipt_last_error().decode()
    keep = np.full(n * 3, POISON_F, dtype=np.uint32)
    b.out = keep.ctypes.data
    assert lib.mipt_upsample(C.byref(opt()), C.byref(b), 1 << 20) == L.ERR_HIP and np.all(host == POISON_F) and np.all(keep == POISON_F)   # no such device
    # the scene renders and a following call works as before
    hdr1 = np.zeros_like(hdr0)
    L.check(lib.mipt_render(sc._handle, L.ptr(sc.camera.uniform), C.byref(ro), L.ptr(hdr1), None, None), "mipt_render")
    assert np.array_equal(hdr0.view(np.uint32), hdr1.view(np.uint32))
    assert _same(_device(rrt, planes, GUIDES), want) and _same(_host(rrt, planes, GUIDES), want)
