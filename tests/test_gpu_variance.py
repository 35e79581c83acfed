"""GPU: mipt_denoise_variance / mipt_denoise_variance_device (csrc/denoise_variance.hip) against the model of
tests/tools/variance_model.py, which tests/test_variance_model.py holds to the contract's properties.  Every comparison is bit for bit
on uint32 views (a NaN equals a NaN: its sign and payload are the implementation's), for `out` and for `variance_out`.  The frames are
the smallest at which the kernels can go wrong: one pixel, less than the 3x3, the 5x5 and a step's reach, one lane short of and one
lane past the 64-pixel tile row, more than one block both ways; steps up to 128 on all of them.  Each model frame is computed once per
input."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import denoise_model as D  # noqa: E402
import temporal_model as T  # noqa: E402
import variance_model as VM  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 2), (5, 5), (63, 5), (65, 9), (61, 37)]
GUIDES = ("normal", "depth", "albedo")
COMBOS = [tuple(g for g, on in zip(GUIDES, bits) if on) for bits in itertools.product((0, 1), repeat=3)]     # all eight
HISTORY = ("variance", "length")
WORDS = dict(hdr=3, normal=3, depth=1, albedo=3, variance=1, length=1, out=3, variance_out=1)
POISON_F, POISON_I = 0x7FA5A5A5, 0x25A5A5A5                     # what a word nobody wrote holds (host buffers / int32 tensors)
ARGS = dict(sigma_luminance=16.0, sigma_normal=0.5, sigma_depth=0.5, short_history=4.0)
SHORT = (0.0, 4.0, 1e9)                                         # never, some pixels of every wave, every pixel


def _fields(size, views, seed=0):
    """random planes [V,H,W(,k)]: radiance in [0, 4), normals of length about 1 in a few directions, depths in smooth patches with
    misses (1e30) beside hits, albedo in (0, 1], variances from 0 up and history lengths drawn per pixel from 1 ... 32, so that both
    sides of short_history = 4 occur among the 64 neighbours of a wave"""
    w, h = size
    rng = np.random.default_rng(7000 * w + 10 * h + views + seed)
    hdr = (rng.random((views, h, w, 3)) ** 2 * 4.0).astype(np.float32)
    dirs = np.array([(0, 0, 1), (0, 1, 0), (0.6, 0, 0.8), (-1, 0, 0)], dtype=np.float32)
    normal = dirs[rng.integers(0, 4, (views, h, w)) * (rng.random((views, h, w)) < 0.3)] + rng.normal(0, 0.05, (views, h, w, 3)).astype(np.float32)
    depth = (2.0 + 0.01 * np.arange(w)[None, None, :] + rng.random((views, h, w)) * 0.3).astype(np.float32)
    depth[rng.random((views, h, w)) < 0.15] = np.float32(1e30)
    albedo = (0.02 + 0.98 * rng.random((views, h, w, 3))).astype(np.float32)
    variance = (rng.random((views, h, w)) ** 3 * 2.0).astype(np.float32)
    variance[rng.random((views, h, w)) < 0.2] = 0.0
    length = np.float32([1.0, 2.0, 3.0, 3.75, 4.0, 5.5, 17.0, 32.0])[rng.integers(0, 8, (views, h, w))]
    return dict(hdr=hdr, normal=np.ascontiguousarray(normal, dtype=np.float32), depth=depth, albedo=albedo, variance=variance, length=length)


def _opt(L, size, views, iterations, **args):
    o = L.MiptVarianceOptions()
    o.width, o.height, o.n_views, o.iterations = size[0], size[1], views, iterations
    a = dict(ARGS, **args)
    o.sigma_luminance, o.sigma_normal, o.sigma_depth, o.short_history = a["sigma_luminance"], a["sigma_normal"], a["sigma_depth"], a["short_history"]
    return o


def _host(rrt, planes, combo, iterations, inplace=False, **args):
    """mipt_denoise_variance on copies of the planes, a sentinel word behind every plane -> (out [V,H,W,3], variance_out [V,H,W])"""
    from rust_ray_tracing_amd import _lib as L
    v, h, w = planes["depth"].shape
    n = v * h * w
    b, keep = L.MiptVarianceBuffers(), {}
    for k in ("hdr",) + tuple(combo):
        keep[k] = np.concatenate([planes[k].reshape(-1).view(np.uint32), [POISON_F]]).astype(np.uint32)
        setattr(b, k, keep[k].ctypes.data)
    out = keep["hdr"] if inplace else np.full(n * 3 + 1, POISON_F, dtype=np.uint32)
    var = np.full(n + 1, POISON_F, dtype=np.uint32)
    b.out, b.variance_out = out.ctypes.data, var.ctypes.data
    rc = rrt.load().mipt_denoise_variance(C.byref(_opt(L, (w, h), v, iterations, **args)), C.byref(b), 0)
    assert rc == 0, (rc, rrt.load().mipt_last_error())
    for k, a in keep.items():
        assert a[-1] == POISON_F, k
        if not (inplace and k == "hdr"):
            assert np.array_equal(a[:-1], planes[k].reshape(-1).view(np.uint32)), k           # an input is not written
    assert out[-1] == POISON_F and var[-1] == POISON_F
    return out[:-1].view(np.float32).reshape(v, h, w, 3), var[:-1].view(np.float32).reshape(v, h, w)


def _device(rrt, planes, combo, iterations, inplace=False, stream=None, want_var=True, **args):
    """mipt_denoise_variance_device: all eight planes are slices of one tensor, a plane that is not passed holds poison and must keep
    it; a sentinel word behind every plane and behind the workspace's declared size -> (out [V,H,W,3], variance_out [V,H,W] or None)"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    v, h, w = planes["depth"].shape
    n = v * h * w
    off, total = {}, 0
    for k, words in WORDS.items():
        off[k], total = total, total + n * words + 1
    host = np.full(total, POISON_I, dtype=np.uint32)
    for k in ("hdr",) + tuple(combo):
        host[off[k]: off[k] + n * WORDS[k]] = planes[k].reshape(-1).view(np.uint32)
    before = host.copy()
    t = torch.from_numpy(host.view(np.int32)).cuda()
    need = int(lib.mipt_denoise_variance_workspace_bytes(w, h, v))
    assert need == n * 48
    ws = torch.full((need // 4 + 4,), POISON_I, dtype=torch.int32, device="cuda")
    b = L.MiptVarianceBuffers()
    for k in ("hdr",) + tuple(combo):
        setattr(b, k, t.data_ptr() + 4 * off[k])
    b.out = t.data_ptr() + 4 * off["hdr" if inplace else "out"]
    if want_var:
        b.variance_out = t.data_ptr() + 4 * off["variance_out"]
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()                                                # the fills above ran on torch's current stream, which need not be `stream`
    rc = lib.mipt_denoise_variance_device(C.byref(_opt(L, (w, h), v, iterations, **args)), C.byref(b), ws.data_ptr(), need, stream)
    assert rc == 0, (rc, lib.mipt_last_error())
    torch.cuda.synchronize()
    got = t.cpu().numpy().view(np.uint32)
    written = ("hdr" if inplace else "out",) + (("variance_out",) if want_var else ())
    for k, words in WORDS.items():
        lo, hi = off[k], off[k] + n * words
        assert got[hi] == POISON_I, k                                      # nothing is written behind a plane
        if k not in written:
            assert np.array_equal(got[lo:hi], before[lo:hi]), k            # inputs, and a plane that was not passed, are untouched
    assert bool(torch.all(ws[need // 4:] == POISON_I))                      # nor behind the workspace's declared size
    lo, lv = off[written[0]], off["variance_out"]
    return got[lo: lo + n * 3].view(np.float32).reshape(v, h, w, 3), (got[lv: lv + n].view(np.float32).reshape(v, h, w) if want_var else None)


def _model(orc, planes, combo, iterations, **args):
    return VM.denoise_variance(orc, planes["hdr"], **{k: planes[k] for k in combo}, iterations=iterations, **dict(ARGS, **args))


def _same(got, want):
    return VM.same_bits(got[0], want[0]) and (got[1] is None or VM.same_bits(got[1], want[1]))


def _differ(got, want):
    return (int((got[0].view(np.uint32) != want[0].view(np.uint32)).sum()), int((got[1].view(np.uint32) != want[1].view(np.uint32)).sum()))


# ---- sizes x views x iterations x guide combinations x history x short_history x entries --------------------------------------------
@pytest.mark.parametrize("iterations", [1, 5, 8])
@pytest.mark.parametrize("views", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_random_fields_against_the_model(rrt, orc, size, views, iterations):
    planes = _fields(size, views)
    if size[0] >= 63:                                                        # both sides of short_history within the first wave's row
        row = planes["length"][0, 0, :63]
        assert (row < 4.0).any() and (row >= 4.0).any()
    changed = 0
    for combo in COMBOS:
        for history in ((), HISTORY):
            for sh in SHORT:
                want = _model(orc, planes, combo + history, iterations, short_history=sh)
                assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
                changed += not VM.same_bits(want[0], planes["hdr"])
                for entry in (_host, _device):
                    got = entry(rrt, planes, combo + history, iterations, short_history=sh)
                    assert _same(got, want), (size, views, iterations, combo, history, sh, entry.__name__, _differ(got, want))
    # the filter does something on every frame but the single pixel, except where nothing has any variance: no history and no estimate
    assert changed >= 40 or size == (1, 1)


@pytest.mark.parametrize("entry", ["host", "device"])
def test_out_may_be_hdr(rrt, orc, entry):
    f = _host if entry == "host" else _device
    for size, views, iterations in (((65, 9), 3, 5), ((61, 37), 1, 8), ((3, 2), 1, 1)):
        planes = _fields(size, views, seed=1)
        for combo in (COMBOS[0], COMBOS[-1] + HISTORY):
            want = _model(orc, planes, combo, iterations)
            assert _same(f(rrt, planes, combo, iterations, inplace=True), want), (size, combo)


def test_variance_out_is_optional(rrt, orc):
    planes = _fields((65, 9), 3, seed=8)
    want = _model(orc, planes, GUIDES + HISTORY, 5)
    got = _device(rrt, planes, GUIDES + HISTORY, 5, want_var=False)          # its plane keeps the poison (checked inside)
    assert got[1] is None and VM.same_bits(got[0], want[0])


def test_special_values(rrt, orc):
    """an inf and a NaN radiance, a zero, a negative and a NaN albedo, a NaN normal, misses beside hits, a NaN, a negative and an
    infinite variance and a NaN length: the NaN rule of the header, and the sides its comparisons name"""
    size, views = (61, 37), 1
    planes = _fields(size, views, seed=2)
    planes["hdr"][0, 5, 7, 1] = np.inf
    planes["hdr"][0, 30, 50] = np.nan
    planes["hdr"][0, 20, 3, 2] = -np.inf
    planes["albedo"][0, 10, 10] = 0.0
    planes["albedo"][0, 11, 40, 0] = np.nan
    planes["albedo"][0, 12, 41, 2] = -0.5
    planes["albedo"][0, 2, 2] = np.float32(1.0 / 256.0)                      # the floor itself: the comparison is strict
    planes["normal"][0, 25, 25, 0] = np.nan
    planes["depth"][0, 15:20, 30:35] = 1e30
    planes["depth"][0, 17, 32] = 3.0                                         # one hit in a patch of misses
    planes["variance"][0, 8, 20] = np.nan
    planes["variance"][0, 9, 45] = -1.0
    planes["variance"][0, 33, 12] = np.inf
    planes["variance"][0, 34, 55] = -np.inf
    planes["length"][0, 28, 20] = np.nan
    planes["length"][0, 3, 33] = np.inf
    planes["length"][0, 4, 50] = -2.0
    planes["length"][0, 6, 58] = 0.0
    for iterations in (1, 2):                                                # a NaN reaches 2 * (1 + 2) pixels each way: most of the frame stays finite
        for combo in COMBOS:
            for history in ((), HISTORY):
                for sh in (0.0, 4.0):
                    want = _model(orc, planes, combo + history, iterations, short_history=sh)
                    assert np.isnan(want[0]).any() and np.isfinite(want[0]).sum() > want[0].size // 2
                    for entry in (_host, _device):
                        got = entry(rrt, planes, combo + history, iterations, short_history=sh)
                        assert _same(got, want), (iterations, combo, history, sh, entry.__name__, _differ(got, want))
    # NaN / negative variances, a NaN length and a NaN or zero albedo alone leave everything finite
    clean = _fields(size, views, seed=2)
    clean["albedo"][0, 10, 10] = 0.0
    clean["albedo"][0, 11, 40, 0] = np.nan
    clean["variance"][0, 8, 20] = np.nan
    clean["variance"][0, 9, 45] = -1.0
    clean["length"][0, 28, 20] = np.nan
    want = _model(orc, clean, ("albedo",) + HISTORY, 5)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and _same(_device(rrt, clean, ("albedo",) + HISTORY, 5), want)


def test_options_reach_the_kernel(rrt, orc):
    planes = _fields((61, 37), 1, seed=3)
    combo = GUIDES + HISTORY
    base = _model(orc, planes, combo, 5)
    for args in (dict(sigma_luminance=0.37), dict(sigma_normal=2.5), dict(sigma_depth=7.0), dict(short_history=2.5), dict(short_history=20.0),
                 dict(sigma_luminance=1e-3, sigma_normal=1e4, sigma_depth=1e-4), dict(sigma_luminance=3e38)):
        want = _model(orc, planes, combo, 5, **args)
        assert not VM.same_bits(want[0], base[0]), args
        for entry in (_host, _device):
            got = entry(rrt, planes, combo, 5, **args)
            assert _same(got, want), (args, entry.__name__, _differ(got, want))


def test_many_tiny_views(rrt, orc):
    """700 views of 3x2 walk the (view, tile) decode far past one block"""
    planes = _fields((3, 2), 700, seed=4)
    combo = GUIDES + HISTORY
    want = _model(orc, planes, combo, 2)
    assert _same(_device(rrt, planes, combo, 2), want)
    alone = _model(orc, {k: a[5:6] for k, a in planes.items()}, combo, 2)
    assert VM.same_bits(want[0][5], alone[0][0]) and VM.same_bits(want[1][5], alone[1][0])     # views never see each other


CAP = 1 << 20                                                   # kFrameMaxGrid (csrc/tile_shape.h): workgroups per launch, one 64x4 tile per trip


def test_more_tiles_than_the_grid_holds(rrt, orc):
    """2^20 + 700 views of 2x1 pixels are as many tiles: 700 workgroups of the pack, the estimate and both passes take a second trip,
    and the (view, tile) decode runs past 2^20.  Every pixel has one neighbour, so a tap beside the centre is weighed.  Both outputs
    start as poison.  Views never see each other (test_many_tiny_views), so the model on a subset of the views -- the first and last
    8, both sides of the first tile of the second trip, 2000 seeded others -- and every view against the same call made in chunks
    of 2^19 views -- below the cap, the path the tests above hold to the model -- cover every word of out and variance_out."""
    views = CAP + 700
    planes = _fields((2, 1), views, seed=7)
    combo = GUIDES + HISTORY
    got = _device(rrt, planes, combo, 2)
    assert not (got[0].view(np.uint32) == POISON_I).any() and not (got[1].view(np.uint32) == POISON_I).any()
    rng = np.random.default_rng(views)
    idx = np.unique(np.concatenate([np.arange(8), np.arange(views - 8, views), np.arange(CAP - 8, CAP + 8), rng.choice(views, 2000, replace=False)]))
    want = _model(orc, {k: a[idx] for k, a in planes.items()}, combo, 2)
    assert not VM.same_bits(want[0], planes["hdr"][idx])
    assert _same((got[0][idx], got[1][idx]), want), _differ((got[0][idx], got[1][idx]), want)
    for lo in range(0, views, CAP // 2):
        part = _device(rrt, {k: a[lo: lo + CAP // 2] for k, a in planes.items()}, combo, 2)
        for g, p in zip(got, part):
            assert np.array_equal(g[lo: lo + CAP // 2].view(np.uint32), p.view(np.uint32)), lo


def test_torch_tensors_on_a_side_stream(rrt, orc):
    import torch
    planes = _fields((65, 9), 3, seed=5)
    want = _model(orc, planes, GUIDES + HISTORY, 5)
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=1, output_image_dimensions=(65, 9), output_image_path="/dev/null"))
    dev = {k: torch.from_numpy(a).cuda() for k, a in planes.items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    call = lambda **kw: r.denoise_variance(dev["hdr"], dev["variance"], dev["length"], dev["normal"], dev["depth"], dev["albedo"], **kw)  # noqa: E731
    with torch.cuda.stream(side):
        busy = torch.ones((1 << 22,), device="cuda").cumsum(0)               # work in front of the passes on the side stream
        a = call()                                                           # torch's current stream
    b, bv = call(stream=side, want_variance=True)                            # the one given
    c = _device(rrt, planes, GUIDES + HISTORY, 5, stream=side.cuda_stream)
    side.synchronize()
    assert busy[-1].item() == float(1 << 22)
    assert a.is_cuda and tuple(a.shape) == planes["hdr"].shape and tuple(bv.shape) == planes["depth"].shape
    assert VM.same_bits(a.cpu().numpy(), want[0]) and _same((b.cpu().numpy(), bv.cpu().numpy()), want) and _same(c, want)
    for k, t in dev.items():
        assert np.array_equal(t.cpu().numpy().view(np.uint32), planes[k].view(np.uint32)), k       # the inputs are not written
    # numpy arrays and a single view through the host entry
    got = r.denoise_variance(planes["hdr"][1], planes["variance"][1], planes["length"][1], planes["normal"][1], planes["depth"][1], planes["albedo"][1],
                             want_variance=True)
    assert isinstance(got[0], np.ndarray) and got[0].shape == (9, 65, 3) and got[1].shape == (9, 65)
    assert VM.same_bits(got[0], want[0][1]) and VM.same_bits(got[1], want[1][1])


# ---- real frames: the buffers the render, the feature pass and the temporal step leave in HBM ---------------------------------------
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


@pytest.mark.parametrize("kind,size,spp", [("cornell", (61, 37), 1), ("atrium", (64, 36), 2)])
def test_render_sequence_with_the_variance_filter(rrt, orc, kind, size, spp):
    """render_sequence(denoise="variance") is the temporal step's planes handed to mipt_denoise_variance_device, and the model
    applied to the buffers the GPU produced; denoise=True and False give what they gave before this filter existed"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    sc = _scene(rrt, kind)
    w, h = size
    path = [[_moved(rrt, sc.camera, **T.COVERAGE_MOVE)], [_moved(rrt, sc.camera)], [_moved(rrt, sc.camera, dp=(0.02, 0.0, 0.01), dyaw=0.4)]]
    r = rrt.Renderer.new(rrt.RendererOptions(samples=spp, max_ray_depth=8, output_image_dimensions=size, output_image_path="/dev/null",
                                             seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED))

    def collect(**kw):
        frames = []
        for fr in r.render_sequence(sc, path, max_history=16.0, **kw):
            torch.cuda.synchronize()
            frames.append({k: fr[k].cpu().numpy() for k in ("out", "accumulated", "noisy", "length", "variance")})
            frames[-1]["features"] = {k: v.cpu().numpy() for k, v in fr["features"].items()}
        return frames

    guided, fixed, plain = collect(denoise="variance"), collect(denoise=True), collect(denoise=False)
    assert len(guided) == len(fixed) == len(plain) == 3
    reused = 0
    for f in range(3):
        g, feat = guided[f], guided[f]["features"]
        for other in (fixed[f], plain[f]):                                   # the same frames up to the filter
            for k in ("accumulated", "noisy", "length", "variance"):
                assert np.array_equal(g[k].view(np.uint32), other[k].view(np.uint32)), (f, k)
        assert tuple(g["out"].shape) == (1, h, w, 3)
        planes = dict(hdr=g["accumulated"], variance=g["variance"], length=g["length"], **{k: feat[k] for k in GUIDES})
        # the call made separately, and the model
        assert VM.same_bits(_device(rrt, planes, GUIDES + HISTORY, 5)[0], g["out"]), f
        want = _model(orc, planes, GUIDES + HISTORY, 5)
        assert VM.same_bits(g["out"], want[0]), f
        assert not VM.same_bits(g["out"], g["accumulated"])
        reused += int((g["length"] >= 2.0).sum())
        # denoise=True: mipt_denoise_device on the accumulated frame, as before; denoise=False: the accumulated frame itself
        den = r.denoise(torch.from_numpy(fixed[f]["accumulated"]).cuda(), torch.from_numpy(feat["normal"]).cuda(), torch.from_numpy(feat["depth"]).cuda(),
                        torch.from_numpy(feat["albedo"]).cuda())
        assert D.same_bits(den.cpu().numpy(), fixed[f]["out"]), f
        assert D.same_bits(fixed[f]["out"], D.denoise(orc, fixed[f]["accumulated"], feat["normal"], feat["depth"], feat["albedo"])), f
        assert D.same_bits(plain[f]["out"], plain[f]["accumulated"]), f
    assert reused > 0 and (guided[0]["length"] == 1.0).all()                 # frame 0 is all estimate, later frames mix both sides
    # the filter's own arguments pass through; the fixed filter's are refused by name
    out = next(r.render_sequence(sc, path[:1], denoise="variance", max_history=16.0, iterations=3, sigma_luminance=4.0, short_history=0.0))["out"]
    planes = dict(hdr=guided[0]["accumulated"], variance=guided[0]["variance"], length=guided[0]["length"], **{k: guided[0]["features"][k] for k in GUIDES})
    assert VM.same_bits(out.cpu().numpy(), _model(orc, planes, GUIDES + HISTORY, 3, sigma_luminance=4.0, short_history=0.0)[0])
    with pytest.raises(ValueError):
        next(r.render_sequence(sc, path[:1], denoise="variance", sigma_color=4.0))


def test_render_denoised_with_the_variance_filter(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    sc = _scene(rrt, "cornell")
    size = (61, 37)
    cams = [_moved(rrt, sc.camera), _moved(rrt, sc.camera, dp=(0.3, -0.2, 0.1), dpitch=7.0, dyaw=-11.0)]
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=8, output_image_dimensions=size, output_image_path="/dev/null",
                                             traversal=L.TRAVERSAL_CULLED))
    den, noisy, feat, _ = r.render_denoised(sc, cams, variance=True)
    fixed, noisy2, _, _ = r.render_denoised(sc, cams)
    torch.cuda.synchronize()
    assert torch.equal(noisy.view(torch.int32), noisy2.view(torch.int32))
    planes = dict(hdr=noisy.cpu().numpy(), **{k: v.cpu().numpy() for k, v in feat.items()})
    assert VM.same_bits(den.cpu().numpy(), _model(orc, planes, GUIDES, 5)[0])           # a single frame without history
    assert D.same_bits(fixed.cpu().numpy(), D.denoise(orc, planes["hdr"], planes["normal"], planes["depth"], planes["albedo"]))
    den3 = r.render_denoised(sc, cams, variance=True, iterations=3, short_history=9.0)[0]
    assert VM.same_bits(den3.cpu().numpy(), _model(orc, planes, GUIDES, 3, short_history=9.0)[0])


# ---- refusals: status, a message naming the field, nothing written, and everything works as before ------------------------------------
def test_refusals_leave_everything_as_before(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc = _scene(rrt, "cornell")
    hdr0 = np.zeros((12, 16, 3), dtype=np.float32)
    ro = rrt.make_options(16, 12, 2, 3)
    L.check(lib.mipt_render(sc._handle, L.ptr(sc.camera.uniform), C.byref(ro), L.ptr(hdr0), None, None), "mipt_render")
    size, views = (61, 37), 1
    w, h = size
    n = w * h
    planes = _fields(size, views, seed=6)
    combo = GUIDES + HISTORY
    want = _model(orc, planes, combo, 5)
    assert _same(_device(rrt, planes, combo, 5), want)
    need = n * 48
    t = torch.full((n * 16 + 32,), POISON_I, dtype=torch.int32, device="cuda")
    ws = torch.full((need // 4 + 4,), POISON_I, dtype=torch.int32, device="cuda")
    host = np.full(n * 3, POISON_F, dtype=np.uint32)
    base = t.data_ptr()
    ptr, at = {}, 0
    for k, words in WORDS.items():                                           # 16 bytes between planes
        ptr[k], at = base + at, at + 4 * n * words + 16

    def bufs(**kw):
        b = L.MiptVarianceBuffers()
        for k, v in dict(ptr, **kw).items():
            if k == "reserved":
                b.reserved[v] = base
            else:
                setattr(b, k, v)
        return b

    def opt(**kw):
        o = _opt(L, size, views, 5)
        for k, v in kw.items():
            if k == "reserved":
                o.reserved[v] = 1
            else:
                setattr(o, k, v)
        return o

    def refused(msg, o=None, b=None, workspace=None, nbytes=need):
        o = opt() if o is None else o
        b = bufs() if b is None else b
        rc = lib.mipt_denoise_variance_device(C.byref(o) if o != "null" else None, C.byref(b) if b != "null" else None,
                                              ws.data_ptr() if workspace is None else workspace, nbytes, None)
        err = lib.mipt_last_error().decode()
        assert rc == L.ERR_INVALID_ARG and msg in err and err.startswith("mipt_denoise_variance_device:"), (msg, rc, err)

    inf, nan = float("inf"), float("nan")
    refused("opt", o="null")
    refused("buffers", b="null")
    refused("null hdr", b=bufs(hdr=None))
    refused("null out", b=bufs(out=None))
    refused("null variance", b=bufs(variance=None))
    refused("null length", b=bufs(length=None))
    for kw, msg in [(dict(width=0), "width"), (dict(height=0), "height"), (dict(n_views=0), "n_views"), (dict(width=1 << 16, height=1 << 16), "below 2^32"),
                    (dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(sigma_luminance=0.0), "sigma_luminance"),
                    (dict(sigma_luminance=nan), "sigma_luminance"), (dict(sigma_luminance=inf), "sigma_luminance"), (dict(short_history=-0.5), "short_history"),
                    (dict(short_history=nan), "short_history"), (dict(short_history=inf), "short_history"), (dict(sigma_normal=inf), "sigma_normal"),
                    (dict(sigma_depth=-1.0), "sigma_depth"), (dict(sigma_depth=1e-25), "sigma_depth"), (dict(flags=2), "flags"), (dict(reserved=3), "reserved")]:
        refused(msg, o=opt(**kw))
    refused("reserved buffer pointers", b=bufs(reserved=1))
    refused("normal overlaps hdr", b=bufs(normal=base + 4))
    refused("out overlaps albedo", b=bufs(out=ptr["albedo"]))
    refused("out overlaps hdr", b=bufs(out=base + 12 * n - 4, normal=None))
    refused("variance_out overlaps out", b=bufs(variance_out=ptr["out"] + 8))
    refused("variance_out overlaps variance", b=bufs(variance_out=ptr["variance"]))
    refused("variance_out overlaps hdr", b=bufs(variance_out=ptr["hdr"] + 12 * n - 4))
    refused("length overlaps variance", b=bufs(length=ptr["variance"] + 4))
    refused("null workspace", workspace=0)
    refused("too small", nbytes=need - 16)
    refused("workspace must be 16-byte aligned", workspace=ws.data_ptr() + 8)
    refused("depth must be 4-byte aligned", b=bufs(depth=ptr["depth"] + 1))
    refused("variance_out must be 4-byte aligned", b=bufs(variance_out=ptr["variance_out"] + 2))
    refused("out overlaps the workspace", b=bufs(out=ws.data_ptr() + 32 * n))
    refused("variance_out overlaps the workspace", b=bufs(variance_out=ws.data_ptr() + need - 4))
    assert base % 16 == 0
    refused("hdr overlaps the workspace", workspace=base)
    refused("albedo is not device memory of hdr's device", b=bufs(albedo=host.ctypes.data))
    refused("variance_out is not device memory of hdr's device", b=bufs(variance_out=host.ctypes.data))
    refused("workspace is not device memory of hdr's device", workspace=(host.ctypes.data + 15) & ~15, nbytes=1 << 40)
    refused("hdr is not device memory", b=bufs(hdr=host.ctypes.data))
    assert bool(torch.all(t == POISON_I)) and bool(torch.all(ws == POISON_I)) and np.all(host == POISON_F)      # no refused call wrote anything
    # the host entry refuses the same way
    b = L.MiptVarianceBuffers()
    b.hdr, b.out = host.ctypes.data, host.ctypes.data + 4
    assert lib.mipt_denoise_variance(C.byref(opt()), C.byref(b), 0) == L.ERR_INVALID_ARG and "out overlaps hdr" in lib.mipt_last_error().decode()
    b.out = host.ctypes.data
    assert lib.mipt_denoise_variance(C.byref(opt()), C.byref(b), 1 << 20) == L.ERR_HIP and np.all(host == POISON_F)        # no such device
    # the scene renders and a following call works as before
    hdr1 = np.zeros_like(hdr0)
    L.check(lib.mipt_render(sc._handle, L.ptr(sc.camera.uniform), C.byref(ro), L.ptr(hdr1), None, None), "mipt_render")
    assert np.array_equal(hdr0.view(np.uint32), hdr1.view(np.uint32))
    assert _same(_device(rrt, planes, combo, 5), want) and _same(_host(rrt, planes, combo, 5), want)
