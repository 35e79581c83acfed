"""GPU: mipt_temporal / mipt_temporal_device (csrc/temporal.hip) against the model of tests/tools/temporal_model.py, which
tests/test_temporal_model.py holds to the contract's properties.  Every comparison is bit for bit on uint32 views (a NaN equals a NaN:
its sign and payload are the implementation's): out, length, variance and every byte of history_out.  The frames are the smallest
at which the kernel can go wrong: one pixel, less than a tile, one lane short of and one lane past the 64-pixel tile row, more than
one block both ways; 9 views cross the 8-view launch group.  The synthetic frames look at a small analytic world (three walls, a
floor and windows onto nothing) so that two cameras see consistent positions, normals and materials and the taps are reused; each
model frame is computed once per input."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import denoise_model as D  # noqa: E402
import temporal_model as T  # noqa: E402
import temporal_world as WD  # noqa: E402
from temporal_world import NEAR, NONE, SAME, SEQUENCE  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 2), (5, 5), (63, 5), (65, 9), (61, 37)]
INPUTS = dict(hdr=3, position=3, normal=3, depth=1, material=1, albedo=3)
OUTPUTS = dict(out=3, length=1, variance=1)
WORDS = dict(INPUTS, **OUTPUTS)
POISON_F, POISON_I = 0x7FA5A5A5, 0x25A5A5A5                     # what a word nobody wrote holds (host buffers / int32 tensors)
def _model(cams, planes, history, albedo=True, **opts):
    return T.step(planes["hdr"], planes["position"], planes["normal"], planes["depth"], planes["material"], cams, history,
                  planes["albedo"] if albedo else None, **dict(T.DEFAULTS, **opts))


# ---- the two entries, with guards --------------------------------------------------------------------------------------------------
def _opt(L, size, views, **opts):
    o = L.MiptTemporalOptions()
    o.width, o.height, o.n_views = size[0], size[1], views
    s = dict(T.DEFAULTS, **opts)
    o.alpha_min, o.max_history, o.normal_tol, o.depth_tol = s["alpha_min"], s["max_history"], s["normal_tol"], s["depth_tol"]
    return o


def _host(rrt, cams, planes, history, albedo=True, extras=True, inplace=False, **opts):
    """mipt_temporal on copies of the planes, a sentinel word behind every plane and behind both histories -> dict of results"""
    from rust_ray_tracing_amd import _lib as L
    v, h, w = planes["depth"].shape
    n = v * h * w
    hw = T.history_words(v, h, w)
    b, keep = L.MiptTemporalBuffers(), {}
    for k in INPUTS:
        if k == "albedo" and not albedo:
            continue
        keep[k] = np.concatenate([planes[k].reshape(-1).view(np.uint32), [POISON_F]]).astype(np.uint32)
        setattr(b, k, keep[k].ctypes.data)
    outs = {k: np.full(n * words + 1, POISON_F, dtype=np.uint32) for k, words in OUTPUTS.items() if k == "out" or extras}
    if inplace:
        outs["out"] = keep["hdr"]
    for k, a in outs.items():
        setattr(b, k, a.ctypes.data)
    new = np.full(hw + 1, POISON_F, dtype=np.uint32)
    b.history_out = new.ctypes.data
    if history is not None:
        old = np.concatenate([history, [POISON_F]]).astype(np.uint32)
        b.history_in = old.ctypes.data
    table = np.ascontiguousarray(cams)
    rc = rrt.load().mipt_temporal(C.byref(_opt(L, (w, h), v, **opts)), L.ptr(table), C.byref(b), 0)
    assert rc == 0, (rc, rrt.load().mipt_last_error())
    for k, a in keep.items():
        assert a[-1] == POISON_F, k
        if not (inplace and k == "hdr"):
            assert np.array_equal(a[:-1], planes[k].reshape(-1).view(np.uint32)), k           # an input is not written
    if history is not None:
        assert np.array_equal(old[:-1], history) and old[-1] == POISON_F
    assert new[-1] == POISON_F and all(a[-1] == POISON_F for a in outs.values())
    res = dict(history=new[:-1].copy(), out=outs["out"][:-1].view(np.float32).reshape(v, h, w, 3))
    if extras:
        res.update(length=outs["length"][:-1].view(np.float32).reshape(v, h, w), variance=outs["variance"][:-1].view(np.float32).reshape(v, h, w))
    return res


def _device(rrt, cams, planes, history, albedo=True, extras=True, inplace=False, stream=None, **opts):
    """mipt_temporal_device: all planes and both histories are slices of one tensor, a plane that is not passed holds poison and must
    keep it; a sentinel word behind every plane and behind each history's declared size -> dict of results"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    v, h, w = planes["depth"].shape
    n = v * h * w
    hw = T.history_words(v, h, w)
    assert lib.mipt_temporal_history_bytes(w, h, v) == 4 * hw
    off, total = {}, 0
    for k, words in WORDS.items():
        off[k], total = total, total + n * words + 1
    for k in ("history_in", "history_out"):
        total = (total + 3) & ~3                                           # 16-byte aligned
        off[k], total = total, total + hw + 1
    host = np.full(total, POISON_I, dtype=np.uint32)
    passed = [k for k in INPUTS if albedo or k != "albedo"]
    for k in passed:
        host[off[k]: off[k] + n * WORDS[k]] = planes[k].reshape(-1).view(np.uint32)
    if history is not None:
        host[off["history_in"]: off["history_in"] + hw] = history
    before = host.copy()
    t = torch.from_numpy(host.view(np.int32)).cuda()
    assert t.data_ptr() % 16 == 0
    b = L.MiptTemporalBuffers()
    for k in passed:
        setattr(b, k, t.data_ptr() + 4 * off[k])
    written = {"out": "hdr" if inplace else "out"}
    if extras:
        written.update(length="length", variance="variance")
    for k, where in written.items():
        setattr(b, k, t.data_ptr() + 4 * off[where])
    b.history_out = t.data_ptr() + 4 * off["history_out"]
    if history is not None:
        b.history_in = t.data_ptr() + 4 * off["history_in"]
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()                                                # the fills above ran on torch's current stream, which need not be `stream`
    table = np.array(cams, copy=True)
    rc = lib.mipt_temporal_device(C.byref(_opt(L, (w, h), v, **opts)), L.ptr(table), C.byref(b), stream)
    table[...] = np.zeros((), dtype=table.dtype)                            # the camera table may be freed on return
    assert rc == 0, (rc, lib.mipt_last_error())
    torch.cuda.synchronize()
    got = t.cpu().numpy().view(np.uint32)
    targets = set(written.values()) | {"history_out"}
    for k in off:
        size = hw if k.startswith("history") else n * WORDS[k]
        lo, hi = off[k], off[k] + size
        assert got[hi] == POISON_I, k                                      # nothing is written behind a plane or a history's declared size
        if k not in targets:
            assert np.array_equal(got[lo:hi], before[lo:hi]), k            # inputs, and a plane that was not passed, are untouched
    res = {k: got[off[where]: off[where] + n * WORDS[k]].view(np.float32).reshape((v, h, w, 3) if WORDS[k] == 3 else (v, h, w)) for k, where in written.items()}
    res["history"] = got[off["history_out"]: off["history_out"] + hw].copy()
    return res


def _same(got, want, shape, what):
    v, h, w = shape
    assert T.same_bits(got["out"], want["out"]), (what, "out", int((got["out"].view(np.uint32) != want["out"].view(np.uint32)).sum()))
    for k in ("length", "variance"):
        if k in got:
            assert T.same_bits(got[k], want[k]), (what, k)
    assert T.same_history(got["history"], want["history"], v, h, w), (what, "history")


# ---- sizes x views x frames x entries x albedo x optional outputs --------------------------------------------------------------------
@pytest.mark.parametrize("views", [1, 3, 9])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_sequences_against_the_model(rrt, size, views):
    """first frame, same camera, a translated and yawed camera, a camera turned far away: each frame from the model's history of the
    frame before, so that every call stands alone"""
    w, h = size
    results = []
    for albedo in (True, False):
        history = None
        for f, move in enumerate(SEQUENCE):
            cams, planes = WD.frame(size, views, move, seed=f)
            want = _model(cams, planes, history, albedo)
            results.append(want)
            for entry in (_host, _device):
                for extras in (True, False):
                    _same(entry(rrt, cams, planes, history, albedo, extras), want, (views, h, w), (size, views, f, albedo, entry.__name__, extras))
            history = want["history"]
    if size == (61, 37):                                                    # the moved cameras put a pixel into every class
        seen = T.classes_present(results)
        assert seen == T.ALL_CLASSES, T.ALL_CLASSES - seen


def test_three_chained_frames_feed_the_gpus_own_history_back(rrt):
    size, views = (65, 9), 3
    for entry in (_host, _device):
        theirs = ours = None
        for f, move in enumerate((SAME, NEAR, NEAR, SAME)):
            cams, planes = WD.frame(size, views, move, seed=10 + f)
            want = _model(cams, planes, ours, max_history=3.0, alpha_min=0.2)
            got = entry(rrt, cams, planes, theirs, max_history=3.0, alpha_min=0.2)
            _same(got, want, (views, size[1], size[0]), (entry.__name__, f))
            theirs, ours = got["history"], want["history"]
        assert float(want["length"].max()) == 3.0 and (want["cls"] >= T.REUSED4).sum() > 0.5 * want["cls"].size


def test_options_reach_the_kernel(rrt):
    size, views = (61, 37), 1
    cams0, planes0 = WD.frame(size, views, SAME)
    history = _model(cams0, planes0, None)["history"]
    history = _model(cams0, planes0, history)["history"]                   # lengths of 2: the cap and the floor both bind below
    cams, planes = WD.frame(size, views, NEAR, seed=2)
    base = _model(cams, planes, history)
    for opts in (dict(alpha_min=0.75), dict(max_history=1.5), dict(normal_tol=0.0005), dict(depth_tol=0.002), dict(normal_tol=0.0, depth_tol=0.0),
                 dict(alpha_min=1.0, max_history=1.0)):
        want = _model(cams, planes, history, **opts)
        assert not T.same_history(want["history"], base["history"], views, size[1], size[0]), opts
        for entry in (_host, _device):
            _same(entry(rrt, cams, planes, history, **opts), want, (views, size[1], size[0]), (opts, entry.__name__))


@pytest.mark.parametrize("entry", ["host", "device"])
def test_special_values_and_out_may_be_hdr(rrt, entry):
    """a synthetic history with +-inf and NaN colour, a NaN normal, a NaN length and misses beside hits; zero, negative and NaN
    albedo, NaN and infinite positions and depths in the frame: the NaN rule of the header, also in place"""
    f = _host if entry == "host" else _device
    size, views = (61, 37), 1
    w, h = size
    cams0, planes0 = WD.frame(size, views, SAME)
    history = _model(cams0, planes0, None)["history"].copy()
    _, p0, p1, p2 = T.unpack_history(history, views, h, w)
    p0[0, 5, 7, 1], p0[0, 6, 30, 0], p0[0, 30, 50, :3], p0[0, 20, 3, 3] = np.inf, -np.inf, np.nan, np.nan
    p1[0, 25, 25, 0], p1[0, 12, 12, 3] = np.nan, np.nan
    p1[0, 15:18, 30:33, 3], p2[0, 15:18, 30:33, 2] = 1e30, NONE           # a patch of misses in the history
    p2[0, 8, 40, 0], p2[0, 9, 41, 1] = np.float32(np.nan).view(np.uint32), np.float32(np.inf).view(np.uint32)
    cams, planes = WD.frame(size, views, NEAR, seed=3)
    planes = {k: a.copy() for k, a in planes.items()}
    planes["albedo"][0, 10, 10] = 0.0
    planes["albedo"][0, 11, 40, 0] = np.nan
    planes["albedo"][0, 12, 41, 2] = -0.5
    planes["albedo"][0, 2, 2] = np.float32(1.0 / 256.0)                     # the floor itself: the comparison is strict
    planes["hdr"][0, 3, 3, 1], planes["hdr"][0, 4, 4] = np.inf, np.nan
    planes["position"][0, 18, 18, 0], planes["position"][0, 19, 19, 2], planes["position"][0, 21, 21, 1] = np.nan, np.inf, -np.inf
    planes["depth"][0, 22, 22], planes["depth"][0, 23, 23] = np.nan, np.inf
    planes["normal"][0, 24, 24, 2] = np.nan
    for albedo in (True, False):
        want = _model(cams, planes, history, albedo)
        assert np.isnan(want["out"]).any() and np.isfinite(want["out"]).sum() > want["out"].size * 0.9
        assert (want["cls"] >= T.REUSED4).sum() > 0.3 * w * h
        for inplace in (False, True):
            _same(f(rrt, cams, planes, history, albedo, inplace=inplace), want, (views, h, w), (albedo, inplace))
    # out == hdr on more than one view and on the first frame
    cams, planes = WD.frame((65, 9), 3, NEAR, seed=4)
    _same(f(rrt, cams, planes, None, inplace=True), _model(cams, planes, None), (3, 9, 65), "first frame in place")


def test_many_tiny_views(rrt):
    """700 views of 3x2: 88 launch groups, the last of four views, and the (view, tile) decode far past one block"""
    size, views = (3, 2), 700
    cams0, planes0 = WD.frame(size, views, SAME)
    history = _model(cams0, planes0, None)["history"]
    cams, planes = WD.frame(size, views, NEAR, seed=5)
    want = _model(cams, planes, history)
    _same(_device(rrt, cams, planes, history), want, (views, 2, 3), "700 views")
    rec, _, _, _ = T.unpack_history(want["history"], views, 2, 3)
    assert T.same_bits(rec[699], T.camera_record(cams[699])) and not T.same_bits(rec[699], rec[698])
    assert (want["cls"] >= T.REUSED4).any()


def test_torch_tensors_on_a_side_stream(rrt):
    import torch
    size, views = (65, 9), 3
    w, h = size
    cams0, planes0 = WD.frame(size, views, SAME)
    first = _model(cams0, planes0, None)
    cams, planes = WD.frame(size, views, NEAR, seed=6)
    want = _model(cams, planes, first["history"])
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=1, output_image_dimensions=size, output_image_path="/dev/null"))
    dev0 = {k: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for k, a in planes0.items()}
    dev = {k: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for k, a in planes.items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = torch.ones((1 << 22,), device="cuda").cumsum(0)               # work in front of the launches on the side stream
        out0, hist0, _ = r.temporal(dev0["hdr"], dev0, cams0)                                     # torch's current stream
        out1, hist1, ex1 = r.temporal(dev["hdr"], dev, cams, history=hist0, want_length=True, want_variance=True)
    out2, hist2, ex2 = r.temporal(dev["hdr"], dev, list(cams), history=hist0, stream=side, want_length=True)   # the one given
    c = _device(rrt, cams, planes, first["history"], stream=side.cuda_stream)
    side.synchronize()
    assert busy[-1].item() == float(1 << 22)
    assert out1.is_cuda and tuple(out1.shape) == planes["hdr"].shape and hist1.dtype == torch.int32 and set(ex1) == {"length", "variance"} and set(ex2) == {"length"}
    _same(dict(out=out0.cpu().numpy(), history=hist0.cpu().numpy().view(np.uint32)), first, (views, h, w), "first")
    for out, hist, ex in ((out1, hist1, ex1), (out2, hist2, ex2)):
        got = dict(out=out.cpu().numpy(), history=hist.cpu().numpy().view(np.uint32), **{k: t.cpu().numpy() for k, t in ex.items()})
        _same(got, want, (views, h, w), "torch")
    _same(c, want, (views, h, w), "raw stream")
    for k, t in dev.items():
        assert np.array_equal(t.cpu().numpy().view(np.uint32), planes[k].view(np.uint32)), k       # the inputs are not written
    # numpy arrays and a single view through Renderer.temporal
    one = {k: a[1] for k, a in planes.items()}
    out, hist, ex = r.temporal(one["hdr"], one, cams[1:2], want_variance=True)
    want1 = _model(cams[1:2], {k: a[1:2] for k, a in planes.items()}, None)
    assert isinstance(out, np.ndarray) and out.shape == (h, w, 3) and hist.dtype == np.uint32 and set(ex) == {"variance"}
    _same(dict(out=out[None], history=hist, variance=ex["variance"][None]), want1, (1, h, w), "numpy")


# ---- real frames: render_sequence is the four calls and the model, step by step -------------------------------------------------------
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
def test_render_sequence_is_the_four_calls_and_the_model(rrt, orc, kind, size, spp):
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc = _scene(rrt, kind)
    w, h = size
    # the frame before the scene's camera comes from T.COVERAGE_MOVE; then a small move
    path = [[_moved(rrt, sc.camera, **T.COVERAGE_MOVE)], [_moved(rrt, sc.camera)], [_moved(rrt, sc.camera, dp=(0.02, 0.0, 0.01), dyaw=0.4)]]
    r = rrt.Renderer.new(rrt.RendererOptions(samples=spp, max_ray_depth=8, output_image_dimensions=size, output_image_path="/dev/null",
                                             seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED))
    one = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=8, output_image_dimensions=size, output_image_path="/dev/null",
                                               seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED))
    frames = []
    for fr in r.render_sequence(sc, path, max_history=16.0):
        torch.cuda.synchronize()
        assert tuple(fr["out"].shape) == (1, h, w, 3) and fr["out"].is_cuda and fr["stats"]["pixels"] == w * h
        frames.append({k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in fr.items() if k != "features"})
        frames[-1]["features"] = {k: v.cpu().numpy() for k, v in fr["features"].items()}
        frames[-1]["history"] = frames[-1]["history"].view(np.uint32)      # the two history tensors are reused: copied here
    assert [fr["frame"] for fr in frames] == [0, 1, 2]
    history, results = None, []
    stream = torch.cuda.current_stream().cuda_stream
    for f, fr in enumerate(frames):
        cams = np.stack([c.uniform for c in path[f]])
        # the four calls made separately
        opt = rrt.make_options(w, h, spp, 8, seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED, sample_begin=1 + f * spp)
        hdr = torch.zeros((1, h, w, 3), dtype=torch.float32, device="cuda")
        assert lib.mipt_render_batch_device(sc._handle, L.ptr(cams), 1, C.byref(opt), hdr.data_ptr(), None, stream, None) == 0
        assert np.array_equal(hdr.cpu().numpy().view(np.uint32), fr["noisy"].view(np.uint32)), f
        sep, _ = one.render_features(sc, path[f], ("depth", "normal", "albedo", "position", "material"), device=True)
        feat = fr["features"]
        assert set(feat) == set(sep)
        for k in sep:
            assert np.array_equal(sep[k].cpu().numpy().view(np.uint32), feat[k].view(np.uint32)), (f, k)
        planes = dict(hdr=fr["noisy"], **{k: feat[k] for k in ("position", "normal", "depth", "albedo")}, material=feat["material"].view(np.uint32))
        got = dict(out=fr["accumulated"], history=fr["history"], length=fr["length"], variance=fr["variance"])
        _same(_device(rrt, cams, planes, history, max_history=16.0), got, (1, h, w), (f, "separate call"))
        den = r.denoise(torch.from_numpy(fr["accumulated"]).cuda(), sep["normal"], sep["depth"], sep["albedo"])
        assert D.same_bits(den.cpu().numpy(), fr["out"]), f
        # and the model, applied to the buffers the GPU produced
        want = _model(cams, planes, history, max_history=16.0)
        results.append(want)
        _same(got, want, (1, h, w), (f, "model"))
        assert D.same_bits(fr["out"], D.denoise(orc, fr["accumulated"], feat["normal"], feat["depth"], feat["albedo"])), f
        history = want["history"]
    hits = int((frames[2]["features"]["depth"] < T.MISS).sum())               # the Cornell box fills a ninth of this frame
    assert (results[2]["cls"] >= T.REUSED4).sum() > 0.6 * hits and float(results[2]["length"].max()) > 2.5
    if kind == "atrium":                                                    # the moved camera puts a pixel into every class
        seen = T.classes_present(results)
        assert seen == T.ALL_CLASSES, T.ALL_CLASSES - seen
    # without the filter the accumulated frame itself comes out; the pixel stream is refused
    plain = [fr["out"].cpu().numpy() for fr in r.render_sequence(sc, path[:2], denoise=False, max_history=16.0)]
    assert D.same_bits(plain[1], frames[1]["accumulated"])
    stream_seeds = rrt.Renderer.new(rrt.RendererOptions(samples=spp, max_ray_depth=8, output_image_dimensions=size, output_image_path="/dev/null"))
    with pytest.raises(ValueError):
        next(stream_seeds.render_sequence(sc, path))


# ---- refusals: status, a message naming the field, nothing written, and everything works as before ------------------------------------
def test_refusals_leave_everything_as_before(rrt):
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
    cams0, planes0 = WD.frame(size, views, SAME)
    history = _model(cams0, planes0, None)["history"]
    cams, planes = WD.frame(size, views, NEAR, seed=7)
    want = _model(cams, planes, history)
    _same(_device(rrt, cams, planes, history), want, (views, h, w), "before")
    hw = T.history_words(views, h, w)
    gap = 4                                                                  # words between planes: 16 bytes
    off, total = {}, 0
    for k, words in list(WORDS.items()) + [("history_in", None), ("history_out", None)]:
        total = (total + 3) & ~3
        off[k], total = total, total + (hw if words is None else n * words) + gap
    t = torch.full((total,), POISON_I, dtype=torch.int32, device="cuda")
    host = np.full(hw + 4, POISON_F, dtype=np.uint32)
    base = t.data_ptr()
    assert base % 16 == 0
    ptr = {k: base + 4 * o for k, o in off.items()}
    table = np.ascontiguousarray(cams)

    def bufs(**kw):
        b = L.MiptTemporalBuffers()
        for k, v in dict(ptr, **kw).items():
            if k == "reserved":
                b.reserved[v] = base
            else:
                setattr(b, k, v)
        return b

    def opt(**kw):
        o = _opt(L, size, views)
        for k, v in kw.items():
            if k == "reserved":
                o.reserved[v] = 1
            else:
                setattr(o, k, v)
        return o

    def refused(msg, o=None, b=None, c=table):
        o = opt() if o is None else o
        b = bufs() if b is None else b
        rc = lib.mipt_temporal_device(C.byref(o) if o != "null" else None, L.ptr(c) if c is not None else None, C.byref(b) if b != "null" else None, None)
        err = lib.mipt_last_error().decode()
        assert rc == L.ERR_INVALID_ARG and msg in err and err.startswith("mipt_temporal_device:"), (msg, rc, err)

    inf, nan = float("inf"), float("nan")
    refused("opt", o="null")
    refused("cameras", c=None)
    refused("buffers", b="null")
    for k in ("hdr", "position", "normal", "depth", "material", "history_out", "out"):
        refused(f"null {k}", b=bufs(**{k: None}))
    for kw, msg in [(dict(width=0), "width"), (dict(height=0), "height"), (dict(n_views=0), "n_views"), (dict(width=1 << 16, height=1 << 16), "below 2^32"),
                    (dict(flags=2), "flags"), (dict(reserved=3), "reserved"), (dict(alpha_min=-0.5), "alpha_min"), (dict(alpha_min=nan), "alpha_min"),
                    (dict(max_history=0.0), "max_history"), (dict(max_history=inf), "max_history"), (dict(normal_tol=-1.0), "normal_tol"),
                    (dict(normal_tol=nan), "normal_tol"), (dict(depth_tol=inf), "depth_tol"), (dict(depth_tol=-0.0001), "depth_tol")]:
        refused(msg, o=opt(**kw))
    singular = table.copy()
    singular[0]["look_at"][1] = singular[0]["look_at"][0]
    refused("cameras[0].look_at", c=singular)
    refused("reserved buffer pointers", b=bufs(reserved=1))
    refused("normal overlaps hdr", b=bufs(normal=base + 4))
    refused("out overlaps albedo", b=bufs(out=ptr["albedo"]))
    refused("out overlaps hdr", b=bufs(out=ptr["hdr"] + 12 * n - 4))
    refused("history_out overlaps history_in", b=bufs(history_out=ptr["history_in"]))
    refused("history_out overlaps history_in", b=bufs(history_out=ptr["history_in"] + 4 * hw - 16))
    refused("length overlaps history_in", b=bufs(length=ptr["history_in"] + 64))
    refused("variance overlaps out", b=bufs(variance=ptr["out"]))
    refused("depth must be 4-byte aligned", b=bufs(depth=ptr["depth"] + 1))
    refused("history_in must be 16-byte aligned", b=bufs(history_in=ptr["history_in"] + 4))
    refused("history_out must be 16-byte aligned", b=bufs(history_out=ptr["history_out"] + 8))
    refused("albedo is not device memory of hdr's device", b=bufs(albedo=host.ctypes.data))
    refused("history_in is not device memory of hdr's device", b=bufs(history_in=(host.ctypes.data + 15) & ~15))
    refused("hdr is not device memory", b=bufs(hdr=host.ctypes.data))
    assert bool(torch.all(t == POISON_I)) and np.all(host == POISON_F)      # no refused call wrote anything
    # the host entry refuses the same way
    b = L.MiptTemporalBuffers()
    keep = {k: np.full(n * words + 1, POISON_F, dtype=np.uint32) for k, words in WORDS.items()}
    keep["history_out"] = np.full(hw, POISON_F, dtype=np.uint32)
    for k, a in keep.items():
        setattr(b, k, a.ctypes.data)
    b.out = keep["hdr"].ctypes.data + 4
    assert lib.mipt_temporal(C.byref(opt()), L.ptr(table), C.byref(b), 0) == L.ERR_INVALID_ARG and "out overlaps hdr" in lib.mipt_last_error().decode()
    b.out = keep["hdr"].ctypes.data
    assert lib.mipt_temporal(C.byref(opt()), L.ptr(table), C.byref(b), 1 << 20) == L.ERR_HIP            # no such device
    assert all(np.all(a == POISON_F) for a in keep.values())
    # the scene renders and a following temporal call works as before
    hdr1 = np.zeros_like(hdr0)
    L.check(lib.mipt_render(sc._handle, L.ptr(sc.camera.uniform), C.byref(ro), L.ptr(hdr1), None, None), "mipt_render")
    assert np.array_equal(hdr0.view(np.uint32), hdr1.view(np.uint32))
    _same(_device(rrt, cams, planes, history), want, (views, h, w), "after")
    _same(_host(rrt, cams, planes, history), want, (views, h, w), "after, host")
