"""GPU: mipt_temporal_counts / mipt_temporal_counts_device (csrc/temporal.hip, the COUNTS kernels) against the model of
tests/tools/temporal_counts_model.py, which tests/test_temporal_counts_model.py holds to the contract.  Every comparison is bit for
bit on uint32 views (a NaN equals a NaN): out, length, variance and every byte of history_out, over two frames of temporal_world's
moving camera.  Sizes: one pixel; less than a tile; 70x9, ragged against the 64x4 tile both ways and more than one block; 9 views,
past the 8-view launch group.  Outputs start as poison with a guard word behind every plane; hdr holds NaN wherever the count is 0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import temporal_counts_model as TC  # noqa: E402
import temporal_model as T  # noqa: E402
import temporal_world as WD  # noqa: E402
from temporal_world import NEAR, SAME  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [((1, 1), 1), ((7, 5), 3), ((70, 9), 2), ((5, 3), 9)]           # (W, H), views
INPUTS = dict(hdr=3, position=3, normal=3, depth=1, material=1, albedo=3, counts=1)
OUTPUTS = dict(out=3, length=1, variance=1)
WORDS = dict(INPUTS, **OUTPUTS)
POISON_F, POISON_I = 0x7FA5A5A5, 0x25A5A5A5
CAP = 5


def _counts(shape, seed):
    """counts from {0, 1, 2, 3, 5, 9} (9 is past the cap of 5), a tile of zeros in the first view's corner"""
    rng = np.random.default_rng(seed)
    c = rng.choice(np.array([0, 1, 2, 3, 5, 9], dtype=np.uint32), size=shape).astype(np.uint32)
    c[0, : max(1, shape[1] // 2), : max(1, shape[2] // 3)] = 0
    c.reshape(-1)[-1] = 9 if c.size > 1 else (0 if seed & 1 else 3)         # a single pixel: traced in the first frame, not in the second
    return np.ascontiguousarray(c)


def _frame(size, views, f):
    """frame f of the sequence: cameras, planes with NaN in hdr under the zero counts, the counts"""
    cams, planes = WD.frame(size, views, (SAME, NEAR)[f], seed=20 + f)
    counts = _counts(planes["depth"].shape, 7 * size[0] + views + f)
    planes = dict(planes, hdr=np.where((counts == 0)[..., None], np.float32(np.nan), planes["hdr"]).astype(np.float32), counts=counts)
    return cams, planes


def _model(cams, p, history, albedo=True, counts=None, **opts):
    o = dict(T.DEFAULTS, **opts)
    if counts is None:
        return T.step(p["hdr"], p["position"], p["normal"], p["depth"], p["material"], cams, history, p["albedo"] if albedo else None, **o)
    return TC.step(p["hdr"], p["position"], p["normal"], p["depth"], p["material"], cams, counts, CAP, history, p["albedo"] if albedo else None, **o)


def _opt(L, size, views, **opts):
    o = L.MiptTemporalOptions()
    o.width, o.height, o.n_views = size[0], size[1], views
    s = dict(T.DEFAULTS, **opts)
    o.alpha_min, o.max_history, o.normal_tol, o.depth_tol = s["alpha_min"], s["max_history"], s["normal_tol"], s["depth_tol"]
    return o


def _host(rrt, cams, planes, history, albedo=True, counted=True, **opts):
    """the host entry on copies of the planes, a sentinel word behind every plane and both histories -> dict of results"""
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    v, h, w = planes["depth"].shape
    n, hw = v * h * w, T.history_words(v, h, w)
    b, keep = L.MiptTemporalBuffers(), {}
    for k in INPUTS:
        if k == "albedo" and not albedo:
            continue
        keep[k] = np.concatenate([planes[k].reshape(-1).view(np.uint32), [POISON_F]]).astype(np.uint32)
        if k != "counts":
            setattr(b, k, keep[k].ctypes.data)
    outs = {k: np.full(n * words + 1, POISON_F, dtype=np.uint32) for k, words in OUTPUTS.items()}
    for k, a in outs.items():
        setattr(b, k, a.ctypes.data)
    new = np.full(hw + 1, POISON_F, dtype=np.uint32)
    b.history_out = new.ctypes.data
    if history is not None:
        old = np.concatenate([history, [POISON_F]]).astype(np.uint32)
        b.history_in = old.ctypes.data
    table = np.ascontiguousarray(cams)
    o = _opt(L, (w, h), v, **opts)
    if counted:
        rc = lib.mipt_temporal_counts(C.byref(o), L.ptr(table), C.byref(b), C.c_void_p(keep["counts"].ctypes.data), CAP, 0)
    else:
        rc = lib.mipt_temporal(C.byref(o), L.ptr(table), C.byref(b), 0)
    assert rc == 0, (rc, lib.mipt_last_error())
    for k, a in keep.items():
        assert a[-1] == POISON_F and np.array_equal(a[:-1], planes[k].reshape(-1).view(np.uint32)), k      # an input is not written
    if history is not None:
        assert np.array_equal(old[:-1], history) and old[-1] == POISON_F
    assert new[-1] == POISON_F and all(a[-1] == POISON_F for a in outs.values())
    return dict(history=new[:-1].copy(), out=outs["out"][:-1].view(np.float32).reshape(v, h, w, 3),
                length=outs["length"][:-1].view(np.float32).reshape(v, h, w), variance=outs["variance"][:-1].view(np.float32).reshape(v, h, w))


def _device(rrt, cams, planes, history, albedo=True, counted=True, **opts):
    """the device entry: all planes and both histories are slices of one tensor of poison, a sentinel word behind every plane and
    behind each history's declared size; what is not an output must come back as it went in"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    v, h, w = planes["depth"].shape
    n, hw = v * h * w, T.history_words(v, h, w)
    off, total = {}, 0
    for k, words in WORDS.items():
        off[k], total = total, total + n * words + 1
    for k in ("history_in", "history_out"):
        total = (total + 3) & ~3                                           # 16-byte aligned
        off[k], total = total, total + hw + 1
    host = np.full(total, POISON_I, dtype=np.uint32)
    passed = [k for k in INPUTS if (albedo or k != "albedo") and (counted or k != "counts")]
    for k in passed:
        host[off[k]: off[k] + n * WORDS[k]] = planes[k].reshape(-1).view(np.uint32)
    if history is not None:
        host[off["history_in"]: off["history_in"] + hw] = history
    before = host.copy()
    t = torch.from_numpy(host.view(np.int32)).cuda()
    assert t.data_ptr() % 16 == 0
    b = L.MiptTemporalBuffers()
    for k in passed:
        if k != "counts":
            setattr(b, k, t.data_ptr() + 4 * off[k])
    for k in OUTPUTS:
        setattr(b, k, t.data_ptr() + 4 * off[k])
    b.history_out = t.data_ptr() + 4 * off["history_out"]
    if history is not None:
        b.history_in = t.data_ptr() + 4 * off["history_in"]
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    table = np.array(cams, copy=True)
    o = _opt(L, (w, h), v, **opts)
    if counted:
        rc = lib.mipt_temporal_counts_device(C.byref(o), L.ptr(table), C.byref(b), C.c_void_p(t.data_ptr() + 4 * off["counts"]), CAP, stream)
    else:
        rc = lib.mipt_temporal_device(C.byref(o), L.ptr(table), C.byref(b), stream)
    assert rc == 0, (rc, lib.mipt_last_error())
    torch.cuda.synchronize()
    got = t.cpu().numpy().view(np.uint32)
    targets = set(OUTPUTS) | {"history_out"}
    for k in off:
        size = hw if k.startswith("history") else n * WORDS[k]
        lo, hi = off[k], off[k] + size
        assert got[hi] == POISON_I, k
        if k not in targets:
            assert np.array_equal(got[lo:hi], before[lo:hi]), k
    res = {k: got[off[k]: off[k] + n * WORDS[k]].view(np.float32).reshape((v, h, w, 3) if WORDS[k] == 3 else (v, h, w)) for k in OUTPUTS}
    res["history"] = got[off["history_out"]: off["history_out"] + hw].copy()
    return res


def _same(got, want, shape, what):
    v, h, w = shape
    for k in ("out", "length", "variance"):
        assert T.same_bits(got[k], want[k]), (what, k, int((got[k].view(np.uint32) != want[k].view(np.uint32)).sum()))
    assert T.same_history(got["history"], want["history"], v, h, w), (what, "history")


@pytest.mark.parametrize("albedo", [True, False], ids=["albedo", "plain"])
@pytest.mark.parametrize("size,views", CASES, ids=[f"{w}x{h}x{v}" for (w, h), v in CASES])
def test_two_frames_against_the_model(rrt, size, views, albedo):
    """the first frame (no history: every traced pixel starts with its own count, every other with nothing) and a second one through a
    moved camera, from the model's history of the first so that each call stands alone; both entries"""
    w, h = size
    history = None
    for f in (0, 1):
        cams, p = _frame(size, views, f)
        want = _model(cams, p, history, albedo, counts=p["counts"])
        zero = p["counts"] == 0
        assert (zero.any() or (size == (1, 1) and f == 0)) and not np.isnan(want["out"][zero]).any()   # the NaN under the zeros reaches nothing
        for entry in (_host, _device):
            _same(entry(rrt, cams, p, history, albedo), want, (views, h, w), (size, views, f, albedo, entry.__name__))
        if f == 1 and size == (70, 9):                                      # conditions on the input: every branch of the new code is reached
            reuse, n = want["reuse"], np.minimum(p["counts"], CAP)
            assert (reuse & (n == 0)).sum() > 20 and (reuse & (n > 0)).sum() > 100 and (~reuse & (n == 0)).sum() > 0
            assert ((want["taps"] > 0) & (want["taps"] < 4) & reuse).any() and float(want["length"].max()) > CAP
        history = want["history"]


def test_options_reach_the_counting_kernel(rrt):
    """max_history below one frame's samples (al stops at 1, the length at the cap) and a floor on the blend factor"""
    size, views = (70, 9), 2
    cams0, p0 = _frame(size, views, 0)
    cams, p = _frame(size, views, 1)
    history = _model(cams0, p0, None, counts=p0["counts"])["history"]
    base = _model(cams, p, history, counts=p["counts"])
    for opts in (dict(max_history=2.5), dict(alpha_min=0.9), dict(max_history=1.0, alpha_min=1.0)):
        want = _model(cams, p, history, counts=p["counts"], **opts)
        assert not T.same_history(want["history"], base["history"], views, size[1], size[0]), opts
        for entry in (_host, _device):
            _same(entry(rrt, cams, p, history, **opts), want, (views, size[1], size[0]), (opts, entry.__name__))


def test_a_plane_of_ones_is_mipt_temporal_and_the_plain_entry_is_untouched(rrt):
    """consequence (a) on the GPU's own bytes, consequence (b) by feeding each entry the other's history, and mipt_temporal_device
    before and after calls of the new entry"""
    size, views = (70, 9), 2
    w, h = size
    cams0, p0 = WD.frame(size, views, SAME, seed=30)
    cams, p = WD.frame(size, views, NEAR, seed=31)
    ones = np.ones((views, h, w), dtype=np.uint32)
    first = _device(rrt, cams0, p0, None, counted=False)
    before = _device(rrt, cams, p, first["history"], counted=False)
    _same(before, _model(cams, p, first["history"]), (views, h, w), "plain entry against its model")
    for albedo in (True, False):
        plain0 = _device(rrt, cams0, p0, None, albedo, counted=False)
        ones0 = _device(rrt, cams0, dict(p0, counts=ones), None, albedo)
        _same(ones0, plain0, (views, h, w), ("first frame", albedo))
        plain1 = _device(rrt, cams, p, plain0["history"], albedo, counted=False)
        _same(_device(rrt, cams, dict(p, counts=ones), ones0["history"], albedo), plain1, (views, h, w), ("second frame", albedo))
        _same(_host(rrt, cams, dict(p, counts=ones), plain0["history"], albedo), plain1, (views, h, w), ("second frame, host", albedo))
    # a history counted in samples, read by the plain entry and by the counting one
    counted = _device(rrt, cams0, dict(p0, counts=_counts((views, h, w), 5)), None)
    _same(_device(rrt, cams, p, counted["history"], counted=False), _model(cams, p, counted["history"]), (views, h, w), "plain after counted")
    after = _device(rrt, cams, p, first["history"], counted=False)
    _same(after, before, (views, h, w), "plain entry after the counting one")


def test_renderer_mirror(rrt):
    import torch
    size, views = (70, 9), 2
    w, h = size
    cams0, p0 = _frame(size, views, 0)
    cams, p = _frame(size, views, 1)
    first = _model(cams0, p0, None, counts=p0["counts"])
    want = _model(cams, p, first["history"], counts=p["counts"])
    r = rrt.Renderer.new(rrt.RendererOptions(samples=CAP, max_ray_depth=1, output_image_dimensions=size, output_image_path="/dev/null"))
    out, hist, ex = r.temporal(p["hdr"], p, cams, history=first["history"], want_length=True, want_variance=True, counts=p["counts"])
    _same(dict(out=out, history=hist, **ex), want, (views, h, w), "numpy, the cap from options.samples")
    dev = {k: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for k, a in p.items()}
    out, hist, ex = r.temporal(dev["hdr"], dev, cams, history=torch.from_numpy(first["history"].view(np.int32)).cuda(), want_length=True,
                               want_variance=True, counts=dev["counts"], samples_cap=CAP)
    torch.cuda.synchronize()
    _same(dict(out=out.cpu().numpy(), history=hist.cpu().numpy().view(np.uint32), **{k: t.cpu().numpy() for k, t in ex.items()}), want,
          (views, h, w), "tensors")
