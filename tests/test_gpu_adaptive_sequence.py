"""-m gpu: render_sequence(adaptive=...) -- every frame's counts are the sample map of the frame before, as the model makes it from
the planes the run itself produced; every frame's trace is render_adaptive with those counts; adaptive=None is the call sequence of
before."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import sample_map_model as SM  # noqa: E402

pytestmark = pytest.mark.gpu

ADAPTIVE = dict(min_samples=1, max_samples=6, budget=2.5)
_scenes = {}


def _scene(rrt):
    from rust_ray_tracing_amd import synth
    if "cornell" not in _scenes:
        tris, mats, texs, cam = synth.make_scene("cornell")
        sc = rrt.Scene.from_arrays(tris, mats, texs)
        sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
        sc.upload(0)
        _scenes["cornell"] = sc
    return _scenes["cornell"]


def _moved(rrt, cam, dp=(0.0, 0.0, 0.0), dyaw=0.0):
    c = rrt.Camera(position=tuple(float(cam.position[i]) + dp[i] for i in range(3)), pitch=cam.pitch, yaw=cam.yaw + dyaw)
    c.update_view()
    return c


def _renderer(rrt, size, samples=2):
    from rust_ray_tracing_amd import _lib as L
    return rrt.Renderer.new(rrt.RendererOptions(samples=samples, max_ray_depth=6, output_image_dimensions=size, output_image_path="/dev/null",
                                                seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("size,upsample", [((32, 24), None), ((64, 48), 2)])
def test_sequence_counts_follow_the_model_and_frames_follow_the_counts(rrt, size, upsample):
    import torch
    sc = _scene(rrt)
    path = [[_moved(rrt, sc.camera)], [_moved(rrt, sc.camera, dp=(0.03, 0.0, 0.01), dyaw=0.5)], [_moved(rrt, sc.camera, dp=(0.06, 0.0, 0.02), dyaw=1.0)]]
    r = _renderer(rrt, size)
    low = _renderer(rrt, (32, 24), samples=ADAPTIVE["max_samples"])         # the renderer the sequence traces with: the cap is max_samples
    frames = []
    for fr in r.render_sequence(sc, path, denoise="variance", upsample=upsample, adaptive=ADAPTIVE, max_history=16.0):
        torch.cuda.synchronize()
        frames.append({k: fr[k].cpu().numpy() for k in ("out", "noisy", "counts", "variance_out")})
        frames[-1]["albedo"] = fr["features"]["albedo"].cpu().numpy()
        frames[-1]["stats"] = fr["stats"]
        if upsample:
            assert tuple(fr["out_full"].shape) == (1, 48, 64, 3)
    assert len(frames) == 3
    assert frames[0]["counts"].shape == (1, 24, 32) and np.all(frames[0]["counts"] == 2)     # floor(2.5) everywhere
    varied = False
    for f in range(3):
        g = frames[f]
        if f > 0:
            p = frames[f - 1]
            want = SM.sample_map(p["variance_out"], p["out"], p["albedo"], **ADAPTIVE)
            assert np.array_equal(g["counts"].view(np.uint32), want), f
            assert int(want.sum()) <= SM.total(ADAPTIVE["budget"], want.size)
            varied = varied or want.min() != want.max()
        hdr, _, st = low.render_adaptive(sc, g["counts"].view(np.uint32), path[f], sample_begin=1 + f * ADAPTIVE["max_samples"])
        assert np.array_equal(_bits(g["noisy"]), _bits(hdr)), f
        assert g["stats"]["pixels"] == st["pixels"] == int(np.count_nonzero(g["counts"]))
    assert varied                                                            # the map did tell pixels apart


def test_adaptive_needs_the_variance_filter_and_none_is_the_path_of_before(rrt):
    import torch
    from rust_ray_tracing_amd import _lib as L
    sc = _scene(rrt)
    size = (32, 24)
    cams = [_moved(rrt, sc.camera)]
    r = _renderer(rrt, size)
    for denoise in (True, False):
        with pytest.raises(ValueError):
            next(r.render_sequence(sc, [cams], denoise=denoise, adaptive=ADAPTIVE))
    with pytest.raises(ValueError):
        next(r.render_sequence(sc, [cams], denoise="variance", adaptive=dict(min_samples=1)))
    fr = next(r.render_sequence(sc, [cams], denoise="variance", adaptive=None, max_history=16.0))
    torch.cuda.synchronize()
    assert "counts" not in fr and "variance_out" not in fr
    # the unchanged call sequence, by hand: batch render, features, temporal, variance filter
    w, h = size
    table = np.ascontiguousarray(np.stack([np.asarray(c.uniform, dtype=L.CAMERA).reshape(()) for c in cams]))
    opt = rrt.make_options(w, h, 2, 6, L.SEED_PER_SAMPLE, L.TRAVERSAL_CULLED, sample_begin=1)
    noisy = torch.empty((1, h, w, 3), dtype=torch.float32, device="cuda")
    st = L.MiptStats()
    L.check(rrt.load().mipt_render_batch_device(sc.upload(0), L.ptr(table), 1, C.byref(opt), noisy.data_ptr(), None, None, C.byref(st)),
            "mipt_render_batch_device")
    one = _renderer(rrt, size, samples=1)
    features, _ = one.render_features(sc, cams, ("depth", "normal", "albedo", "position", "material"), device=True)
    acc, _, extras = r.temporal(noisy, features, table, want_length=True, want_variance=True, max_history=16.0)
    out = r.denoise_variance(acc, extras["variance"], extras["length"], features["normal"], features["depth"], features["albedo"])
    torch.cuda.synchronize()
    assert torch.equal(fr["noisy"].view(torch.int32), noisy.view(torch.int32))
    assert torch.equal(fr["out"].view(torch.int32), out.view(torch.int32))
    assert fr["stats"]["pixels"] == st.pixels == w * h
