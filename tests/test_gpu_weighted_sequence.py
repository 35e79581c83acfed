"""-m gpu: render_sequence(adaptive=dict(..., blend="counts", rounds=R)) over 3 moving frames at 32x24.  With blend="counts" every
frame's accumulated frame, length, variance and history are the count-aware model's, fed the planes and the count plane the sequence
itself used; with rounds every frame's counts are the filling map's model on the frame before; with neither key the frames are the
plain temporal model's and the plain map's, as before."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import sample_map_fill_model as FM  # noqa: E402
import sample_map_model as SM  # noqa: E402
import temporal_counts_model as TC  # noqa: E402
import temporal_model as T  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE = (32, 24)
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


def _run(rrt, adaptive):
    """the sequence's three frames as numpy arrays, the history copied (its two tensors are reused), and the camera tables"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    sc = _scene(rrt)
    path = [[_moved(rrt, sc.camera)], [_moved(rrt, sc.camera, dp=(0.03, 0.0, 0.01), dyaw=0.5)], [_moved(rrt, sc.camera, dp=(0.06, 0.0, 0.02), dyaw=1.0)]]
    r = rrt.Renderer.new(rrt.RendererOptions(samples=2, max_ray_depth=6, output_image_dimensions=SIZE, output_image_path="/dev/null",
                                             seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED))
    frames = []
    for fr in r.render_sequence(sc, path, denoise="variance", adaptive=adaptive, max_history=16.0):
        torch.cuda.synchronize()
        g = {k: fr[k].cpu().numpy() for k in ("out", "accumulated", "noisy", "counts", "variance_out", "length", "variance")}
        g["history"] = fr["history"].cpu().numpy().view(np.uint32).copy()
        g["features"] = {k: v.cpu().numpy() for k, v in fr["features"].items()}
        frames.append(g)
    assert len(frames) == 3
    return frames, [np.stack([c.uniform for c in cams]) for cams in path]


def _temporal_matches(frames, tables, counted, cap):
    w, h = SIZE
    history, seen_zero, seen_reuse = None, 0, 0
    for f, g in enumerate(frames):
        ft = g["features"]
        args = (g["noisy"], ft["position"], ft["normal"], ft["depth"], ft["material"].view(np.uint32), tables[f])
        opts = dict(T.DEFAULTS, max_history=16.0)
        if counted:
            want = TC.step(*args, g["counts"].view(np.uint32), cap, history, ft["albedo"], **opts)
            seen_zero += int((want["n"] == 0).sum())
            seen_reuse += int(want["reuse"].sum())
        else:
            want = T.step(*args, history, ft["albedo"], **opts)
        assert T.same_bits(g["accumulated"], want["out"]), (f, "accumulated")
        assert T.same_bits(g["length"], want["length"]) and T.same_bits(g["variance"], want["variance"]), f
        assert T.same_history(g["history"], want["history"], 1, h, w), (f, "history")
        history = g["history"]                                             # the sequence's own, as it used it
    return seen_zero, seen_reuse


@pytest.mark.parametrize("adaptive", [dict(min_samples=1, max_samples=6, budget=2.5), dict(min_samples=0, max_samples=6, budget=1.5)],
                         ids=["min1", "min0"])
def test_blend_by_counts_is_the_counting_model(rrt, adaptive):
    frames, tables = _run(rrt, dict(adaptive, blend="counts"))
    assert np.all(frames[0]["counts"] == max(1, int(adaptive["budget"])))   # frame 0: the uniform plane, and the blend gets it
    zero, reuse = _temporal_matches(frames, tables, True, adaptive["max_samples"])
    assert reuse > 100 and (zero > 0 or adaptive["min_samples"] > 0)        # pixels without a sample occur where the floor allows them
    assert float(frames[2]["length"].max()) > 3.0                           # lengths count samples: more than one per frame
    for f in (1, 2):                                                        # the map is the plain one: `rounds` is absent
        p = frames[f - 1]
        assert np.array_equal(frames[f]["counts"].view(np.uint32), SM.sample_map(p["variance_out"], p["out"], p["features"]["albedo"], **adaptive)), f


def test_rounds_make_the_counts_the_filling_maps(rrt):
    adaptive = dict(min_samples=1, max_samples=6, budget=2.5)
    frames, tables = _run(rrt, dict(adaptive, rounds=3))
    raised = 0
    for f in (1, 2):
        p = frames[f - 1]
        planes = (p["variance_out"], p["out"], p["features"]["albedo"])
        want = FM.fill(*planes, **adaptive, rounds=3)
        assert np.array_equal(frames[f]["counts"].view(np.uint32), want), f
        assert int(want.sum()) <= SM.total(adaptive["budget"], want.size)
        raised += int(np.count_nonzero(want != SM.sample_map(*planes, **adaptive)))
    assert raised > 0                                                       # the later rounds had something to hand on
    _temporal_matches(frames, tables, False, None)                          # `blend` is absent: the plain accumulation


def test_both_keys_together_and_neither(rrt):
    adaptive = dict(min_samples=1, max_samples=6, budget=2.5)
    frames, tables = _run(rrt, dict(adaptive, blend="counts", rounds=3))
    _temporal_matches(frames, tables, True, 6)
    p = frames[1]
    assert np.array_equal(frames[2]["counts"].view(np.uint32), FM.fill(p["variance_out"], p["out"], p["features"]["albedo"], **adaptive, rounds=3))
    # neither key: the sequence of before -- the plain map over the plain accumulation
    frames, tables = _run(rrt, adaptive)
    _temporal_matches(frames, tables, False, None)
    for f in (1, 2):
        p = frames[f - 1]
        assert np.array_equal(frames[f]["counts"].view(np.uint32), SM.sample_map(p["variance_out"], p["out"], p["features"]["albedo"], **adaptive)), f
    sc = _scene(rrt)
    from rust_ray_tracing_amd import _lib as L
    r = rrt.Renderer.new(rrt.RendererOptions(samples=2, max_ray_depth=6, output_image_dimensions=SIZE, output_image_path="/dev/null",
                                             seed_mode=L.SEED_PER_SAMPLE))
    with pytest.raises(ValueError):
        next(r.render_sequence(sc, [[_moved(rrt, sc.camera)]], denoise="variance", adaptive=dict(adaptive, blend="frames")))
    with pytest.raises(ValueError):
        next(r.render_sequence(sc, [[_moved(rrt, sc.camera)]], denoise="variance", adaptive=dict(adaptive, passes=2)))
