"""-m gpu: the uv panel (tests/tools/uv_panel.py) through the real kernels.  Every triangle of the panel carries one edge coordinate
pair, so whole patches of the frame look their textures up at texel boundaries, negative, subnormal, huge, infinite and NaN
coordinates -- in the trace kernels (single view and batch, three traversal arms, both seed modes) against the oracle, and in the
first-hit pass against the features model.  What the panel reaches is asserted from the model side before anything is compared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))

import features_model as F  # noqa: E402
import uv_panel as P  # noqa: E402

ARMS = ((0, 0.0), (1, 0.0078125), (1, 0.0))
COUNTERS = ("rays", "inner_steps", "tri_tests", "hits", "texel_fetches", "tex_clamped", "max_stack")


@pytest.fixture(scope="module")
def panel(rrt):
    """the panel, resident on device 0 for this module's tests and released after them; `rays` keeps the model's camera rays per seed mode"""
    sc = P.scene(rrt)
    sc.upload(0)
    sc.rays = {}
    yield sc
    sc.release()


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _render(rrt, sc, cam, arm, seed_mode, flags):
    from rust_ray_tracing_amd import _lib as L
    w, h = P.SIZE
    o = rrt.make_options(w, h, P.SPP, P.DEPTH, seed_mode=seed_mode, traversal=arm[0], flags=flags, cull_margin=arm[1])
    hdr, rgba, st = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 4), np.uint8), L.MiptStats()
    L.check(rrt.load().mipt_render(sc._handle, L.ptr(cam.uniform), C.byref(o), L.ptr(hdr), L.ptr(rgba), C.byref(st)), "mipt_render")
    return hdr, rgba, st.as_dict()


@pytest.mark.parametrize("seed_mode", [0, 1])
@pytest.mark.parametrize("arm", ARMS, ids=["ref", "cullsafe", "cull0"])
def test_trace_equals_oracle_on_the_panel(rrt, orc, panel, arm, seed_mode):
    from rust_ray_tracing_amd import _lib as L
    sc = panel
    w, h = P.SIZE
    ref, ref_rgba, rst = orc.render(sc.tris, sc.bvh_nodes, sc.materials_array(), sc.textures, sc.camera.uniform, w, h, P.SPP, P.DEPTH,
                                    seed_mode=seed_mode, cull=arm[0], cull_margin=arm[1])
    assert 0 < rst["tex_clamped"] < rst["texel_fetches"]                      # from the oracle: some lookups leave their texture, not all
    hdr, rgba, st = _render(rrt, sc, sc.camera, arm, seed_mode, L.FLAG_COUNT)
    assert _same(hdr, ref) and np.array_equal(rgba, ref_rgba)
    for k in COUNTERS:
        assert st[k] == rst[k], (k, st[k], rst[k])
    assert st["pixels"] == w * h and st["stack_overflows"] == 0
    hdr, rgba, st = _render(rrt, sc, sc.camera, arm, seed_mode, 0)            # the product build: no counters but tex_clamped
    assert _same(hdr, ref) and np.array_equal(rgba, ref_rgba) and st["tex_clamped"] == rst["tex_clamped"]


@pytest.mark.parametrize("seed_mode,samples", [(0, 1), (1, 2)])
def test_first_hit_equals_model_on_the_panel(rrt, orc, panel, seed_mode, samples):
    from rust_ray_tracing_amd import _lib as L
    sc = panel
    w, h = P.SIZE
    names = ("material", "uv", "albedo", "emission")
    for arm in ARMS:
        cull = arm[0] == 1
        want, counters, _ = F.frame(orc, sc, sc.camera.uniform, w, h, seed_mode, samples, 0, cull, arm[1], rays=sc.rays.setdefault(seed_mode, {}))
        if samples == 1:
            P.assert_coverage(sc, want)                                       # index 0 and n-1 of every texture, NaN, negative-unclamped, 0 < clamped < fetches
            clamped = P.first_hit_lookups(sc, want)[1]["clamped"]
        else:
            clamped = sum(P.first_hit_lookups(sc, F.frame(orc, sc, sc.camera.uniform, w, h, 1, 1, s, cull, arm[1], rays=sc.rays[seed_mode])[0])[1]["clamped"]
                          for s in range(1, samples + 1))
        for flags in (L.FLAG_COUNT, 0):
            o = rrt.make_options(w, h, samples, 1, seed_mode=seed_mode, traversal=arm[0], flags=flags, cull_margin=arm[1])
            bufs, st, got = L.MiptFeatureBuffers(), L.MiptStats(), {}
            for k in names:
                got[k] = np.zeros((h, w) + ((F.WIDTH[k],) if F.WIDTH[k] > 1 else ()), dtype=np.uint32 if k in F.UINT else np.float32)
                setattr(bufs, k, got[k].ctypes.data)
            cam = np.ascontiguousarray(np.asarray(sc.camera.uniform, dtype=L.CAMERA).reshape(1))
            L.check(rrt.load().mipt_render_features(sc._handle, L.ptr(cam), 1, C.byref(o), C.byref(bufs), C.byref(st)), "mipt_render_features")
            st = st.as_dict()
            assert np.array_equal(got["material"], want["material"])
            for k in ("uv", "albedo", "emission"):
                assert _same(got[k], want[k]), (k, arm, flags)
            assert st["tex_clamped"] == clamped and st["pixels"] == w * h
            if flags:
                for k in F.COUNTERS:
                    assert st[k] == counters[k], (k, st[k], counters[k])


def test_batch_of_three_views_equals_its_single_renders(rrt, panel):
    from rust_ray_tracing_amd import _lib as L
    sc = panel
    w, h = P.SIZE
    cams = P.cameras(rrt)
    o = rrt.make_options(w, h, P.SPP, P.DEPTH, flags=L.FLAG_COUNT)
    table = np.ascontiguousarray(np.stack([np.asarray(c.uniform, dtype=L.CAMERA).reshape(()) for c in cams]))
    hdr, rgba, st = np.zeros((3, h, w, 3), np.float32), np.zeros((3, h, w, 4), np.uint8), L.MiptStats()
    L.check(rrt.load().mipt_render_batch(sc._handle, L.ptr(table), 3, C.byref(o), L.ptr(hdr), L.ptr(rgba), C.byref(st)), "mipt_render_batch")
    st = st.as_dict()
    singles = [_render(rrt, sc, c, ARMS[0], 0, L.FLAG_COUNT) for c in cams]
    for v, (one, one_rgba, _) in enumerate(singles):
        assert _same(hdr[v], one) and np.array_equal(rgba[v], one_rgba), v
    for k in COUNTERS[:-1] + ("pixels",):
        assert st[k] == sum(s[2][k] for s in singles), k
