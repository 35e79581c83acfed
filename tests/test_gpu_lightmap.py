"""GPU: mipt_bake_surface, mipt_lightmap_filter, mipt_lightmap_dilate (csrc/bake.hip, csrc/lightmap.hip, csrc/mipt_lightmap.cpp), their
_device forms and Scene.bake_lightmap(filter=, dilate=) against the models of tests/tools/lightmap_model.py.  Every output is
compared on the bits (a NaN equal to a NaN), is prefilled with a poison pattern and has a sentinel behind it.  The shapes are the
smallest at which the 64 x 4 tiling can go wrong; the launches past their caps are those DESIGN.md section 21 names."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import bake_model as B  # noqa: E402
import hard_inputs as H  # noqa: E402
import launch_thresholds as LT  # noqa: E402
import lightmap_model as M  # noqa: E402
import test_gpu_bake as TB  # noqa: E402
from test_lightmap_model import separated_charts  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = TB.SENTINEL
POISON = 0x7FB1B2B3                             # a NaN pattern no output has
EXTRA = 4
K_MAX_GRID = 1 << 16                            # restated from csrc/tile_shape.h (kAtlasMaxGrid): edit together with it


def _poisoned(n_words, device):
    import torch
    a = np.full(n_words + EXTRA, POISON, dtype=np.uint32)
    a[n_words:] = SENTINEL
    return torch.from_numpy(a.view(np.int32)).cuda() if device else a


def _words(buf, n_words):
    a = buf.cpu().numpy().view(np.uint32) if hasattr(buf, "cpu") else buf
    assert np.all(a[n_words:] == SENTINEL), "written past the output"
    return a[:n_words].copy()


def _p(buf):
    from rust_ray_tracing_amd import _lib as L
    return None if buf is None else (buf.data_ptr() if hasattr(buf, "data_ptr") else L.ptr(buf))


# ---- surface -------------------------------------------------------------------------------------------------------------------------
def _surface(rrt, sc, pts, unit=False, device=False, want=(True, True), handle=None, lib=None, stream=None):
    """one call of the C entry -> (rc, position or None, normal or None), each [n, 3] f32; poison in, sentinels checked"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = lib or rrt.load()
    n = len(pts)
    opt = L.MiptBakeSurfaceOptions()
    opt.flags = 1 if unit else 0
    outs = [_poisoned(n * 3, device) if w else None for w in want]
    h = handle if handle is not None else sc._handle
    if device:
        d_p = TB._dev(pts)
        rc = lib.mipt_bake_surface_device(h, d_p.data_ptr(), n, C.byref(opt), _p(outs[0]), _p(outs[1]), stream)
        torch.cuda.synchronize()
    else:
        p = np.ascontiguousarray(pts)
        rc = lib.mipt_bake_surface(h, L.ptr(p), n, C.byref(opt), _p(outs[0]), _p(outs[1]))
    return (rc,) + tuple(None if o is None else _words(o, n * 3).view(np.float32).reshape(n, 3) for o in outs)


def _check_surface(rrt, sc, caller, pts, what, handle=None, lib=None):
    for unit in (False, True):
        wp, wn = M.surface_all(caller, pts, unit)
        for device in (False, True):
            rc, gp, gn = _surface(rrt, sc, pts, unit, device, handle=handle, lib=lib)
            assert rc == 0, (what, (lib or rrt.load()).mipt_last_error())
            assert M.same_bits(gp, wp) and M.same_bits(gn, wn), (what, unit, device, H.bad_rows(gp, wp), H.bad_rows(gn, wn))
            none = pts["prim"] == B.NONE
            assert not gp[none].view(np.uint32).any() and not gn[none].view(np.uint32).any()        # +0, not -0
    return wp, wn


@pytest.mark.parametrize("kind", ["cornell", "helmet"])
def test_surface_model_parity(rrt, orc, kind):
    """the 257 points of tests/test_gpu_bake.py (both sides, corners, no point, texels, hits) on a scene built on the device from a
    shuffled array; raw and unit normals, both entries, and one output NULL at a time"""
    sc, _, caller, pts = TB._case(rrt, orc, kind)
    wp, wn = _check_surface(rrt, sc, caller, pts, kind)
    assert len(np.unique(wp, axis=0)) > 200 and np.abs(wn).max() > 0
    for device in (False, True):
        rc, gp, gn = _surface(rrt, sc, pts, True, device, want=(True, False))
        assert rc == 0 and gn is None and M.same_bits(gp, wp)
        rc, gp, gn = _surface(rrt, sc, pts, True, device, want=(False, True))
        assert rc == 0 and gp is None and M.same_bits(gn, wn)


def test_surface_hard_points_and_the_callers_tree(rrt):
    """the hard points of tests/tools/hard_inputs.py (zero, NaN, huge and tiny normals, a zero-area triangle, u and v out of range,
    junk in the unused prim bits) among random ones, on a device-built scene and on one created from the caller's own tree"""
    import test_gpu_bake_hard as TH
    for name, sc, caller, special in TH._special_scenes(rrt):
        hard, tags = H.hard_points(caller, special)
        pts, _, _ = H.interleave(hard, TB._random_points(caller, 96, TB.POINT_SEED))
        _, wn = _check_surface(rrt, sc, caller, pts, name)
        unit = M.surface_all(caller, pts, True)[1]
        assert np.isnan(unit).any() and np.isnan(wn).any()                                            # normalized(0) and the NaN normal


def test_surface_on_a_mesh_scene_after_refit_and_after_rebuild(rrt):
    from rust_ray_tracing_amd import _lib as L
    tris = TB._soup(rrt, 96, seed=5)
    tris["vertices"]["normal"] = np.random.default_rng(3).normal(size=(96, 3, 3)).astype(np.float32)
    v = tris["vertices"]
    mesh = rrt.Scene.from_mesh(positions=v["position"].reshape(-1, 3), normals=v["normal"].reshape(-1, 3),
                               tex_coords=np.stack([v["tex_coord_x"], v["tex_coord_y"]], axis=-1).reshape(-1, 2),
                               indices=np.arange(96 * 3, dtype=np.uint32), parts=[(0, 40, 0), (40, 56, 0)], materials=[rrt.material_default()])
    caller = mesh.expand_mesh().copy()
    mesh.upload_from_mesh(0)
    _check_surface(rrt, mesh, caller, TB._random_points(caller, 130, 5), "mesh")

    sc, caller = TB._from_triangles(rrt, tris, [rrt.material_default()])
    pts = TB._random_points(caller[:60], 130, 6)
    before, _ = _check_surface(rrt, sc, caller, pts, "first tree")                                     # the index map of the first tree is in place
    new = caller.copy()
    new["vertices"]["position"] = (new["vertices"]["position"] * np.float32(1.25) + np.float32(0.5)).astype(np.float32)
    new["vertices"]["normal"] = new["vertices"]["normal"][:, ::-1].copy()
    sc.tris = np.ascontiguousarray(new[sc._tri_order])
    sc.update_device(L.UPDATE_REFIT)
    after, _ = _check_surface(rrt, sc, new, pts, "refit")
    assert not M.same_bits(before, after)
    order = sc._tri_order
    rebuilt = new[:60][::-1].copy()                                                                  # another count and order: a new tree, a new map
    sc.tris, sc._tri_order = rebuilt, None
    sc.update_device(L.UPDATE_REBUILD)
    assert len(sc.tris) == 60 and not np.array_equal(sc._tri_order, order[:60])
    last, _ = _check_surface(rrt, sc, rebuilt, pts, "rebuild")
    assert not M.same_bits(last, after)


def test_surface_on_a_replica_handle_a_side_stream_and_the_wrapper(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    sc, _, caller, pts = TB._case(rrt, orc, "cornell")
    wp, wn = M.surface_all(caller, pts, True)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rc, gp, gn = _surface(rrt, sc, pts, True, True, stream=side.cuda_stream)
        dp, dn = sc.bake_surface(TB._dev(pts), unit_normals=True)
    side.synchronize()
    assert rc == 0 and M.same_bits(gp, wp) and M.same_bits(gn, wn)
    assert M.same_bits(dp.cpu().numpy(), wp) and M.same_bits(dn.cpu().numpy(), wn)
    hp, hn = sc.bake_surface(pts, unit_normals=True)
    assert M.same_bits(hp, wp) and M.same_bits(hn, wn)
    only, none = sc.bake_surface(pts, want=("position",))
    assert none is None and M.same_bits(only, wp)
    mt = L.load_multitest()
    host = rrt.Scene.from_arrays(caller, sc.materials, sc.textures, build_bvh=False)
    d = host.desc()
    multi = C.c_void_p()
    assert mt.mipt_multi_create_from_triangles(C.byref(d), (C.c_int * 2)(0, 0), 2, C.byref(multi)) == 0, mt.mipt_last_error()
    try:
        _check_surface(rrt, None, caller, pts, "replica", handle=mt.mipt_multi_scene(multi, 1), lib=mt)
    finally:
        mt.mipt_multi_destroy(multi)


def test_surface_past_the_lanes_and_a_bad_prim_there(rrt, orc):
    """bake_surface_kernel and check_points_kernel walk the points with a grid-stride loop: lanes_cap + 4 099 points, every word of
    both outputs against the model (the points repeat with a period of 1 031, the model is evaluated once per period); then two bad
    triangle indices above the cap, the lower one named and nothing written"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc, _, caller, _ = TB._case(rrt, orc, "helmet")
    cap = LT.lanes_cap(LT.device_n_cu())
    n, period = cap + 4099, 1031
    base = TB._random_points(caller, period, 12)
    bp, bn = M.surface_all(caller, base, True)
    idx = np.arange(n) % period
    pts = base[idx]
    assert (n - 1) % period != (cap - 1) % period
    for device in (True, False):
        rc, gp, gn = _surface(rrt, sc, pts, True, device)
        assert rc == 0, lib.mipt_last_error()
        bad = np.flatnonzero(~(((gp.view(np.uint32) == bp[idx].view(np.uint32)) | (np.isnan(gp) & np.isnan(bp[idx]))).all(1)))
        assert len(bad) == 0, (device, len(bad), bad[:4], cap)
        assert M.same_bits(gn, bn[idx]), device
        assert M.same_bits(gp[cap - 3: cap + 3], bp[idx[cap - 3: cap + 3]]) and M.same_bits(gp[-1], bp[idx[-1]])      # both sides of the cap, named
    lower, upper = cap + 130, cap + 3001
    pts = pts.copy()
    pts["prim"][lower], pts["prim"][upper] = (len(caller) + 7) | B.FRONT, len(caller)
    d_pos, d_nrm = _poisoned(n * 3, True), _poisoned(n * 3, True)
    rc = lib.mipt_bake_surface_device(sc._handle, TB._dev(pts).data_ptr(), n, None, d_pos.data_ptr(), d_nrm.data_ptr(), None)
    msg = lib.mipt_last_error().decode()
    assert rc == L.ERR_INVALID_ARG and msg == f"mipt_bake_surface_device: points[{lower}].prim names a triangle the scene does not have ({len(caller)} triangles)", msg
    torch.cuda.synchronize()
    assert np.all(_words(d_pos, n * 3) == POISON) and np.all(_words(d_nrm, n * 3) == POISON)
    small = pts[lower - 5: upper + 1]
    rc, _, _ = _surface(rrt, sc, small, device=False)
    assert rc == L.ERR_INVALID_ARG and "points[5].prim" in lib.mipt_last_error().decode()


# ---- filter --------------------------------------------------------------------------------------------------------------------------
def _filter(rrt, rad, pts, pos=None, nrm=None, device=False, alias=False, stream=None, **o):
    """one call of the C entry -> out [H, W, 3]; `alias`: out == radiance"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    h, w, _ = rad.shape
    n = h * w
    opt = L.MiptLightmapFilterOptions()
    opt.width, opt.height = w, h
    opt.iterations, opt.sigma_color, opt.sigma_normal, opt.sigma_plane, opt.sigma_distance = 5, 4.0, 0.5, 0.05, 0.5
    for k, v in o.items():
        setattr(opt, k, v)
    b = L.MiptLightmapFilterBuffers()
    keep = []

    def up(a, dtype=np.float32):
        if a is None:
            return None
        a = np.ascontiguousarray(a).view(np.uint32).reshape(-1)
        t = torch.from_numpy(a.view(np.int32).copy()).cuda() if device else a.copy()
        keep.append(t)
        return _p(t)

    out = _poisoned(n * 3, device)
    if alias:
        src = np.concatenate([np.ascontiguousarray(rad).view(np.uint32).reshape(-1), np.full(EXTRA, SENTINEL, np.uint32)])
        out = torch.from_numpy(src.view(np.int32)).cuda() if device else src
        b.radiance = _p(out)
    else:
        b.radiance = up(rad)
    b.points, b.position, b.normal, b.out = up(pts), up(pos), up(nrm), _p(out)
    if device:
        need = lib.mipt_lightmap_filter_workspace_bytes(w, h)
        ws = torch.full((need // 4 + EXTRA,), SENTINEL, dtype=torch.int32, device="cuda")
        rc = lib.mipt_lightmap_filter_device(C.byref(opt), C.byref(b), ws.data_ptr(), need, stream)
        torch.cuda.synchronize()
        assert bool((ws[need // 4:] == SENTINEL).all()), "written past the workspace"
    else:
        rc = lib.mipt_lightmap_filter(C.byref(opt), C.byref(b), 0)
    assert rc == 0, lib.mipt_last_error()
    return _words(out, n * 3).view(np.float32).reshape(h, w, 3)


def _coverages(w, h, rng):
    board = (np.add.outer(np.arange(h), np.arange(w)) % 2) == 0
    one = np.zeros((h, w), dtype=bool)
    one[h // 2, w // 3] = True
    charts = np.zeros((h, w), dtype=bool)                          # two rectangular charts, a 2-texel gutter between them
    cut = max(w // 2 - 1, 0)
    charts[:, :cut] = True
    charts[: max(h - 1, 1), cut + 2:] = True
    return [("all", np.ones((h, w), dtype=bool)), ("none", np.zeros((h, w), dtype=bool)), ("one", one), ("board", board), ("charts", charts)]


def _atlas(w, h, rng):
    rad = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
    pos = np.empty((h, w, 3), dtype=np.float32)                    # a gently curved sheet, 0.1 per texel, plus noise
    pos[..., 0], pos[..., 1] = np.arange(w)[None, :] * 0.1, np.arange(h)[:, None] * 0.1
    pos[..., 2] = rng.uniform(-0.05, 0.05, (h, w))
    nrm = rng.normal(size=(h, w, 3)) * 0.3 + np.array([0, 0, 1.0])
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    return rad, pos, nrm


SHAPES = [(1, 1), (5, 3), (64, 4), (65, 5), (130, 9)]
COMBOS = [(it, g) for it in (1, 2, 5, 8) for g in ((False, False), (True, False), (False, True), (True, True))]


@pytest.mark.parametrize("w,h", SHAPES)
def test_filter_model_parity(rrt, orc, w, h):
    """every coverage pattern at this shape; the 16 combinations of (iterations 1, 2, 5, 8) x (guide subset) are dealt over the
    patterns, four each, so that each shape runs all of them; both entries"""
    rng = np.random.default_rng(w * 100 + h)
    rad, pos, nrm = _atlas(w, h, rng)
    seen = set()
    for ci, (name, cov) in enumerate(_coverages(w, h, rng)):
        pts = M.points_of(cov)
        for j in range(4):
            it, (use_pos, use_nrm) = COMBOS[(ci * 4 + j) % 16]
            seen.add((it, use_pos, use_nrm))
            kw = dict(iterations=it, sigma_color=1.5, sigma_normal=0.8, sigma_plane=0.2, sigma_distance=0.3)
            p, q = (pos if use_pos else None), (nrm if use_nrm else None)
            want = M.filter(orc, rad, cov, position=p, normal=q, **kw)
            assert np.array_equal(want.view(np.uint32)[~cov], rad.view(np.uint32)[~cov])
            for device in (False, True):
                got = _filter(rrt, rad, pts, p, q, device, **kw)
                assert M.same_bits(got, want), (name, it, use_pos, use_nrm, device, H.bad_rows(got.reshape(-1, 3), want.reshape(-1, 3)))
    assert len(seen) == 16


def test_filter_out_may_be_radiance_and_a_side_stream(rrt, orc):
    import torch
    rng = np.random.default_rng(9)
    w, h = 65, 5
    rad, pos, nrm = _atlas(w, h, rng)
    cov = _coverages(w, h, rng)[4][1]
    kw = dict(iterations=3, sigma_distance=0.4, sigma_plane=0.3)
    want = M.filter(orc, rad, cov, position=pos, normal=nrm, **kw)
    for device in (False, True):
        got = _filter(rrt, rad, M.points_of(cov), pos, nrm, device, alias=True, **kw)
        assert M.same_bits(got, want), device
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _filter(rrt, rad, M.points_of(cov), pos, nrm, True, stream=side.cuda_stream, **kw)
    assert M.same_bits(got, want)


def test_filter_nan_and_inf_and_what_uncovered_texels_hold(rrt, orc):
    """a NaN and an inf radiance in covered texels and a NaN normal spread as the model says; a NaN radiance in every UNCOVERED texel
    reaches no covered output -- the test that fails if a kernel weights an uncovered tap by zero instead of skipping it"""
    rng = np.random.default_rng(17)
    w, h = 65, 5
    rad, pos, nrm = _atlas(w, h, rng)
    cov = rng.random((h, w)) < 0.7
    cov[1, 3] = cov[2, 40] = cov[4, 64] = True
    clean = M.filter(orc, rad, cov, position=pos, normal=nrm, iterations=3, sigma_distance=0.4, sigma_plane=0.3)
    dirty = rad.copy()
    dirty[~cov] = np.nan
    for device in (False, True):
        got = _filter(rrt, dirty, M.points_of(cov), pos, nrm, device, iterations=3, sigma_distance=0.4, sigma_plane=0.3)
        assert np.array_equal(got.view(np.uint32)[cov], clean.view(np.uint32)[cov]), device
        assert np.array_equal(got.view(np.uint32)[~cov], dirty.view(np.uint32)[~cov])                 # word for word, payload and all
    hard, hn = rad.copy(), nrm.copy()
    hard[1, 3, 0], hard[2, 40, 1], hn[4, 64, 2] = np.nan, np.inf, np.nan
    want = M.filter(orc, hard, cov, position=pos, normal=hn, iterations=2, sigma_distance=0.4, sigma_plane=0.3)
    assert np.isnan(want[cov]).any() and not np.isnan(want[cov]).all()
    for device in (False, True):
        got = _filter(rrt, hard, M.points_of(cov), pos, hn, device, iterations=2, sigma_distance=0.4, sigma_plane=0.3)
        assert M.same_bits(got, want), device


def test_filter_keeps_charts_apart_that_are_far_apart_in_the_world(rrt, orc):
    rad, cov, pos, a, b, kw = separated_charts()
    other = rad.copy()
    other[b] = other[b] * np.float32(3.0) + np.float32(1.0)
    for device in (False, True):
        base = _filter(rrt, rad, M.points_of(cov), pos, None, device, **kw)
        out = _filter(rrt, other, M.points_of(cov), pos, None, device, **kw)
        assert M.same_bits(base, M.filter(orc, rad, cov, position=pos, **kw))
        assert np.array_equal(out.view(np.uint32)[a], base.view(np.uint32)[a]) and not np.array_equal(out.view(np.uint32)[b], base.view(np.uint32)[b])


def test_more_tiles_than_the_grid_holds(rrt, orc):
    """an atlas of 1 x (4 * kAtlasMaxGrid + 5): one tile more than a launch has workgroups, a ragged one behind it, and the vertical taps
    of the filter and the neighbours of the dilation cross between a workgroup's first trip and another's second"""
    import torch
    w, h = 1, 4 * K_MAX_GRID + 5
    rng = np.random.default_rng(23)
    rad = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
    cov = rng.random((h, w)) < 0.5
    pos = np.zeros((h, w, 3), dtype=np.float32)
    pos[..., 1] = np.arange(h)[:, None] * 0.1
    kw = dict(iterations=2, sigma_color=1.5, sigma_distance=0.3)
    want = M.filter(orc, rad, cov, position=pos, **kw)
    got = _filter(rrt, rad, M.points_of(cov), pos, None, True, **kw)
    tail = slice(4 * K_MAX_GRID - 8, None)
    assert M.same_bits(got[tail], want[tail]) and M.same_bits(got, want)
    want, wl = M.dilate(rad, cov, 2)
    got, gl = _dilate(rrt, rad, M.points_of(cov), 2, True)
    assert M.same_bits(got, want) and np.array_equal(gl, wl) and (wl[tail] > 1).any()
    torch.cuda.synchronize()


# ---- dilate --------------------------------------------------------------------------------------------------------------------------
def _dilate(rrt, rad, pts, radius, device=False, level=True, alias=False, stream=None):
    """one call of the C entry -> (out [H, W, 3], level [H, W] u32 or None)"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    h, w, _ = rad.shape
    n = h * w
    opt = L.MiptLightmapDilateOptions()
    opt.width, opt.height, opt.radius = w, h, radius
    b = L.MiptLightmapDilateBuffers()

    def up(a):
        a = np.ascontiguousarray(a).view(np.uint32).reshape(-1)
        return torch.from_numpy(a.view(np.int32).copy()).cuda() if device else a.copy()

    d_pts = up(pts)
    if alias:
        src = np.concatenate([np.ascontiguousarray(rad).view(np.uint32).reshape(-1), np.full(EXTRA, SENTINEL, np.uint32)])
        out = d_rad = torch.from_numpy(src.view(np.int32)).cuda() if device else src
    else:
        out, d_rad = _poisoned(n * 3, device), up(rad)
    lev = _poisoned(n, device) if level else None
    b.radiance, b.points, b.out, b.level = _p(d_rad), _p(d_pts), _p(out), _p(lev)
    if device:
        need = lib.mipt_lightmap_dilate_workspace_bytes(w, h)
        ws = torch.full((need // 4 + EXTRA,), SENTINEL, dtype=torch.int32, device="cuda")
        rc = lib.mipt_lightmap_dilate_device(C.byref(opt), C.byref(b), ws.data_ptr(), need, stream)
        torch.cuda.synchronize()
        assert bool((ws[need // 4:] == SENTINEL).all()), "written past the workspace"
    else:
        rc = lib.mipt_lightmap_dilate(C.byref(opt), C.byref(b), 0)
    assert rc == 0, lib.mipt_last_error()
    return _words(out, n * 3).view(np.float32).reshape(h, w, 3), (None if lev is None else _words(lev, n).reshape(h, w))


def _dilate_cases():
    rng = np.random.default_rng(41)
    cases = []
    for w, h in ((1, 1), (5, 3), (64, 4), (65, 5), (130, 9)):          # the tile edges 64 / 65 and 4 / 5
        cov = rng.random((h, w)) < 0.08
        cov[h // 2, w // 2] = True
        cases.append((f"{w}x{h}", w, h, cov))
    corner = np.zeros((9, 20), dtype=bool)
    corner[0, 0] = True
    cases.append(("corner", 20, 9, corner))                              # radius 64 reaches beyond both sides
    cases.append(("none", 7, 6, np.zeros((6, 7), dtype=bool)))
    cases.append(("all", 7, 6, np.ones((6, 7), dtype=bool)))
    meet = np.zeros((5, 11), dtype=bool)                                 # two charts whose fronts meet on column 5, equidistant from both
    meet[:, :3], meet[:, 8:] = True, True
    cases.append(("meet", 11, 5, meet))
    return cases


@pytest.mark.parametrize("radius", [0, 1, 3, 64])
def test_dilate_model_parity(rrt, radius):
    rng = np.random.default_rng(radius)
    for name, w, h, cov in _dilate_cases():
        rad = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
        if name == "65x5":
            ys, xs = np.nonzero(cov)
            rad[ys[0], xs[0], 1] = np.nan                                # a NaN in a covered border texel spreads with the passes
        want, wl = M.dilate(rad, cov, radius)
        assert np.array_equal(wl, M.chebyshev_level(cov, radius))
        if name == "meet" and radius >= 3:
            assert np.all(wl[:, 5] == 4) and np.all(wl[:, 4] == 3)
        pts = M.points_of(cov)
        for device in (False, True):
            got, gl = _dilate(rrt, rad, pts, radius, device)
            assert M.same_bits(got, want) and np.array_equal(gl, wl), (name, radius, device)
            got, gl = _dilate(rrt, rad, pts, radius, device, level=False, alias=True)
            assert gl is None and M.same_bits(got, want), (name, radius, device, "out == radiance, no level")


def test_dilate_on_a_side_stream_and_the_wrappers(rrt, orc):
    import torch
    rng = np.random.default_rng(4)
    w, h = 65, 5
    rad, pos, nrm = _atlas(w, h, rng)
    cov = _coverages(w, h, rng)[4][1]
    pts = M.points_of(cov)
    want, wl = M.dilate(rad, cov, 3)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got, gl = _dilate(rrt, rad, pts, 3, True, stream=side.cuda_stream)
    assert M.same_bits(got, want) and np.array_equal(gl, wl)
    out, lev = rrt.lightmap_dilate(rad, pts, radius=3, want_level=True)
    assert M.same_bits(out, want) and np.array_equal(lev, wl)
    d_out, d_lev = rrt.lightmap_dilate(torch.from_numpy(rad).cuda(), TB._dev(pts), radius=3, want_level=True)
    assert M.same_bits(d_out.cpu().numpy(), want) and np.array_equal(d_lev.cpu().numpy().view(np.uint32), wl)
    kw = dict(iterations=2, sigma_color=1.5, sigma_distance=0.4, sigma_plane=0.3)
    fw = M.filter(orc, rad, cov, position=pos, normal=nrm, **kw)
    assert M.same_bits(rrt.lightmap_filter(rad, pts, position=pos, normal=nrm.reshape(-1, 3), **kw), fw)
    d = rrt.Scene.lightmap_filter(torch.from_numpy(rad).cuda(), TB._dev(pts), position=torch.from_numpy(pos).cuda(), normal=torch.from_numpy(nrm).cuda(), **kw)
    assert d.is_cuda and M.same_bits(d.cpu().numpy(), fw)


# ---- pipeline ------------------------------------------------------------------------------------------------------------------------
def test_bake_lightmap_filtered_and_dilated_is_the_models_composed(rrt, orc):
    base = TB._base_scene(rrt, "cornell")
    v = base.tris["vertices"]                                      # the box's UVs tile the atlas: shrink them into a chart with a gutter around it
    real = (v["tex_coord_x"] < 2).all(axis=1)                      # (the debris keeps its UVs far outside)
    v["tex_coord_x"][real] = v["tex_coord_x"][real] * np.float32(0.55) + np.float32(0.2)
    v["tex_coord_y"][real] = v["tex_coord_y"][real] * np.float32(0.6) + np.float32(0.15)
    rng = np.random.default_rng(31)
    sc, caller = TB._from_triangles(rrt, base.tris[rng.permutation(len(base.tris))], base.materials, base.textures)
    w = h = 16
    pts, winfo = B.texels(caller, w, h)
    cov = (pts["prim"] != B.NONE).reshape(h, w)
    assert 4 * winfo["covered"] >= w * h and 10 * (w * h - winfo["covered"]) >= w * h, winfo
    mean = B.Gather(orc, sc, caller).run(pts, 2, 4)["mean"].reshape(h, w, 3)
    pos, nrm = M.surface_all(caller, pts, unit=True)
    fopt = dict(iterations=2, sigma_color=2.0, sigma_normal=0.5, sigma_plane=0.1, sigma_distance=0.5)
    filtered = M.filter(orc, mean, cov, position=pos, normal=nrm, **fopt)
    assert not M.same_bits(filtered, mean)
    want, level = M.dilate(filtered, cov, 2)
    assert (level > 1).sum() >= 10 and not M.same_bits(want, filtered)
    for device in (True, False):
        plain, covered, _ = sc.bake_lightmap(w, h, 2, device=device, max_ray_depth=4)
        same, _, _ = sc.bake_lightmap(w, h, 2, device=device, max_ray_depth=4, filter=None, dilate=0)
        atlas, covered2, stats = sc.bake_lightmap(w, h, 2, device=device, max_ray_depth=4, filter=fopt, dilate=2)
        only_f, _, _ = sc.bake_lightmap(w, h, 2, device=device, max_ray_depth=4, filter=fopt)
        if device:
            assert atlas.is_cuda and covered2.is_cuda
            plain, same, atlas, only_f, covered, covered2 = (t.cpu().numpy() for t in (plain, same, atlas, only_f, covered, covered2))
        assert B.same_bits(plain, mean) and B.same_bits(same, plain)                                  # today's result, on the bits
        assert np.array_equal(covered, cov) and np.array_equal(covered2, cov)                         # the texel pass's mask
        assert atlas.shape == (h, w, 3) and atlas.dtype == np.float32
        assert M.same_bits(only_f, filtered), (device, H.bad_rows(only_f.reshape(-1, 3), filtered.reshape(-1, 3)))
        assert M.same_bits(atlas, want), (device, H.bad_rows(atlas.reshape(-1, 3), want.reshape(-1, 3)))
        assert stats["texels"]["covered_texels"] == winfo["covered"]
