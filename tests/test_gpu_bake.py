"""GPU: mipt_bake_texels / mipt_bake_gather and their _device forms (csrc/bake.hip, csrc/mipt_bake.cpp) against the models of
tests/tools/bake_model.py: the texel pass as a numpy f32 brute force over all triangles, the gather as a Python loop over the oracle's
one-ray entries.  Every comparison is on the bytes.  Scenes are built on the device from a shuffled triangle array, so that the
tree's order is not the caller's; the culled arm of the gather runs at margin 0, the rule the one-ray oracle entries restate."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import bake_model as B  # noqa: E402
import launch_thresholds as LT  # noqa: E402
import radiance_model as R  # noqa: E402

pytestmark = pytest.mark.gpu

REF, CULL = 0, 1
SENTINEL = 0x7FA5A5A5                          # a NaN pattern no record and no radiance has
N_POINTS = 257
PART, FIRST = 42, 100                          # points FIRST ... FIRST + PART - 1 come from bake_texels, the next PART from query_closest
POINT_SEED = 4                                 # chosen on the CPU: with it the model alone meets B.conditions on every scene kind


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def _from_triangles(rrt, caller, mats, texs=()):
    """(resident Scene built on the device with its tree mirrored, the caller's array); the tree's order is asserted not to be the caller's"""
    caller = np.ascontiguousarray(caller).copy()
    sc = rrt.Scene.from_arrays(caller, mats, texs, build_bvh=False)
    sc.upload_from_triangles(0, fetch_bvh=True)
    assert len(caller) >= 64 and not np.array_equal(sc._tri_order, np.arange(len(caller)))
    return sc, caller


def _soup(rrt, n, seed=1):
    """n small triangles scattered in a box, normals up, UVs far outside the atlas (around (7, 7)): fillers that cover nothing"""
    from rust_ray_tracing_amd import _lib as L
    rng = np.random.default_rng(seed)
    t = np.zeros(n, dtype=L.TRIANGLE)
    c = rng.uniform(-4, 4, (n, 1, 3))
    t["vertices"]["position"] = (c + rng.uniform(-0.3, 0.3, (n, 3, 3))).astype(np.float32)
    t["vertices"]["normal"] = (0, 1, 0)
    uv = 7.0 + rng.uniform(0, 0.5, (n, 3, 2))
    t["vertices"]["tex_coord_x"], t["vertices"]["tex_coord_y"] = uv[..., 0].astype(np.float32), uv[..., 1].astype(np.float32)
    return t


def _set_uv(tris, k, uv):
    tris["vertices"]["tex_coord_x"][k], tris["vertices"]["tex_coord_y"][k] = np.float32(uv)[:, 0], np.float32(uv)[:, 1]


def _uv_scene(rrt, layout, n=64, seed=1):
    """the soup with the UV triangles of `layout` ({caller index: 3 x 2}) set"""
    tris = _soup(rrt, n, seed)
    for k, uv in layout.items():
        _set_uv(tris, k, uv)
    return _from_triangles(rrt, tris, [rrt.material_default()])


QUAD = {20: [(0, 0), (1, 0), (1, 1)], 41: [(0, 0), (1, 1), (0, 1)]}     # two triangles over the unit square, the diagonal shared


def _texels(rrt, sc, w, h, device=False, handle=None, lib=None, stream=None, extra=4):
    """One call of the C entry with a sentinel behind the output -> (records [w * h], info dict); the sentinel is asserted"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = lib or rrt.load()
    n = w * h
    info = L.MiptBakeTexelInfo()
    hd = handle if handle is not None else sc._handle
    if device:
        d_out = torch.full((n * 4 + extra,), SENTINEL, dtype=torch.int32, device="cuda")
        rc = lib.mipt_bake_texels_device(hd, w, h, None, d_out.data_ptr(), stream, C.byref(info))
        if stream is not None:
            torch.cuda.synchronize()
        out = d_out.cpu().numpy().view(np.uint32)
    else:
        out = np.full(n * 4 + extra, SENTINEL, dtype=np.uint32)
        rc = lib.mipt_bake_texels(hd, w, h, None, L.ptr(out), C.byref(info))
    assert rc == 0, lib.mipt_last_error()
    assert np.all(out[n * 4:] == SENTINEL), "written past width * height records"
    return out[: n * 4].copy().view(B.POINT), info.as_dict()


def _bad_texels(got, want):
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4))
    return len(bad), [(int(i // 4), got[i // 4].tolist(), want[i // 4].tolist()) for i in bad[:4]]


def _check_texels(rrt, sc, caller, w, h, main=True, index=None):
    want, winfo = B.texels(caller, w, h, index)
    if main:                                                     # conditions on the model
        assert 4 * winfo["covered"] >= len(want) and 10 * (len(want) - winfo["covered"]) >= len(want), winfo
    for device in (False, True):
        got, info = _texels(rrt, sc, w, h, device)
        sel = got if index is None else got[index]
        assert B.same_bits(sel, want), (w, h, device, _bad_texels(sel, want))
        assert info["degenerate_tris"] == winfo["degenerate"] and info["kernel_ms"] > 0
        if index is None:
            assert info["covered_texels"] == winfo["covered"]
    return want, winfo


# ---- texels --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(8, 8), (7, 5), (32, 32), (1, 1)])
def test_texels_quad(rrt, w, h):
    """8x8: the shared diagonal runs through texel centres, which both triangles cover (u == 0 for one, u + v == 1 for the other):
    the lower index gets them.  7x5: odd and not square.  32x32: boxes above 64 texels, the wave's walk.  1x1: one centre, on the
    diagonal of the unscaled quad."""
    layout = {k: np.float32(v) * np.float32(0.75) + np.float32(0.125) for k, v in QUAD.items()} if (w, h) != (1, 1) else QUAD
    sc, caller = _uv_scene(rrt, layout)
    want, _ = _check_texels(rrt, sc, caller, w, h, main=(w, h) != (1, 1))
    owners = set((want["prim"][want["prim"] != B.NONE] & B.TRI_MASK).tolist())
    assert owners == ({20} if (w, h) == (1, 1) else {20, 41})
    if (w, h) == (8, 8):
        on_diag = [y * w + y for y in range(1, 7)]
        assert all(int(want["prim"][i]) == (20 | B.FRONT) for i in on_diag)


def test_texels_identical_uvs_go_to_the_lower_caller_index(rrt):
    probe, _ = _uv_scene(rrt, {})
    pos = np.empty(64, dtype=np.int64)
    pos[probe._tri_order] = np.arange(64)                        # caller index -> tree position (positions alone decide the tree)
    i, j = next((i, j) for i in range(64) for j in range(i + 1, 64) if pos[i] > pos[j])
    tri = [(0.1, 0.1), (0.9, 0.2), (0.3, 0.95)]
    sc, caller = _uv_scene(rrt, {i: tri, j: tri})
    assert np.array_equal(sc._tri_order, probe._tri_order) and pos[i] > pos[j]        # the lower index comes LATER in tree order
    want, _ = _check_texels(rrt, sc, caller, 16, 16)
    assert set((want["prim"][want["prim"] != B.NONE] & B.TRI_MASK).tolist()) == {i}


def test_texels_degenerate_nan_and_outside(rrt):
    nan = float("nan")
    layout = {3: [(0.2, 0.2), (0.6, 0.6), (0.4, 0.4)],           # collinear and exactly representable differences: d == 0
              9: [(0.5, 0.5), (0.5, 0.5), (0.5, 0.5)],           # a point
              17: [(0.1, nan), (0.8, 0.1), (0.1, 0.8)],          # a NaN corner
              30: [(0.5, -0.5), (1.5, 0.5), (0.5, 1.5)],         # half outside [0, 1]
              44: [(0.05, 0.3), (0.45, 0.35), (0.1, 0.9)]}
    sc, caller = _uv_scene(rrt, layout)
    want, winfo = _check_texels(rrt, sc, caller, 24, 20)
    assert winfo["degenerate"] == 3
    assert set((want["prim"][want["prim"] != B.NONE] & B.TRI_MASK).tolist()) == {30, 44}


def test_texels_one_triangle_over_many_tiny_ones(rrt):
    """The cooperative path: the last triangle covers all of a 256 x 256 atlas (its box goes to the grid-wide kernel), 4 096 tiny
    ones of lower index own what they cover.  Compared with the model on 4 096 sampled texels and on every texel's coverage."""
    from rust_ray_tracing_amd import _lib as L
    rng = np.random.default_rng(6)
    n = 4097
    tris = _soup(rrt, n, seed=2)
    c = rng.uniform(0, 1, (n - 1, 1, 2))
    uv = c + rng.uniform(-3.0, 3.0, (n - 1, 3, 2)) / 256                                  # a few texels each: the lane's loop or the wave's
    tris["vertices"]["tex_coord_x"][: n - 1], tris["vertices"]["tex_coord_y"][: n - 1] = uv[..., 0].astype(np.float32), uv[..., 1].astype(np.float32)
    _set_uv(tris, n - 1, [(-1, -1), (3, -1), (-1, 3)])
    sc, caller = _from_triangles(rrt, tris, [rrt.material_default()])
    index = np.sort(rng.choice(256 * 256, 4096, replace=False)).astype(np.uint32)
    want, winfo = _check_texels(rrt, sc, caller, 256, 256, main=False, index=index)
    owners = want["prim"] & B.TRI_MASK
    assert winfo["covered"] == 4096 and 8 * int((owners != n - 1).sum()) >= 4096 and 4 * int((owners == n - 1).sum()) >= 4096
    got, info = _texels(rrt, sc, 256, 256, device=True)
    assert info["covered_texels"] == 256 * 256 and not np.any(got["prim"] == B.NONE)


def test_texels_past_the_lanes_in_flight(rrt):
    """More texels than any launch holds lanes (tests/tools/launch_thresholds.py): the resolve kernel's lanes take a second texel, and
    the two triangles of the quad, whose boxes go to the grid-wide coverage kernel, are more than its lanes hold as well."""
    cap = LT.lanes_cap(LT.device_n_cu())
    w, h = 1024, cap // 1024 + 77
    assert w * h > cap and 9 * w * h > 8 * cap                   # either triangle's box is 9/16 of the atlas: above that kernel's lanes, cap / 2
    layout = {k: np.float32(v) * np.float32(0.75) + np.float32(0.125) for k, v in QUAD.items()}
    sc, caller = _uv_scene(rrt, layout)
    _check_texels(rrt, sc, caller, w, h)


def test_texels_follow_refit_and_rebuild(rrt):
    from rust_ray_tracing_amd import _lib as L
    sc, caller = _uv_scene(rrt, QUAD)
    _check_texels(rrt, sc, caller, 12, 10, main=False)
    for mode, layout in ((L.UPDATE_REFIT, {5: [(0.1, 0.1), (0.7, 0.2), (0.2, 0.8)], 20: [(2, 2), (3, 2), (2, 3)], 41: [(0.4, 0.3), (0.95, 0.5), (0.5, 0.97)]}),
                         (L.UPDATE_REBUILD, {50: [(0.0, 0.0), (0.8, 0.1), (0.1, 0.7)], 5: [(0.3, 0.3), (0.9, 0.4), (0.4, 0.9)], 41: [(5, 5), (6, 5), (5, 6)]})):
        new = caller.copy()
        for k, uv in layout.items():
            _set_uv(new, k, uv)
        if mode == L.UPDATE_REBUILD:
            new["vertices"]["position"] = new["vertices"]["position"][::-1].copy()      # other positions: another tree
        src = new[sc._tri_order] if sc._tri_order is not None else new
        sc.tris = np.ascontiguousarray(src)                      # update_device scatters the tree-ordered mirror back to the caller's order
        sc.update_device(mode)
        caller = new
        _check_texels(rrt, sc, caller, 12, 10)


def test_texels_on_a_mesh_scene(rrt):
    tris = _soup(rrt, 96, seed=5)
    for k, uv in {7: [(0.1, 0.1), (0.9, 0.15), (0.2, 0.9)], 60: [(0.3, 0.3), (0.95, 0.6), (0.6, 0.95)]}.items():
        _set_uv(tris, k, uv)
    v = tris["vertices"]
    sc = rrt.Scene.from_mesh(positions=v["position"].reshape(-1, 3), normals=v["normal"].reshape(-1, 3),
                             tex_coords=np.stack([v["tex_coord_x"], v["tex_coord_y"]], axis=-1).reshape(-1, 2),
                             indices=np.arange(96 * 3, dtype=np.uint32), parts=[(0, 40, 0), (40, 56, 0)], materials=[rrt.material_default()])
    caller = sc.expand_mesh().copy()
    assert B.same_bits(B.corner_uvs(caller), B.corner_uvs(tris))
    sc.upload_from_mesh(0)
    _check_texels(rrt, sc, caller, 20, 20)


def test_texels_device_entry_on_a_side_stream_and_the_wrapper(rrt):
    import torch
    sc, caller = _uv_scene(rrt, QUAD)
    want, winfo = B.texels(caller, 40, 30)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got, _ = _texels(rrt, sc, 40, 30, device=True, stream=side.cuda_stream)
        dev, info = sc.bake_texels(40, 30, device=True)
    side.synchronize()
    host, hinfo = sc.bake_texels(40, 30)
    assert B.same_bits(got, want) and B.same_bits(host, want) and B.same_bits(dev.cpu().numpy().view(np.uint32).reshape(-1).view(B.POINT), want)
    assert info["covered_texels"] == hinfo["covered_texels"] == winfo["covered"]


# ---- gather: scenes, points, the model ------------------------------------------------------------------------------------------------
def _base_scene(rrt, kind):
    """the scene kinds of tests/test_gpu_radiance.py, built the same way"""
    from rust_ray_tracing_amd import synth
    import wgsl_scenes as S
    if kind == "wgsl_pbr":
        return S.pbr_scene(rrt, n_target=20000, tex_size=16)
    kw = dict(n_target=4000, tex_size=64) if kind == "helmet" else {}
    tris, mats, texs, cam = synth.make_scene(kind, **kw)
    if len(tris) < 64:                                           # the cornell box has 12 triangles: debris floating inside it fills the array
        P = tris["vertices"]["position"].reshape(-1, 3)
        lo, hi = P.min(0), P.max(0)
        extra = _soup(rrt, 64 - len(tris), seed=8)
        q = (extra["vertices"]["position"] + np.float32(4.3)) / np.float32(8.6)          # the soup's box -> [0, 1]^3
        extra["vertices"]["position"] = (lo + (hi - lo) * (np.float32(0.1) + np.float32(0.8) * q)).astype(np.float32)
        tris = np.concatenate([tris, extra])
    return rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)


_scenes, _models = {}, {}


def _random_points(caller, n, seed):
    """n points made from `seed` alone: interior points and corners (u = 1, v = 0) on random triangles, both sides, and every 15th
    no point at all; seeds 7 i + 3"""
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=B.POINT)
    b = rng.dirichlet((1.0, 1.0, 1.0), n).astype(np.float32)
    p["u"], p["v"] = b[:, 1], b[:, 2]
    corner = np.arange(n) % 5 == 2
    p["u"][corner], p["v"][corner] = 1.0, 0.0
    p["prim"] = rng.integers(0, len(caller), n).astype(np.uint32) | np.where(rng.random(n) < 0.5, B.FRONT, 0).astype(np.uint32)
    p["prim"][np.arange(n) % 15 == 14] = B.NONE
    p["seed"] = 7 * np.arange(n, dtype=np.uint32) + 3
    return p


def _case(rrt, orc, kind):
    """(resident device-built Scene, B.Gather, the caller's triangles, N_POINTS points) -- made once per scene, left unchanged.  The
    points: two parts random (_random_points), a sixth covered texels of a 48 x 48 atlas, a sixth what query_closest found."""
    if kind not in _scenes:
        base = _base_scene(rrt, kind)
        rng = np.random.default_rng(11)
        sc, caller = _from_triangles(rrt, base.tris[rng.permutation(len(base.tris))], base.materials, base.textures)
        part = PART
        pts = _random_points(caller, N_POINTS, POINT_SEED)
        tex, _ = sc.bake_texels(48, 48)
        tex = tex[tex["prim"] != B.NONE]
        assert len(tex) >= part
        pts[FIRST: FIRST + part] = tex[:: len(tex) // part][:part]
        rays = R.make_rays(caller, part, seed=9)
        rays["t_max"] = 1e30
        raw, _ = sc._query(False, rays, None, REF, 0.0, False, None, None)
        assert int((raw["prim"] != B.NONE).sum()) * 4 >= part
        hit_pts = raw.view(B.POINT).copy()
        hit_pts["seed"] = 1000 + np.arange(part, dtype=np.uint32)
        pts[FIRST + part: FIRST + 2 * part] = hit_pts
        kinds = (int((pts["prim"] == B.NONE).sum()), int(((pts["prim"] & B.FRONT) == 0).sum()), int(((pts["u"] == 1) & (pts["v"] == 0)).sum()))
        assert min(kinds) >= 5, kinds
        _scenes[kind] = (sc, B.Gather(orc, sc, caller), caller, pts)
    return _scenes[kind]


def _model(rrt, orc, kind, samples, depth, shading, cull, first_sample=0, stride=None, n=N_POINTS):
    key = (kind, samples, depth, shading, cull, first_sample, stride, n)
    if key not in _models:
        _, g, _, pts = _case(rrt, orc, kind)
        out = g.run(pts[:n], samples, depth, shading=shading, cull=cull, first_sample=first_sample, stride=stride)
        B.conditions(out, pts[:n])
        _models[key] = out
    return _models[key]


def _dev(points):
    import torch
    return torch.from_numpy(np.ascontiguousarray(points).view(np.int32).reshape(-1, 4).copy()).cuda()


def _gather(rrt, sc, points, samples, depth, shading=0, traversal=REF, flags=0, device=False, first_sample=0, stride=None, handle=None, lib=None,
            d_out=None, extra=4):
    """One call of the C entry with a sentinel behind the output -> (rc, radiance [n, 3] f32, stats dict); the sentinel is asserted"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = lib or rrt.load()
    n = len(points)
    opt = L.MiptBakeOptions()
    opt.samples, opt.max_ray_depth, opt.traversal, opt.cull_margin, opt.shading, opt.flags = samples, depth, traversal, 0.0, shading, flags
    opt.first_sample, opt.sample_stride = first_sample, (n if stride is None else stride)
    st = L.MiptStats()
    h = handle if handle is not None else sc._handle
    if device:
        d_p = _dev(points)
        if d_out is None:
            d_out = torch.full((n * 3 + extra,), SENTINEL, dtype=torch.int32, device="cuda")
        rc = lib.mipt_bake_gather_device(h, d_p.data_ptr(), n, C.byref(opt), d_out.data_ptr(), None, C.byref(st))
        out = d_out.cpu().numpy().view(np.uint32).reshape(-1)
    else:
        out = np.full(n * 3 + extra, SENTINEL, dtype=np.uint32)
        p = np.ascontiguousarray(points)
        rc = lib.mipt_bake_gather(h, L.ptr(p), n, C.byref(opt), L.ptr(out), C.byref(st))
    assert np.all(out[n * 3:] == SENTINEL), "written past n * 3 floats"
    return rc, out[: n * 3].view(np.float32).reshape(n, 3), st.as_dict()


def _bad_rows(got, want):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = np.flatnonzero((g != w).any(axis=1))
    return len(bad), [(int(i), g[i].tolist(), w[i].tolist()) for i in bad[:4]]


# ---- gather: model parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("traversal", [REF, CULL])
@pytest.mark.parametrize("kind,shading", [("cornell", 0), ("cornell", 1), ("helmet", 0), ("helmet", 1), ("wgsl_pbr", 1), ("wgsl_pbr", 0)])
def test_gather_model_parity(rrt, orc, kind, shading, traversal):
    from rust_ray_tracing_amd import _lib as L
    sc, _, _, pts = _case(rrt, orc, kind)
    for samples in (1, 3):
        want = _model(rrt, orc, kind, samples, 4, shading, traversal)
        assert not np.any(want["sum"][pts["prim"] == B.NONE]) and np.any(want["sum"][pts["prim"] != B.NONE])
        for device in (False, True):
            for flags, key in ((0, "mean"), (L.FLAG_SUM, "sum"), (L.FLAG_COUNT, "mean")):
                rc, got, st = _gather(rrt, sc, pts, samples, 4, shading, traversal, flags, device)
                assert rc == 0 and B.same_bits(got, want[key]), (kind, shading, traversal, samples, device, flags, _bad_rows(got, want[key]))
                assert st["kernel_ms"] > 0 and st["stack_overflows"] == 0 and st["pixels"] == len(pts) * samples


def test_gather_index_independence(rrt, orc):
    sc, _, _, pts = _case(rrt, orc, "helmet")
    want = _model(rrt, orc, "helmet", 3, 4, 0, REF)["mean"]
    n = len(pts)
    for order in (np.arange(n)[::-1], np.roll(np.arange(n), 100)):
        for device in (False, True):
            rc, got, _ = _gather(rrt, sc, pts[order], 3, 4, device=device)                 # the stride stays n: the same streams
            assert rc == 0 and B.same_bits(got, want[order]), (device, _bad_rows(got, want[order]))
    rc, got, _ = _gather(rrt, sc, pts[:100], 3, 4, stride=n)                              # fewer points, the same stride
    assert rc == 0 and B.same_bits(got, want[:100])


def test_gather_accumulate_splits_the_sum(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    sc, _, _, pts = _case(rrt, orc, "helmet")
    n = len(pts)
    whole = _model(rrt, orc, "helmet", 8, 4, 0, REF)
    rc, one, _ = _gather(rrt, sc, pts, 8, 4, flags=L.FLAG_SUM, device=True)
    assert rc == 0 and B.same_bits(one, whole["sum"])
    none = pts["prim"] == B.NONE
    for split in ((4, 4), (1, 5, 2)):
        d_acc = torch.zeros((n * 3 + 4,), dtype=torch.float32, device="cuda").view(torch.int32)
        d_acc[n * 3:] = SENTINEL
        first = 0
        for k in split:
            rc, got, _ = _gather(rrt, sc, pts, k, 4, flags=L.FLAG_SUM | L.FLAG_ACCUM, device=True, first_sample=first, d_out=d_acc)
            assert rc == 0
            first += k
        assert B.same_bits(got, whole["sum"]), (split, _bad_rows(got, whole["sum"]))
    # a point without a surface is left untouched under ACCUM; the others go on from what the buffer held
    d_acc = torch.full((n * 3 + 4,), 2.5, dtype=torch.float32, device="cuda").view(torch.int32)
    d_acc[n * 3:] = SENTINEL
    rc, got, _ = _gather(rrt, sc, pts, 1, 4, flags=L.FLAG_SUM | L.FLAG_ACCUM, device=True, d_out=d_acc)
    s1 = _model(rrt, orc, "helmet", 1, 4, 0, REF)["sum"]
    assert rc == 0 and np.all(got[none] == 2.5) and B.same_bits(got[~none], (np.float32(2.5) + s1)[~none])
    # the wrapper: accumulate_into
    acc = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    for first in (0, 4):
        out, _ = sc.bake_gather(_dev(pts), samples=4, max_ray_depth=4, first_sample=first, accumulate_into=acc)
        assert out is acc
    assert B.same_bits(acc.cpu().numpy(), whole["sum"])
    # refused on the host entry, the output untouched
    lib = rrt.load()
    opt = L.MiptBakeOptions()
    opt.samples, opt.max_ray_depth, opt.sample_stride, opt.flags = 2, 4, n, L.FLAG_SUM | L.FLAG_ACCUM
    out = np.zeros((n, 3), np.float32)
    assert lib.mipt_bake_gather(sc._handle, L.ptr(np.ascontiguousarray(pts)), n, C.byref(opt), L.ptr(out), None) == L.ERR_INVALID_ARG
    assert "mipt_bake_gather_device" in lib.mipt_last_error().decode() and not out.any()


def test_gather_first_sample_and_stride(rrt, orc):
    sc, _, _, pts = _case(rrt, orc, "cornell")
    base = _model(rrt, orc, "cornell", 3, 4, 0, REF)["sum"]
    for first, stride in ((5, 1000), (0xFFFFFFFE, 3), (2, 1)):
        want = _model(rrt, orc, "cornell", 3, 4, 0, REF, first_sample=first, stride=stride)
        assert not B.same_bits(want["sum"], base)
        for device in (False, True):
            rc, got, _ = _gather(rrt, sc, pts, 3, 4, device=device, first_sample=first, stride=stride)
            assert rc == 0 and B.same_bits(got, want["mean"]), (first, stride, device, _bad_rows(got, want["mean"]))
    # the wrapper: sample_stride None = the number of points; hits of query_closest with seeds
    got, st = sc.bake_gather(pts, samples=3, max_ray_depth=4)
    assert B.same_bits(got, _model(rrt, orc, "cornell", 3, 4, 0, REF)["mean"]) and st["pixels"] == 3 * len(pts)
    hits = pts[FIRST + PART: FIRST + 2 * PART]
    d = dict(u=hits["u"], v=hits["v"], prim=np.where(hits["prim"] == B.NONE, -1, (hits["prim"] & B.TRI_MASK).astype(np.int64)),
             front_face=(hits["prim"] != B.NONE) & ((hits["prim"] & B.FRONT) != 0))
    got, _ = sc.bake_gather(d, seeds=hits["seed"], samples=3, max_ray_depth=4, sample_stride=len(pts))
    assert B.same_bits(got, _model(rrt, orc, "cornell", 3, 4, 0, REF)["mean"][FIRST + PART: FIRST + 2 * PART])


# ---- gather: scene state --------------------------------------------------------------------------------------------------------------
def test_gather_after_a_rebuild_uses_a_new_index_map(rrt, orc):
    from rust_ray_tracing_amd import _lib as L
    base = _base_scene(rrt, "helmet")
    rng = np.random.default_rng(21)
    sc, caller = _from_triangles(rrt, base.tris[rng.permutation(len(base.tris))], base.materials, base.textures)
    pts = _random_points(caller[: len(caller) - 40], 128, 8)                              # triangles both arrays have
    before = B.Gather(orc, sc, caller).run(pts, 2, 4)
    rc, got, _ = _gather(rrt, sc, pts, 2, 4)
    assert rc == 0 and B.same_bits(got, before["mean"])                                   # the map of the first tree is in place
    new = caller[: len(caller) - 40][::-1].copy()                                          # another count and another order: a new tree
    order = sc._tri_order
    sc.tris, sc._tri_order = new, None                                                    # the caller's order, as update_device wants it
    sc.update_device(L.UPDATE_REBUILD)
    assert len(sc.tris) == len(new) and not np.array_equal(sc._tri_order, order[: len(new)])
    m = B.Gather(orc, sc, new)
    after = m.run(pts, 2, 4, shading=1, cull=1)
    B.conditions(after, pts)
    assert not B.same_bits(after["mean"], before["mean"])                                 # prim k is another triangle now: the caller's k
    for device in (False, True):
        rc, got, _ = _gather(rrt, sc, pts, 2, 4, 1, CULL, device=device)
        assert rc == 0 and B.same_bits(got, after["mean"]), (device, _bad_rows(got, after["mean"]))


def test_gather_and_texels_on_a_replica_handle(rrt, orc):
    from rust_ray_tracing_amd import _lib as L
    mt = L.load_multitest()
    base = _base_scene(rrt, "cornell")
    rng = np.random.default_rng(11)
    caller = np.ascontiguousarray(base.tris[rng.permutation(len(base.tris))])
    host = rrt.Scene.from_arrays(caller, base.materials, base.textures, build_bvh=False)
    d = host.desc()
    multi = C.c_void_p()
    assert mt.mipt_multi_create_from_triangles(C.byref(d), (C.c_int * 2)(0, 0), 2, C.byref(multi)) == 0, mt.mipt_last_error()
    try:
        sc, g, ref_caller, pts = _case(rrt, orc, "cornell")                                # the same triangles in the same order: the same tree
        assert B.same_bits(ref_caller, caller)
        want = _model(rrt, orc, "cornell", 3, 4, 0, REF)["mean"]
        want_tex, _ = B.texels(caller, 24, 24)
        for rank in (0, 1):
            h = mt.mipt_multi_scene(multi, rank)
            for device in (False, True):
                rc, got, st = _gather(rrt, None, pts, 3, 4, device=device, handle=h, lib=mt)
                assert rc == 0 and B.same_bits(got, want), (rank, device, _bad_rows(got, want))
                tex, _ = _texels(rrt, None, 24, 24, device, handle=h, lib=mt)
                assert B.same_bits(tex, want_tex), (rank, device)
    finally:
        mt.mipt_multi_destroy(multi)


def _render(rrt, sc):
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=3, output_image_dimensions=(32, 24), output_image_path="/dev/null"))
    return r.render_buffers(sc)[0].view(np.uint32).copy()


def test_device_entry_refusals_leave_the_scene_rendering(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth
    lib = rrt.load()
    sc, _, caller, pts = _case(rrt, orc, "cornell")
    cam = synth.make_scene("cornell")[3]
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    before = _render(rrt, sc)
    n = 64
    opt = L.MiptBakeOptions()
    opt.samples, opt.max_ray_depth, opt.sample_stride = 2, 4, n
    d_out = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    bad = pts[:n].copy()
    bad["prim"][bad["prim"] == B.NONE] = 0
    for where in ((40,), (63, 17, 50)):
        p = bad.copy()
        p["prim"][list(where)] = (len(caller) + np.arange(len(where))).astype(np.uint32) | np.uint32(B.FRONT)
        assert lib.mipt_bake_gather_device(sc._handle, _dev(p).data_ptr(), n, C.byref(opt), d_out.data_ptr(), None, None) == L.ERR_INVALID_ARG
        assert f"points[{min(where)}].prim" in lib.mipt_last_error().decode(), lib.mipt_last_error()
        h_out = np.zeros((n, 3), np.float32)
        assert lib.mipt_bake_gather(sc._handle, L.ptr(p), n, C.byref(opt), L.ptr(h_out), None) == L.ERR_INVALID_ARG
        assert f"points[{min(where)}].prim" in lib.mipt_last_error().decode() and not h_out.any()
    h_buf = np.zeros(n * 16 + 16, dtype=np.uint8)
    p_ptr = h_buf.ctypes.data + (-h_buf.ctypes.data) % 16
    d_p = _dev(bad)
    f = lib.mipt_bake_gather_device
    for args, msg in (((sc._handle, d_p.data_ptr(), n, C.byref(opt), h_buf.ctypes.data, None, None), "d_radiance is not device memory"),
                      ((sc._handle, p_ptr, n, C.byref(opt), d_out.data_ptr(), None, None), "d_points is not device memory"),
                      ((sc._handle, d_p.data_ptr() + 4, n - 1, C.byref(opt), d_out.data_ptr(), None, None), "d_points must be 16-byte aligned"),
                      ((sc._handle, d_p.data_ptr(), n, C.byref(opt), d_p.data_ptr() + 16 * (n - 1), None, None), "d_points overlaps d_radiance")):
        assert f(*args) == L.ERR_INVALID_ARG, msg
        assert msg in lib.mipt_last_error().decode(), lib.mipt_last_error()
    assert lib.mipt_bake_texels_device(sc._handle, 4, 4, None, p_ptr, None, None) == L.ERR_INVALID_ARG
    assert "d_points is not device memory" in lib.mipt_last_error().decode()
    assert torch.count_nonzero(d_out).item() == 0 and not h_buf.any()
    assert np.array_equal(_render(rrt, sc), before)                                # the scene renders bit-exactly afterwards
    rc, got, _ = _gather(rrt, sc, pts, 3, 4, device=True)
    assert rc == 0 and B.same_bits(got, _model(rrt, orc, "cornell", 3, 4, 0, REF)["mean"])


# ---- gather: chunks, launches past the lanes in flight -------------------------------------------------------------------------------
def test_gather_across_a_chunk_boundary(rrt):
    """2^22 + 65 paths on a one-triangle scene at depth 1, against the same points gathered in two smaller calls.  Three samples per
    point put the chunk boundary INSIDE a point's samples (2^22 is no multiple of 3), so the carried sum is crossed as well; the ray
    generation and reduce kernels run far past the lanes a launch holds in flight."""
    import torch
    from rust_ray_tracing_amd import _lib as L
    tri = _soup(rrt, 1, seed=3)
    tri["vertices"]["position"][0] = [(-1, 0, -1), (1, 0, -1), (0, 0, 1)]
    sc = rrt.Scene.from_arrays(tri, [rrt.material_default()])
    sc.upload(0)
    samples = 3
    n = ((1 << 22) + 65 + samples - 1) // samples
    assert n * samples >= (1 << 22) + 65 and (1 << 22) % samples != 0
    assert n > 2 * LT.lanes_cap(LT.device_n_cu())                                          # every new grid-stride kernel refills its lanes
    rng = np.random.default_rng(2)
    pts = np.zeros(n, dtype=B.POINT)
    b = rng.dirichlet((1.0, 1.0, 1.0), n).astype(np.float32)
    pts["u"], pts["v"], pts["seed"] = b[:, 1], b[:, 2], np.arange(n, dtype=np.uint32)
    pts["prim"] = np.where(rng.random(n) < 0.5, B.FRONT, 0).astype(np.uint32)
    pts["prim"][::97] = B.NONE
    d_p = _dev(pts)
    whole, st = sc.bake_gather(d_p, samples=samples, max_ray_depth=1, sum_only=True, sample_stride=n)
    assert st["pixels"] == n * samples
    cut = n // 2 + 11
    parts = [sc.bake_gather(d_p[a:b_].contiguous(), samples=samples, max_ray_depth=1, sum_only=True, sample_stride=n)[0] for a, b_ in ((0, cut), (cut, n))]
    whole, halves = whole.cpu().numpy(), torch.cat(parts).cpu().numpy()
    assert B.same_bits(whole, halves), _bad_rows(whole, halves)
    # Closed form: nothing can be hit from the scene's only triangle, so every path brings back the sky's 1, 1, 1 (ray.rs:184-193) and
    # a running sum that held p ends at ((p + 1) + 1) + 1 -- exact in f32 for small integers.  Every point gets its own p mod 251, so
    # a point lost, doubled or shifted at the boundary shows, and so does a sample lost from the point that spans it.
    none = pts["prim"] == B.NONE
    pre = np.repeat((np.arange(n) % 251).astype(np.float32)[:, None], 3, axis=1)
    acc = torch.from_numpy(pre.copy()).cuda()
    sc.bake_gather(d_p, samples=samples, max_ray_depth=1, sample_stride=n, accumulate_into=acc)
    want = np.where(none[:, None], pre, pre + np.float32(samples))
    assert B.same_bits(acc.cpu().numpy(), want), _bad_rows(acc.cpu().numpy(), want)
    assert B.same_bits(whole, np.where(none[:, None], np.float32(0), np.float32(samples)) * np.ones((1, 3), np.float32))
    straddler = (1 << 22) // samples                                                       # its samples lie on both sides of the boundary
    assert not none[straddler] and straddler * samples < (1 << 22) < (straddler + 1) * samples


def test_bake_lightmap_is_texels_then_gather(rrt, orc):
    base = _base_scene(rrt, "wgsl_pbr")
    v = base.tris["vertices"]                                                               # the atrium's UVs tile the atlas: shrink them into a chart
    v["tex_coord_x"], v["tex_coord_y"] = v["tex_coord_x"] * np.float32(0.2) + np.float32(0.1), v["tex_coord_y"] * np.float32(0.15) + np.float32(0.2)
    rng = np.random.default_rng(31)
    sc, caller = _from_triangles(rrt, base.tris[rng.permutation(len(base.tris))], base.materials, base.textures)
    g = B.Gather(orc, sc, caller)
    w = h = 16
    want_pts, winfo = B.texels(caller, w, h)
    assert 4 * winfo["covered"] >= w * h and 10 * (w * h - winfo["covered"]) >= w * h, winfo
    want = g.run(want_pts, 2, 4)                                                           # seeds = texel indices, stride = the texel count
    B.conditions(want, want_pts)
    for device in (True, False):
        atlas, covered, stats = sc.bake_lightmap(w, h, 2, device=device, max_ray_depth=4)
        if device:
            assert atlas.is_cuda and covered.is_cuda
            atlas, covered = atlas.cpu().numpy(), covered.cpu().numpy()
        assert atlas.shape == (h, w, 3) and atlas.dtype == np.float32 and covered.shape == (h, w) and covered.dtype == bool
        assert np.array_equal(covered.reshape(-1), want_pts["prim"] != B.NONE)
        assert B.same_bits(atlas.reshape(-1, 3), want["mean"]), (device, _bad_rows(atlas.reshape(-1, 3), want["mean"]))
        assert stats["texels"]["covered_texels"] == winfo["covered"] and stats["pixels"] == 2 * w * h
