"""GPU: mipt_bake_texels / mipt_bake_gather and their _device forms (csrc/bake.hip, csrc/mipt_bake.cpp) against the models of
tests/tools/bake_model.py: the texel pass as a numpy f32 brute force over all triangles, the gather as a Python loop over the oracle's
one-ray entries.  Every comparison is on the bytes.  Scenes are built on the device from a shuffled triangle array, so that the
tree's order is not the caller's; the culled arm of the gather runs at margin 0 here and at MIPT_CULL_MARGIN_SAFE, with counters and
hard points, in tests/test_gpu_bake_hard.py.
The last part takes the texel kernels where no small layout does: past the lanes of their grids, past the
list of cover_huge_kernel, to atlas sides of 2^19, onto slivers the box clause decides and onto a scene without an order array;
there the model is B.texels_indexed, which tests/test_bake_model.py holds to the brute force, and each test asserts on the model
alone that its input is what it is for, printing the figures and what each phase took ("[bake] ...", shown with -s)."""
import ctypes as C
import os
import sys
import time

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


def _soup(rrt, n, seed=1, size=0.3):
    """n small triangles scattered in a box, normals up, UVs far outside the atlas (around (7, 7)): fillers that cover nothing"""
    from rust_ray_tracing_amd import _lib as L
    rng = np.random.default_rng(seed)
    t = np.zeros(n, dtype=L.TRIANGLE)
    c = rng.uniform(-4, 4, (n, 1, 3))
    t["vertices"]["position"] = (c + rng.uniform(-size, size, (n, 3, 3))).astype(np.float32)
    t["vertices"]["normal"] = (0, 1, 0)
    uv = 7.0 + rng.uniform(0, 0.5, (n, 3, 2))
    t["vertices"]["tex_coord_x"], t["vertices"]["tex_coord_y"] = uv[..., 0].astype(np.float32), uv[..., 1].astype(np.float32)
    return t


def _set_uv(tris, k, uv):
    tris["vertices"]["tex_coord_x"][k], tris["vertices"]["tex_coord_y"][k] = np.float32(uv)[:, 0], np.float32(uv)[:, 1]


def _layout_tris(rrt, layout, n=64, seed=1):
    """the soup with the UV triangles of `layout` ({caller index: 3 x 2}) set"""
    tris = _soup(rrt, n, seed)
    for k, uv in layout.items():
        _set_uv(tris, k, uv)
    return tris


def _uv_scene(rrt, layout, n=64, seed=1):
    return _from_triangles(rrt, _layout_tris(rrt, layout, n, seed), [rrt.material_default()])


# The small layouts, at module level: tests/test_bake_model.py (CPU) holds the second statement of the model to the first on each.
QUAD = {20: [(0, 0), (1, 0), (1, 1)], 41: [(0, 0), (1, 1), (0, 1)]}     # two triangles over the unit square, the diagonal shared
QUAD_SIZES = [(8, 8), (7, 5), (32, 32), (1, 1)]
IDENTICAL_TRI = [(0.1, 0.1), (0.9, 0.2), (0.3, 0.95)]
_NAN = float("nan")
DEGENERATE = {3: [(0.2, 0.2), (0.6, 0.6), (0.4, 0.4)],                   # collinear and exactly representable differences: d == 0
              9: [(0.5, 0.5), (0.5, 0.5), (0.5, 0.5)],                   # a point
              17: [(0.1, _NAN), (0.8, 0.1), (0.1, 0.8)],                 # a NaN corner
              30: [(0.5, -0.5), (1.5, 0.5), (0.5, 1.5)],                 # half outside [0, 1]
              44: [(0.05, 0.3), (0.45, 0.35), (0.1, 0.9)]}


def _quad_layout(w, h):
    """the quad scaled into the atlas, except at 1 x 1, whose one centre lies on the diagonal of the unscaled quad"""
    return {k: np.float32(v) * np.float32(0.75) + np.float32(0.125) for k, v in QUAD.items()} if (w, h) != (1, 1) else QUAD


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


def _check_texels(rrt, sc, caller, w, h, main=True, index=None, model=None):
    """both entries against `model` = (records, info), by default B.texels of the texels `index` (all of them)"""
    want, winfo = model if model is not None else B.texels(caller, w, h, index)
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
@pytest.mark.parametrize("w,h", QUAD_SIZES)
def test_texels_quad(rrt, w, h):
    """8x8: the shared diagonal runs through texel centres, which both triangles cover (u == 0 for one, u + v == 1 for the other):
    the lower index gets them.  7x5: odd and not square.  32x32: boxes above 64 texels, the wave's walk.  1x1: one centre, on the
    diagonal of the unscaled quad."""
    sc, caller = _uv_scene(rrt, _quad_layout(w, h))
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
    sc, caller = _uv_scene(rrt, {i: IDENTICAL_TRI, j: IDENTICAL_TRI})
    assert np.array_equal(sc._tri_order, probe._tri_order) and pos[i] > pos[j]        # the lower index comes LATER in tree order
    want, _ = _check_texels(rrt, sc, caller, 16, 16)
    assert set((want["prim"][want["prim"] != B.NONE] & B.TRI_MASK).tolist()) == {i}


def test_texels_degenerate_nan_and_outside(rrt):
    sc, caller = _uv_scene(rrt, DEGENERATE)
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
    sc, caller = _uv_scene(rrt, _quad_layout(w, h))
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
            d_out=None, extra=4, cull_margin=0.0):
    """One call of the C entry with a sentinel behind the output -> (rc, radiance [n, 3] f32, stats dict); the sentinel is asserted"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = lib or rrt.load()
    n = len(points)
    opt = L.MiptBakeOptions()
    opt.samples, opt.max_ray_depth, opt.traversal, opt.cull_margin, opt.shading, opt.flags = samples, depth, traversal, cull_margin, shading, flags
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


def test_gather_points_longer_than_a_chunk(rrt, orc):
    """Four points of 2^22 + 2^21 + 7 samples each at depth 1, the third of them no point: whole chunks inside one point and straddles
    at different offsets, so both carry slots are written and read more than once.  Against the same entry in SUM | ACCUM calls of at
    most 2^21 samples: 2^21 divides a chunk, so no point of such a call crosses one, and such calls are on the path the small cases
    hold to the model.  The three real points see the box's light (chosen on the CPU: their sums are no whole numbers, so the order
    of the additions shows)."""
    import torch
    from rust_ray_tracing_amd import _lib as L
    sc, _, _, pts = _case(rrt, orc, "cornell")
    four = pts[[0, 1, 14, 2]].copy()
    assert four["prim"][2] == B.NONE and np.all(four["prim"][[0, 1, 3]] != B.NONE)
    per = (1 << 22) + (1 << 21) + 7
    assert per > (1 << 22) and len({(k * per) % (1 << 22) for k in (1, 2, 3)}) == 3 and (1 << 22) % (1 << 21) == 0
    rc, whole, st = _gather(rrt, sc, four, per, 1, flags=L.FLAG_SUM, device=True, stride=4)
    assert rc == 0 and st["pixels"] == 4 * per                                           # a NONE point's placeholder paths count
    d_acc = torch.zeros((4 * 3 + 4,), dtype=torch.float32, device="cuda").view(torch.int32)
    d_acc[4 * 3:] = SENTINEL
    first = 0
    while first < per:
        k = min(1 << 21, per - first)
        rc, parts, _ = _gather(rrt, sc, four, k, 1, flags=L.FLAG_SUM | L.FLAG_ACCUM, device=True, stride=4, first_sample=first, d_out=d_acc)
        assert rc == 0                                                                    # (_gather asserts the sentinels)
        first += k
    real = whole[[0, 1, 3]]
    assert np.all(np.isfinite(real)) and np.all(real > 0) and not B.same_bits(real[0], real[1]) and not B.same_bits(real[1], real[2])
    assert not whole[2].view(np.uint32).any() and not parts[2].view(np.uint32).any()      # +0, bit for bit
    assert B.same_bits(whole, parts), _bad_rows(whole, parts)


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


# ---- the texel kernels where no small layout takes them ---------------------------------------------------------------------------------
# Restated from csrc/bake.hip (kLaneTexels, kWaveTexels) and csrc/mipt_bake.cpp (kHugeCap): edit together with them.
K_LANE_TEXELS, K_WAVE_TEXELS, K_HUGE_CAP = 64, 1 << 16, 8192
# The kernel classes a triangle by the box it walks, not by the exact one: per axis the exact range of centres, widened by pad = 1
# a side, and by one more where the float estimate of an end rounds across an integer (sides below 2^19) -- at most 4 more a side.
BOX_SLACK = 4
N_SAMPLED = 4096


def _timed(name, t0, **figures):
    """one line per phase for the log: what each new test spends where, and the values its conditions took"""
    print(f"[bake] {name}: {time.perf_counter() - t0:.2f} s " + " ".join(f"{k}={v}" for k, v in figures.items()), flush=True)


def _classes(tris, w, h):
    """0 lane / 1 wave / 2 huge per triangle by the model's exact boxes, -1 where the kernel's box could fall into another class"""
    x0, x1, y0, y1, _ = B.boxes(tris, w, h)
    nx, ny = x1 - x0, y1 - y0
    exact, most = nx * ny, (nx + BOX_SLACK) * (ny + BOX_SLACK)
    cls = np.full(len(tris), -1)
    cls[most <= K_LANE_TEXELS] = 0
    cls[(exact > K_LANE_TEXELS) & (most <= K_WAVE_TEXELS)] = 1
    cls[exact > K_WAVE_TEXELS] = 2
    return cls


# -- slivers the box clause decides
SLIVERS = [(64, 1, 64), (96, 2, 128), (100, 2, 128)]                 # side, k, count
SLIVER_SEED = 4                                                      # chosen on the CPU: 44, 56 and 58 texels change owner without the clause


def _sliver_tris(rrt, w, h, n, k, seed=SLIVER_SEED):
    tris = _soup(rrt, n, seed=3)
    uv = B.sliver_uvs(w, h, n, k, seed)
    tris["vertices"]["tex_coord_x"], tris["vertices"]["tex_coord_y"] = uv[..., 0], uv[..., 1]
    return tris


@pytest.mark.parametrize("side,k,n", SLIVERS)
def test_texels_slivers_that_the_box_clause_decides(rrt, side, k, n):
    """Slivers along lines of texel centres (B.sliver_uvs): centres OUTSIDE a sliver's box, which the kernel's padded walk visits, pass
    u >= 0, v >= 0, u + v <= 1 by rounding noise, and only the four box comparisons of covers() keep them out.  A power-of-two side
    and two whose centres are not representable; a good part of the slivers has d == 0, so the ballot that counts unusable
    triangles sees mixed waves."""
    t0 = time.perf_counter()
    sc, caller = _from_triangles(rrt, _sliver_tris(rrt, side, side, n, k), [rrt.material_default()])
    want, winfo = B.texels(caller, side, side)
    loose, _ = B.texels(caller, side, side, box=False)
    decided = int((want["prim"] != loose["prim"]).sum())
    _timed(f"slivers {side}: model", t0, decided=decided, covered=winfo["covered"], unusable=winfo["degenerate"])
    assert decided >= 16 and winfo["covered"] >= 100 and 4 <= winfo["degenerate"] <= n // 2
    t0 = time.perf_counter()
    _check_texels(rrt, sc, caller, side, side, main=False, model=(want, winfo))
    _timed(f"slivers {side}: gpu", t0)


# -- cover_kernel and invert_order_kernel past the lanes of their grids
BIG_W, BIG_H = 768, 640
BIG_SOUP_SIZE = 0.02                                                 # chosen on the CPU: with it the model alone meets B.conditions


def _big_uvs(n, seed=12):
    """[n, 3, 2] f32 on the BIG_W x BIG_H atlas, three classes by box size mixed inside every run of 64 indices: mostly triangles
    within 1.8 texels of their centre (the lane's loop), every 16th with a box of 9 ... 60 texels a side (the wave's walk), 20 among
    the lowest and 20 among the highest 640 indices thin and long across a box of more than 2^16 texels (the list).  The small ones
    stay left of 0.78 of the width: the right of the atlas is bare but for the long ones, which so own texels there whatever
    their index.  Two in a thousand are unusable (a NaN corner; two equal corners, d == 0 exactly)."""
    rng = np.random.default_rng(seed)
    w, h = BIG_W, BIG_H
    kind = np.zeros(n, dtype=np.int8)
    kind[5::16] = 1
    kind[np.concatenate([rng.choice(640, 20, replace=False), n - 1 - rng.choice(640, 20, replace=False)])] = 2
    c = rng.uniform((0.05 * w, 0.05 * h), (0.78 * w, 0.95 * h), (n, 2))                    # in texels
    off = rng.uniform(-1.8, 1.8, (n, 3, 2))
    r = rng.uniform(4.6, 7.0, n)
    wide = (np.arange(n) // 16) % 64 == 9
    r[wide] = rng.uniform(7.0, 30.0, int(wide.sum()))
    f = rng.uniform(-1, 1, (n, 2))
    box = np.stack([np.stack([-r, -r], -1), np.stack([r, r * f[:, 0]], -1), np.stack([r * f[:, 1], r], -1)], axis=1)      # exactly 2r x 2r
    uv = c[:, None, :] + np.where((kind == 1)[:, None, None], box, off)
    k = np.flatnonzero(kind == 2)
    a = np.stack([rng.uniform(0.50 * w, 0.56 * w, len(k)), rng.uniform(0.05 * h, 0.30 * h, len(k))], -1)
    b = a + np.stack([rng.uniform(300, 330, len(k)), rng.uniform(225, 240, len(k))], -1)
    third = a + np.stack([rng.uniform(3, 6, len(k)), np.zeros(len(k))], -1)
    flip = rng.random(len(k)) < 0.5                                                         # the other diagonal
    a[flip, 1], b[flip, 1] = b[flip, 1].copy(), a[flip, 1].copy()
    third[flip, 1] = a[flip, 1]
    uv[k] = np.stack([a, b, third], axis=1)
    uv = (uv / np.array([w, h], dtype=np.float64)).astype(np.float32)
    uv[777::1001, 1, 0] = np.nan
    uv[300::997, 2] = uv[300::997, 1]
    return uv


_big = {}


def _big_case(rrt):
    """One scene of 2 lanes_cap + 4 099 triangles (no multiple of 64: the last wave is ragged), built on the device with its tree
    mirrored and shared by the two tests below: every lane of cover_kernel and of invert_order_kernel takes a third trip.  The
    positions are a soup drawn index by index, so the array is in no spatial order and the tree's order is not the caller's."""
    if not _big:
        t0 = time.perf_counter()
        cap = LT.lanes_cap(LT.device_n_cu())
        n = 2 * cap + 4099
        assert n % 64 != 0
        tris = _soup(rrt, n, seed=14, size=BIG_SOUP_SIZE)
        uv = _big_uvs(n)
        tris["vertices"]["tex_coord_x"], tris["vertices"]["tex_coord_y"] = uv[..., 0], uv[..., 1]
        sc, caller = _from_triangles(rrt, tris, [rrt.material_default()])
        pos = np.empty(n, dtype=np.int64)
        pos[sc._tri_order] = np.arange(n)                            # caller index -> tree position
        _big.update(sc=sc, caller=caller, cap=cap, pos=pos)
        _timed("big: scene", t0, triangles=n, lanes_cap=cap)
    return _big


def test_texels_past_the_lanes_of_cover_kernel(rrt):
    """cover_kernel's grid-stride loop over the triangles, all three classes of box in every trip, against B.texels_indexed on every
    byte; 4 096 seeded texels against the brute force as well, which ties the second statement of the model to the first at this size."""
    big = _big_case(rrt)
    sc, caller, cap, pos = big["sc"], big["caller"], big["cap"], big["pos"]
    n, w, h = len(caller), BIG_W, BIG_H
    t0 = time.perf_counter()
    stats = {}
    want, winfo = B.texels_indexed(caller, w, h, stats=stats)
    _timed("big: indexed model", t0, pairs=stats["pairs"], covered=winfo["covered"], unusable=winfo["degenerate"])
    # conditions, on the model alone
    cls = _classes(caller, w, h)
    assert not np.any(cls < 0) and int((cls == 2).sum()) >= 36
    assert 4 * winfo["covered"] >= w * h and 10 * winfo["covered"] <= 9 * w * h, winfo
    assert winfo["degenerate"] >= 64
    late = pos >= cap
    owned = [int(stats["owned"][(cls == c) & late].sum()) for c in (0, 1, 2)]
    huge_owners = int(((stats["owned"] > 0) & (cls == 2) & late).sum())
    by_wave = np.zeros((-(-n // 64), 3), dtype=bool)
    by_wave[pos // 64, cls] = True
    mixed = int(by_wave.all(axis=1).sum())
    _timed("big: conditions", t0, owned_past_cap_lane_wave_huge=owned, huge_owners_past_cap=huge_owners, waves_of_all_three=mixed)
    assert owned[0] >= 1000 and owned[1] >= 1000 and huge_owners >= 1 and mixed >= 1
    t0 = time.perf_counter()
    _check_texels(rrt, sc, caller, w, h, main=False, model=(want, winfo))
    _timed("big: gpu, both entries", t0)
    t0 = time.perf_counter()
    index = np.sort(np.random.default_rng(15).choice(w * h, N_SAMPLED, replace=False)).astype(np.uint32)
    brute, _ = B.texels(caller, w, h, index)
    _timed("big: brute force on 4096 texels", t0)
    assert B.same_bits(brute, want[index]), _bad_texels(want[index], brute)
    got, _ = _texels(rrt, sc, w, h)
    assert B.same_bits(got[index], brute), _bad_texels(got[index], brute)


def test_gather_past_the_lanes_of_invert_order_kernel(rrt, orc):
    """The map caller index -> tri_pos record is made by a grid-stride loop over the RECORDS: half of the points lie on triangles whose
    record index is at or above the lanes a launch holds, half below.  The record of a triangle is read from the host's restatement of
    the layout (word 9 of a record is its triangle's tree index), not from the device."""
    big = _big_case(rrt)
    sc, caller, cap, pos = big["sc"], big["caller"], big["cap"], big["pos"]
    n = len(caller)
    t0 = time.perf_counter()
    geom, _, info = sc.host_layout()
    first = info["n_pair_records"] * 64
    tree_of_record = geom[first: first + n * 64].view(np.uint32).reshape(n, 16)[:, 9].astype(np.int64)
    assert np.array_equal(np.sort(tree_of_record), np.arange(n))
    record = np.empty(n, dtype=np.int64)
    record[tree_of_record] = np.arange(n)
    record = record[pos]                                             # caller index -> record
    assert not np.array_equal(record, pos)                           # the records are not in tree order
    pts = _random_points(caller, 192, 17)
    rng = np.random.default_rng(18)
    tri = np.where(np.arange(192) % 2 == 0, rng.choice(np.flatnonzero(record >= cap), 192), rng.choice(np.flatnonzero(record < cap), 192))
    real = pts["prim"] != B.NONE
    pts["prim"][real] = (pts["prim"][real] & np.uint32(B.FRONT)) | tri[real].astype(np.uint32)
    q = record[pts["prim"][real] & B.TRI_MASK]
    assert 3 * int((q >= cap).sum()) >= 192 and 3 * int((q < cap).sum()) >= 192
    _timed("big gather: layout and points", t0, records_past_cap=int((q >= cap).sum()), below=int((q < cap).sum()))
    t0 = time.perf_counter()
    want = B.Gather(orc, sc, caller).run(pts, 2, 3)
    B.conditions(want, pts)
    _timed("big gather: model", t0, first_hits=int(want["first_hit"].sum()), of=2 * int(real.sum()))
    t0 = time.perf_counter()
    for traversal, device in ((REF, False), (CULL, False), (REF, True)):
        model = want if traversal == REF else B.Gather(orc, sc, caller).run(pts, 2, 3, cull=1)
        rc, got, _ = _gather(rrt, sc, pts, 2, 3, traversal=traversal, device=device)
        assert rc == 0 and B.same_bits(got, model["mean"]), (traversal, device, _bad_rows(got, model["mean"]))
    _timed("big gather: gpu", t0)


# -- more huge triangles than the list holds
FULL_W, FULL_H = 384, 320
FULL_HUGE, FULL_SMALL, FULL_EDGE = K_HUGE_CAP + 300, 64, 300


def _full_list_uvs(seed=21):
    """[FULL_HUGE + FULL_SMALL, 3, 2] f32 on the FULL_W x FULL_H atlas: thin wedges, a texel or a few wide at one end and a point at
    the other, each across a box of about 300 x 230 texels, either diagonal, at their own offsets, with 64 triangles of a few texels
    spread through the order.  Wedges start at their wide end and run down the atlas; those of the highest FULL_EDGE indices start in
    rows 2 ... 22, the others below row 24, so the highest indices own texels nobody else covers."""
    rng = np.random.default_rng(seed)
    n, w, h = FULL_HUGE + FULL_SMALL, FULL_W, FULL_H
    small = 7 + 129 * np.arange(FULL_SMALL)
    assert small[-1] < n - FULL_EDGE
    top = np.arange(n) >= n - FULL_EDGE
    a = np.stack([rng.uniform(2, 75, n), np.where(top, rng.uniform(2, 6, n), rng.uniform(24, 85, n))], -1)
    b = a + np.stack([rng.uniform(300, 305, n), rng.uniform(226, 232, n)], -1)
    third = a + np.stack([np.where(top, rng.uniform(1.0, 1.5, n), rng.uniform(2, 5, n)), np.zeros(n)], -1)
    flip = (rng.random(n) < 0.5) & ~top                                                     # the other diagonal: wide at the bottom left
    a[flip, 1], b[flip, 1] = b[flip, 1].copy(), a[flip, 1].copy()
    third[flip, 1] = a[flip, 1]
    uv = np.stack([a, b, third], axis=1)
    c = rng.uniform((5, 5), (w - 5, h - 5), (FULL_SMALL, 2))
    uv[small] = c[:, None, :] + rng.uniform(-2.5, 2.5, (FULL_SMALL, 3, 2))
    return (uv / np.array([w, h], dtype=np.float64)).astype(np.float32), small


def _merge(first, second, cut):
    """texel records of the scenes caller[:cut] and caller[cut:] -> those of the whole array: per texel the lower caller index"""
    out = first.copy()
    take = first["prim"] == B.NONE
    out[take] = second[take]
    has = take & (second["prim"] != B.NONE)
    out["prim"][has] = ((second["prim"][has] & np.uint32(B.TRI_MASK)) + np.uint32(cut)) | np.uint32(B.FRONT)
    return out


def test_texels_with_more_huge_triangles_than_the_list_holds(rrt):
    """kHugeCap + 300 triangles whose box holds more than 2^16 texels: the list of cover_huge_kernel fills, 300 of them (which ones is
    up to the order of an atomicAdd) are walked by their wave, and cover_huge_kernel clamps a counter that ran past the cap.  A full
    model would be 5.6e8 (triangle, texel) pairs, so: (a) 4 096 seeded texels against the brute force; (b) every texel against the
    merge of the same entry on the two halves of the array, each below the cap and so on the path the 256 x 256 test holds to
    the model -- u, v are a function of texel and triangle alone, so the merge is exact; (c) covered_texels is the count of (b).
    Twice, with equal bytes: the result may not depend on who overflowed."""
    t0 = time.perf_counter()
    w, h = FULL_W, FULL_H
    uv, small = _full_list_uvs()
    n = len(uv)
    tris = _soup(rrt, n, seed=22)
    tris["vertices"]["tex_coord_x"], tris["vertices"]["tex_coord_y"] = uv[..., 0], uv[..., 1]
    x0, x1, y0, y1, usable = B.boxes(tris, w, h)
    huge = (x1 - x0) * (y1 - y0) > K_WAVE_TEXELS                     # the centres in the exact box; the kernel's padded box is no smaller
    assert int(huge.sum()) >= K_HUGE_CAP + 256 and usable.all() and not huge[small].any()
    index = np.sort(np.random.default_rng(23).choice(w * h, N_SAMPLED, replace=False)).astype(np.uint32)
    brute, binfo = B.texels(tris, w, h, index)
    owners = np.unique(brute["prim"][brute["prim"] != B.NONE] & B.TRI_MASK).astype(np.int64)
    owners = owners[huge[owners]]
    figures = dict(boxes_above_2_16=int(huge.sum()), sampled_owners=len(owners), top=int((owners >= n - FULL_EDGE).sum()),
                   bottom=int((owners < FULL_EDGE).sum()), sampled_covered=binfo["covered"])
    _timed("full list: model", t0, **figures)
    assert len(owners) >= 64 and figures["top"] >= 8 and figures["bottom"] >= 8
    t0 = time.perf_counter()
    sc, caller = _from_triangles(rrt, tris, [rrt.material_default()])
    cut = n // 2
    assert int(huge[:cut].sum()) < K_HUGE_CAP and int(huge[cut:].sum()) < K_HUGE_CAP
    halves = [_from_triangles(rrt, caller[a:b], [rrt.material_default()])[0] for a, b in ((0, cut), (cut, n))]
    for device in (False, True):
        merged = _merge(*[_texels(rrt, half, w, h, device)[0] for half in halves], cut)
        covered = int((merged["prim"] != B.NONE).sum())
        assert 4 * covered >= w * h and B.same_bits(merged[index], brute)                 # the reference itself, on the sampled texels
        for again in (0, 1):
            got, info = _texels(rrt, sc, w, h, device)
            assert B.same_bits(got[index], brute), (device, again, _bad_texels(got[index], brute))
            assert B.same_bits(got, merged), (device, again, _bad_texels(got, merged))
            assert info["covered_texels"] == covered and info["degenerate_tris"] == 0
    _timed("full list: gpu", t0, covered=covered)


# -- atlas sides around 2^19, where span()'s padding grows and its float estimate is off by a visible part of a texel
LONG = 1 << 19
LONG_ATLASES = [(LONG + 3, 3), (3, LONG + 3), (LONG - 1, 2)]         # pad 2 along x; pad 2 along y; the largest side with pad 1


def _unsteady_centres(size):
    """[(column, at_hi)]: the centres c whose product with the side does not round back to c + 0.5 in f32, between columns 40 and
    size - 41.  Only there can an estimate `lo * size - 0.5` of a box's end lie on the wrong side of the column that an exact
    `s == lo` (at_hi False: the product is too large) or `s == hi` (True: too small) decides, and a walk without padding lose it;
    for every lo below a steady centre the product is no larger than the centre's, since a rounded product is monotone.  Found
    here by trying every column: 146 091 and 494 253 at 2^19 + 3, none at 2^19 - 1."""
    a = np.arange(size, dtype=np.uint32).astype(np.float32) + np.float32(0.5)
    back = (a / np.float32(size)) * np.float32(size)
    return [(int(c), bool(back[c] < a[c])) for c in np.flatnonzero(back != a) if 40 <= c < size - 41]


def _long_uvs(w, h, n=4096, seed=31):
    """[n, 3, 2] f32: triangles of 1 ... 40 texels along the long side whose corners there are texel centres, so that the first and the
    last column (row) of every box is decided by an exact equality s == lo, s == hi.  A third have two corners on the first centre (an
    edge along the column of lo, across the whole short side), a third on the last, the others one corner at each end."""
    rng = np.random.default_rng(seed)
    long_axis = 0 if w >= h else 1
    size = max(w, h)
    cen = B.centre_lines(size, 1)[0]
    i = rng.integers(0, size - 41, n)
    e = rng.integers(1, 41, n)
    j = (rng.random(n) * (e + 1)).astype(np.int64)
    kind = np.arange(n) % 3
    for k, (c, at_hi) in enumerate(_unsteady_centres(size)):                               # the lowest indices: they own what they cover
        kind[k], e[k] = (1 if at_hi else 0), 7
        i[k] = c - 7 if at_hi else c
    j = np.where(kind == 0, 0, np.where(kind == 1, e, j))
    uv = np.zeros((n, 3, 2), dtype=np.float32)
    uv[:, 0, long_axis], uv[:, 1, long_axis], uv[:, 2, long_axis] = cen[i], cen[i + e], cen[i + j]
    short = rng.uniform(-0.2, 1.2, (n, 3))
    short[kind == 0, 0], short[kind == 0, 2] = -0.1, 1.1                                    # corners 0 and 2 share the first centre
    short[kind == 1, 1], short[kind == 1, 2] = -0.1, 1.1                                    # corners 1 and 2 share the last
    uv[:, :, 1 - long_axis] = short
    return uv


@pytest.mark.parametrize("w,h", LONG_ATLASES)
def test_texels_on_atlas_sides_around_2_to_19(rrt, w, h):
    """span() where its rounding argument matters: the padding is 2 from a side of 2^19 on, and the float estimate of a box's end is
    off by up to 1/32 of a texel.  Every box begins and ends on a texel centre; at 2^19 + 3 the two centres at which an unpadded walk
    would lose the column carry the first (last) column of the two lowest triangles.  At 2^19 - 1 there is no such centre, and
    nowhere is the estimate off by a whole texel: a padding of 0 is only seen at 2^19 + 3, one of 1 in place of 2 nowhere."""
    t0 = time.perf_counter()
    unsteady = _unsteady_centres(max(w, h))
    assert sorted(at_hi for _, at_hi in unsteady) == ([False, True] if max(w, h) == LONG + 3 else [])
    n = 4096
    tris = _soup(rrt, n + 64, seed=32)
    uv = _long_uvs(w, h, n)
    tris["vertices"]["tex_coord_x"][:n], tris["vertices"]["tex_coord_y"][:n] = uv[..., 0], uv[..., 1]
    want, winfo = B.texels_indexed(tris, w, h)
    # conditions, on the model alone
    has = np.flatnonzero(want["prim"] != B.NONE)
    own = (want["prim"][has] & B.TRI_MASK).astype(np.int64)
    along = B.texel_centres(w, h, has)[0 if w >= h else 1]
    c = B.corner_uvs(tris)[own][:, :, 0 if w >= h else 1]
    at_lo, at_hi = int((along == c.min(axis=1)).sum()), int((along == c.max(axis=1)).sum())
    _timed(f"long {w}x{h}: model", t0, covered=winfo["covered"], at_lo=at_lo, at_hi=at_hi)
    assert at_lo >= 256 and at_hi >= 256 and 100 * winfo["covered"] > w * h
    cen = B.centre_lines(max(w, h), 1)[0]
    for k, (col, is_hi) in enumerate(unsteady):                      # triangle k owns texels of its unsteady first (last) column
        mine = own == k
        assert int((mine & (along == cen[col]) & (along == (c.max(axis=1) if is_hi else c.min(axis=1)))).sum()) >= 2, (k, col, is_hi)
    t0 = time.perf_counter()
    sc, caller = _from_triangles(rrt, tris, [rrt.material_default()])
    _check_texels(rrt, sc, caller, w, h, main=False, model=(want, winfo))
    _timed(f"long {w}x{h}: gpu", t0)


# -- a scene that keeps the caller's tree: tri_order == NULL in cover_kernel, cover_huge_kernel and invert_order_kernel
def _own_tree_scene(rrt, tris, mats, texs=()):
    """(resident Scene created from the caller's nodes, the caller's array).  The host builder reorders the triangles; what it leaves is
    the array handed to mipt_scene_create, and its order is the caller's.  Such a scene keeps no order array: asserted, so that the
    test cannot run the other branch unnoticed."""
    sc = rrt.Scene.from_arrays(tris, mats, texs)
    assert len(sc.tris) >= 64 and not B.same_bits(sc.tris, np.ascontiguousarray(tris))
    sc.upload(0)
    assert sc._tri_order is None and sc.info()["built_on_device"] == 0
    return sc, sc.tris.copy()


def test_texels_and_gather_on_a_scene_with_the_callers_tree(rrt, orc):
    t0 = time.perf_counter()
    sc, caller = _own_tree_scene(rrt, _layout_tris(rrt, _quad_layout(24, 20)), [rrt.material_default()])
    _check_texels(rrt, sc, caller, 24, 20)
    assert sorted(_classes(caller, FULL_W, FULL_H).tolist())[-2:] == [2, 2]      # at this size both go to cover_huge_kernel's list
    _check_texels(rrt, sc, caller, FULL_W, FULL_H)
    base = _base_scene(rrt, "cornell")
    sc, caller = _own_tree_scene(rrt, base.tris, base.materials, base.textures)
    want, winfo = _check_texels(rrt, sc, caller, 24, 20, main=False)
    assert winfo["covered"] >= 24 * 20 // 4 and len(np.unique(want["prim"])) >= 2     # the box's UVs tile: two triangles own everything
    pts = _random_points(caller, 64, POINT_SEED)
    model = B.Gather(orc, sc, caller).run(pts, 2, 4)
    B.conditions(model, pts)
    for device in (False, True):
        rc, got, _ = _gather(rrt, sc, pts, 2, 4, device=device)
        assert rc == 0 and B.same_bits(got, model["mean"]), (device, _bad_rows(got, model["mean"]))
    _timed("caller's tree", t0)
