"""-m gpu: shading mode 1 (the wgpu shader's material model) on the device.

Part one: the device functions shade_wgsl inlines (csrc/pt_device_wgsl.h), evaluated element-wise through libmipt_diag.so's
mipt_debug_wgsl, must equal the C oracle's statement of the same pieces bit for bit (NaN = NaN) -- on about 10^6 random inputs
per op and on the edges where such code goes wrong.  Part two: whole renders, kernel against oracle (radiance, RGBA8, counters) on
more than the one scene of test_wgpu_material_model_matches_its_oracle.  Every case is one bounded launch; non-finite values are
data here, never addresses: the sampler's indices are checked through the oracle before anything is launched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))

OUT_FLOATS = {0: 4, 1: 6, 2: 3, 3: 3, 4: 4, 5: 3, 6: 13}
TRAVERSALS = ((0, 0.0), (1, 0.0078125), (1, 0.0))
COUNTERS = ("rays", "inner_steps", "tri_tests", "hits", "texel_fetches")


def _probe(rrt, op, rows, tex=None):
    lib = rrt.load_diag()
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    out = np.zeros((len(rows), OUT_FLOATS[op]), dtype=np.float32)
    words, w, h = None, 0, 0
    if tex is not None:
        tex = np.ascontiguousarray(tex, dtype=np.uint8)
        words, w, h = tex.view(np.uint32).reshape(-1).copy(), tex.shape[1], tex.shape[0]
    rc = lib.mipt_debug_wgsl(op, rows.ctypes.data, len(rows), None if words is None else words.ctypes.data, w, h, out.ctypes.data)
    assert rc == 0, lib.mipt_diag_last_error()
    return out


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _assert_same(got, want, what):
    same = _bits_equal(got, want)
    if not same.all():
        bad = np.argwhere(~same)[0]
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} differ, first at {tuple(bad)}: {got[tuple(bad)]!r} != {want[tuple(bad)]!r}")


def _as_bits(u32):
    return np.ascontiguousarray(u32, dtype=np.uint32).view(np.float32)


def _unstep(y):
    """The xorshift32 state whose next output is y."""
    t = y
    for _ in range(7):
        t = y ^ ((t << 5) & 0xFFFFFFFF)
    y, t = t, t
    for _ in range(2):
        t = y ^ (t >> 17)
    y, t = t, t
    for _ in range(3):
        t = y ^ ((t << 13) & 0xFFFFFFFF)
    return t


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ---- part one: the building blocks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 1), (3, 3), (16, 16), (19, 37)])          # (height, width)
def test_device_sampler_equals_oracle(rrt, orc, shape):
    h, w = shape
    rng = np.random.default_rng(h * 64 + w)
    tex = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    n = 170_000                                                               # six sizes: about 10^6 in all
    u = np.concatenate([rng.uniform(-6, 6, n // 2), rng.standard_normal(n // 4) * 1e3, rng.integers(-4096, 4096, n // 4) / 1024.0]).astype(np.float32)
    v = np.concatenate([rng.uniform(-6, 6, n // 2), rng.standard_normal(n // 4) * 1e3, rng.integers(-4096, 4096, n // 4) / 1024.0]).astype(np.float32)
    # edges: exact texel centres and texel edges over three periods, negatives, the 1e9 guard from both sides, infinities, NaN
    cx = np.concatenate([(np.arange(-w, 2 * w) + 0.5) / w, np.arange(-w, 2 * w + 1) / w])
    cy = np.concatenate([(np.arange(-h, 2 * h) + 0.5) / h, np.arange(-h, 2 * h + 1) / h])
    guard = [1e8, -1e8, 2e9, -2e9, 1e9 / w, -1e9 / w, np.nextafter(np.float32(1e9 / w), np.float32(0)), 3e38, -3e38, np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-45]
    ex = np.concatenate([cx, guard]).astype(np.float32)
    ey = np.concatenate([cy, guard]).astype(np.float32)
    gx, gy = np.meshgrid(ex, ey)
    u, v = np.concatenate([u, gx.reshape(-1)]), np.concatenate([v, gy.reshape(-1)])
    want, idx = orc.wgsl_sample_texture(tex, u, v)
    assert idx.min() >= 0 and idx.max() < w * h                               # what the guard is for -- before the launch
    got = _probe(rrt, 0, np.stack([u, v], axis=1), tex)
    _assert_same(got, want, f"sampler {w}x{h}")


def test_device_basis_and_frames_equal_oracle(rrt, orc):
    rng = np.random.default_rng(5)
    n = _unit(rng.standard_normal((1_000_000, 3))).astype(np.float32)
    thr = np.float32(0.9999999)
    edge = []
    for z in (thr, np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(2)), np.float32(1.0)):
        for sgn in (1.0, -1.0):
            for phi in (0.0, 0.9, 2.2, 4.4):
                s = np.sqrt(max(0.0, 1.0 - float(z) ** 2))
                edge.append((s * np.cos(phi), s * np.sin(phi), sgn * float(z)))
    edge += [(0, 0, 0), (0, 0, 1), (0, 0, -1), (1, 0, 0), (0, 1, 0), (np.nan, 0, 1), (np.inf, 0, 0), (1e-30, 0, 0), (3, 4, 12)]
    n = np.concatenate([n, np.array(edge, np.float32)])
    t, b = orc.wgsl_onb(n)
    _assert_same(_probe(rrt, 1, n), np.concatenate([t, b], axis=1), "build_onb")
    l = rng.standard_normal(n.shape).astype(np.float32)
    for op in (0, 1):
        _assert_same(_probe(rrt, 2 + op, np.concatenate([n, l], axis=1)), orc.wgsl_frame(op, n, l), "to_world" if op == 0 else "to_local")


def test_device_vndf_equals_oracle(rrt, orc):
    rng = np.random.default_rng(6)
    m = 1_000_000
    ve = _unit(rng.standard_normal((m, 3)))
    ve[:, 2] = np.abs(ve[:, 2])
    alpha = rng.choice([1e-4, 1e-3, 0.05, 0.3, 1.0], m)
    seeds = rng.integers(1, 2 ** 32, m, dtype=np.uint64).astype(np.uint32)
    # edges: view along +-z (lensq == 0), grazing, alpha at both ends of its clamp, the draws at 0 (state 0) and at 1
    u1_one = _unstep(0xFFFFFFFF)                                              # first draw rounds to exactly 1
    u2_one = _unstep(_unstep(0xFFFFFFC0))                                     # second draw rounds to exactly 1
    e_ve = [(0, 0, 1), (0, 0, -1), (1, 0, 0), (0, 1, 0), (1, 0, 1e-7), (-0.6, 0.8, 1e-4), (0.6, 0, 0.8), (0, 0, 0), (1e-20, 0, 1)]
    e_seed = [0, u1_one, u2_one, 1, 0x80000000, 0xFFFFFFFF, 12345]
    e_alpha = [1e-4, 1.0]
    rows = [(v, a, s) for v in e_ve for a in e_alpha for s in e_seed]
    ve = np.concatenate([ve, np.array([r[0] for r in rows], np.float64)]).astype(np.float32)
    alpha = np.concatenate([alpha, [r[1] for r in rows]]).astype(np.float32)
    seeds = np.concatenate([seeds, np.array([r[2] for r in rows], np.uint32)])
    want, state = orc.wgsl_vndf(ve, alpha, alpha, seeds, return_state=True)
    got = _probe(rrt, 4, np.concatenate([ve, alpha[:, None], alpha[:, None], _as_bits(seeds)[:, None]], axis=1))
    _assert_same(got[:, :3], want, "sample_ggx_vndf")
    assert np.array_equal(got[:, 3].view(np.uint32), state)                   # two draws each
    lib = orc.load()
    st = C.c_uint32(u1_one)
    assert lib.orc_rand_f32(C.byref(st)) == 1.0                               # rand_f32 is inclusive of 1: the edge above is real


def test_device_cosine_hemisphere_equals_oracle(rrt, orc):
    rng = np.random.default_rng(7)
    m = 1_000_000
    ux = (rng.integers(1, 2 ** 32, m, dtype=np.uint64).astype(np.float32) / np.float32(4294967296.0))     # rand_f32's own value set
    uy = (rng.integers(1, 2 ** 32, m, dtype=np.uint64).astype(np.float32) / np.float32(4294967296.0))
    # edges: u_offset exactly zero, |ox| == |oy| in all four quadrants, ox == 0, oy == 0, the draws at 0 and at 1
    e = [(0.5, 0.5), (0.75, 0.75), (0.25, 0.75), (0.75, 0.25), (0.25, 0.25), (0.5, 0.3), (0.5, 0.9), (0.3, 0.5), (0.9, 0.5),
         (0, 0), (1, 1), (0, 1), (1, 0), (0, 0.5), (0.5, 0), (1, 0.5), (0.5, 1), (2.3283064e-10, 2.3283064e-10), (0.5, 0.50000006), (0.50000006, 0.5)]
    ux = np.concatenate([ux, [a for a, _ in e]]).astype(np.float32)
    uy = np.concatenate([uy, [b for _, b in e]]).astype(np.float32)
    _assert_same(_probe(rrt, 5, np.stack([ux, uy], axis=1)), orc.wgsl_cosine_from(ux, uy), "cosine_hemisphere_from")


def test_device_fresnel_reflect_refract_equal_oracle(rrt, orc):
    rng = np.random.default_rng(8)
    m = 1_000_000
    d = _unit(rng.standard_normal((m, 3)))
    n = _unit(rng.standard_normal((m, 3)))
    eta = rng.choice([1 / 2.4, 1 / 1.5, 1 / 1.33, 0.7, 1.0, 1.33, 1.5, 2.4], m)
    met = rng.choice([0.0, 0.3, 1.0], m)
    base = rng.random((m, 3))
    # edges: refraction with k just either side of 0 (the critical angle of eta = 1.5 and 2.4, +- a few ulps of the angle), a zero
    # normal, normal and grazing incidence
    ed, en, ee = [], [], []
    for e_ in (1.5, 2.4):
        crit = np.arcsin(1.0 / e_)
        for dth in (-1e-3, -1e-6, -1e-7, 0.0, 1e-7, 1e-6, 1e-3):
            th = crit + dth
            ed.append((np.sin(th), 0.0, -np.cos(th))); en.append((0, 0, 1)); ee.append(e_)
    for dd, nn in (((0, 0, -1), (0, 0, 1)), ((1, 0, 0), (0, 0, 1)), ((0, 0, -1), (0, 0, 0)), ((0, 0, 1), (0, 0, 1)), ((0.6, 0, -0.8), (0, 0, 1))):
        for e_ in (1 / 1.5, 1.0, 1.5):
            ed.append(dd); en.append(nn); ee.append(e_)
    k = len(ed)
    d = np.concatenate([d, np.array(ed, np.float64)]).astype(np.float32)
    n = np.concatenate([n, np.array(en, np.float64)]).astype(np.float32)
    eta = np.concatenate([eta, ee]).astype(np.float32)
    met = np.concatenate([met, np.zeros(k)]).astype(np.float32)
    base = np.concatenate([base, np.full((k, 3), 0.5)]).astype(np.float32)
    want = orc.wgsl_fresnel_step(d, n, eta, met, base)
    assert (want["k"][m:m + 14] < 0).any() and (want["k"][m:m + 14] > 0).any()        # both sides of k = 0 are among the edges
    got = _probe(rrt, 6, np.concatenate([d, n, eta[:, None], met[:, None], base], axis=1))
    _assert_same(got, want["raw"], "fresnel / reflect / refract")


# ---- part two: whole renders --------------------------------------------------------------------------------------------------------
def _render(rrt, sc, w, h, spp, depth, **kw):
    r = rrt.Renderer.new(rrt.RendererOptions(samples=spp, max_ray_depth=depth, output_image_dimensions=(w, h),
                                             output_image_path="/dev/null", shading=rrt.SHADING_WGPU, **kw))
    return r.render_buffers(sc, flags=rrt.FLAG_COUNT)


def _parity(rrt, orc, sc, w, h, spp, depth, what, tris=None, nodes=None):
    tris = sc.tris if tris is None else tris
    nodes = sc.bvh_nodes if nodes is None else nodes
    stats = None
    for trav, margin in TRAVERSALS:
        hdr, rgba, st = _render(rrt, sc, w, h, spp, depth, traversal=trav, cull_margin=margin)
        ref, ref_rgba, rst = orc.render(tris, nodes, sc.materials_array(), sc.textures, sc.camera.uniform, w, h, spp, depth,
                                        cull=trav, cull_margin=margin, shading=1)
        same = _bits_equal(hdr, ref)
        assert same.all(), (what, trav, margin, int((~same).sum()))
        assert np.array_equal(rgba, ref_rgba), (what, trav, margin)
        for k in COUNTERS:
            assert st[k] == rst[k], (what, k, trav, margin, st[k], rst[k])
        stats = rst
    return stats


@pytest.mark.parametrize("case", ["glass_dragon_1.5", "glass_helmet_2.4", "odd_textures", "depth_1", "depth_3", "depth_4", "depth_5"])
def test_mode1_scenes_match_oracle(rrt, orc, case):
    """The scenes of tests/test_wgsl_second_reading.py -- refraction with Beer absorption and total internal reflection, odd-sized
    textures with a normal map in every material, the depth limits that bracket the start of roulette -- at full small-frame size."""
    import wgsl_scenes as S
    if case.startswith("glass_dragon"):
        sc, depth = S.glass_scene(rrt, "dragon", 30000, ior=1.5), 16
    elif case.startswith("glass_helmet"):
        sc, depth = S.glass_scene(rrt, "helmet", 4000, ior=2.4, roughness=0.05), 16
    elif case == "odd_textures":
        sc, depth = S.odd_texture_scene(rrt, "helmet", 4000), 12
    else:
        sc, depth = S.pbr_scene(rrt, n_target=20000, tex_size=16), int(case.split("_")[1])
    st = _parity(rrt, orc, sc, 96, 54, 3, depth, case)
    assert st["hits"] > 0 and (depth == 1 or st["rays"] > 96 * 54 * 3)


@pytest.mark.parametrize("seed", range(12))
def test_mode1_fuzz_random_scenes_match_oracle(rrt, orc, seed):
    """test_fuzz_random_scenes_match_oracle for shading mode 1: random soups with degenerate and zero-normal triangles (normalize(0)
    is reachable from a mesh without normals), materials over the whole parameter box, odd textures in random slots, lattice cameras."""
    import wgsl_scenes as S
    sc = S.fuzz_scene(rrt, seed)
    _parity(rrt, orc, sc, 65, 33, 3, 12, ("fuzz", seed))


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (17, 1), (1, 9), (63, 65), (127, 5)])
def test_mode1_odd_frame_sizes(rrt, orc, w, h):
    import wgsl_scenes as S
    sc = S.pbr_scene(rrt, n_target=5000, tex_size=16)
    _parity(rrt, orc, sc, w, h, 2, 10, (w, h))


def test_mode1_single_sample_and_progressive_accumulation(rrt, orc):
    """samples = 1, and sample ranges that start past 1 through the device entry with FLAG_SUM and FLAG_SUM | FLAG_ACCUM, against the
    oracle's sum_only partials of the same ranges (test_progressive_accumulation_and_postprocess, for mode 1)."""
    import torch
    import wgsl_scenes as S
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc = S.pbr_scene(rrt, n_target=5000, tex_size=16)
    w, h, depth = 80, 45, 10
    _parity(rrt, orc, sc, w, h, 1, depth, "one sample")
    hnd = sc.upload(0)
    m = sc.materials_array()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for trav, margin in TRAVERSALS:
        acc = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
        expect = np.zeros((h, w, 3), dtype=np.float32)
        done = 0
        for n in (1, 2, 3):
            part, _, _ = orc.render(sc.tris, sc.bvh_nodes, m, sc.textures, sc.camera.uniform, w, h, n, depth, seed_mode=1, sample_begin=done + 1,
                                    sum_only=1, want_rgba8=False, shading=1, cull=trav, cull_margin=margin)
            one = torch.full((w * h * 3,), 7.0, dtype=torch.float32, device="cuda")                      # FLAG_SUM alone overwrites
            o = rrt.make_options(w, h, n, depth, seed_mode=L.SEED_PER_SAMPLE, flags=L.FLAG_SUM, sample_begin=done + 1, traversal=trav,
                                 cull_margin=margin, shading=L.SHADING_WGPU)
            L.check(lib.mipt_render_device(hnd, L.ptr(sc.camera.uniform), C.byref(o), C.c_void_p(one.data_ptr()), None, stream, None), "render")
            torch.cuda.synchronize()
            assert _bits_equal(one.cpu().numpy(), part.reshape(-1)).all(), (trav, margin, n, "SUM")
            o.flags = L.FLAG_SUM | L.FLAG_ACCUM
            L.check(lib.mipt_render_device(hnd, L.ptr(sc.camera.uniform), C.byref(o), C.c_void_p(acc.data_ptr()), None, stream, None), "render")
            torch.cuda.synchronize()
            expect = expect + part
            done += n
            assert _bits_equal(acc.cpu().numpy(), expect.reshape(-1)).all(), (trav, margin, n, "SUM | ACCUM")
    out16 = torch.zeros(w * h * 4, dtype=torch.int16, device="cuda")
    L.check(lib.mipt_postprocess_device(C.c_void_p(acc.data_ptr()), w * h, float(done), C.c_void_p(out16.data_ptr()), stream), "postprocess")
    torch.cuda.synchronize()
    assert np.array_equal(out16.cpu().numpy().view(np.uint16).reshape(h, w, 4), orc.postprocess(expect, divisor=float(done)))


def test_mode1_after_refit(rrt, orc):
    """Mode 1 reads its own 128-byte material table and the rewritten shading stream: after a REFIT with moved vertices, new
    normals and new uvs the frame is the oracle's on the new triangles and the refitted tree."""
    import wgsl_scenes as S
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import host
    lib = rrt.load()
    sc = S.pbr_scene(rrt, n_target=5000, tex_size=16)
    sc.upload(0)
    _parity(rrt, orc, sc, 64, 36, 2, 10, "before the refit")
    rng = np.random.default_rng(9)
    new = sc.tris.copy()
    new["vertices"]["position"] += (rng.standard_normal(new["vertices"]["position"].shape) * 0.02).astype(np.float32)
    nrm = new["vertices"]["normal"] + (rng.standard_normal(new["vertices"]["normal"].shape) * 0.2).astype(np.float32)
    new["vertices"]["normal"] = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    new["vertices"]["tex_coord_x"] = new["vertices"]["tex_coord_x"] * np.float32(1.5) - np.float32(0.75)
    assert lib.mipt_scene_update_triangles(sc._handle, L.ptr(new), len(new), L.UPDATE_REFIT, None) == 0, lib.mipt_last_error()
    nodes = host.refit_nodes(sc.bvh_nodes, new)
    _parity(rrt, orc, sc, 64, 36, 2, 10, "after the refit", tris=new, nodes=nodes)


@pytest.mark.parametrize("mode", [0, 1])
def test_mode1_after_set_transforms(rrt, orc, mode):
    import test_gpu_mesh as gm
    import wgsl_scenes as S
    tris, mats, texs, cam = gm._case("helmet")
    rng = np.random.default_rng(12)
    texs = list(texs) + [rng.integers(0, 256, (5, 3, 4), dtype=np.uint8)]
    for i, k in enumerate(mats.keys()):
        m = mats[k]
        m["roughness"], m["metallic"], m["transmission"] = [0.1, 0.6][i % 2], [0.0, 0.7][i % 2], [0.8, 0.0][i % 2]
        m["normal_tex_id"] = len(texs) - 1
    mesh, _ = gm.mesh_model.mesh_from_triangles(tris, 5, shared=False, empty_parts=1)
    sc = rrt.Scene.from_mesh(materials=mats, textures=texs, transforms=None, **mesh)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    sc.upload_from_mesh(0, fetch_bvh=True)
    _parity(rrt, orc, sc, 64, 36, 2, 10, "as created")
    sc.set_transforms(gm._pose(len(sc.mesh["parts"]), 31, 0.4), mode)
    _parity(rrt, orc, sc, 64, 36, 2, 10, ("after set_transforms", mode))
