"""CPU: the C oracle's restatement of the wgpu shaders (shading mode 1: trace_wgsl / orc_postprocess in oracle/pt_oracle.c)
against a second, independent reading of rt_compute.wgsl / pp_compute.wgsl (oracle/pt_oracle_py.py render_wgsl /
postprocess_wgsl, pure Python over float32 scalars, transcendentals through the platform libm).  The kernel's shade_wgsl was
written from the C restatement, so a misreading of the shader would be shared by kernel and oracle; two readings that agree
bit for bit -- on scenes that provably reach every rarely taken branch -- are the pin for "did the oracle misread the WGSL?".

The Python reading follows the shader's traversal, which culls children beyond the best hit (rt_compute.wgsl:348); the oracle
is run with the same rule (cull=1, margin 0), so the traversal counters are comparable too."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))

# (name, scene builder, width, height, spp, depth, pixel stride): each a few hundred pixels for the pure-Python reading
CASES = [
    ("pbr_atrium",       lambda rrt, S: S.pbr_scene(rrt, n_target=2500, tex_size=16),             48, 27, 2, 12, 5),   # (a)
    ("glass_dragon_1.5", lambda rrt, S: S.glass_scene(rrt, "dragon", 1500, ior=1.5),              40, 30, 2, 10, 5),   # (b)
    ("glass_helmet_2.4", lambda rrt, S: S.glass_scene(rrt, "helmet", 1200, ior=2.4, roughness=0.05), 40, 30, 2, 10, 5),
    ("odd_textures",     lambda rrt, S: S.odd_texture_scene(rrt, "helmet", 1200),                 40, 30, 2, 8, 5),    # (c)
    ("pbr_depth_1",      lambda rrt, S: S.pbr_scene(rrt, n_target=2500, tex_size=16),             48, 27, 2, 1, 7),    # (d)
    ("pbr_depth_3",      lambda rrt, S: S.pbr_scene(rrt, n_target=2500, tex_size=16),             48, 27, 2, 3, 7),
    ("pbr_depth_4",      lambda rrt, S: S.pbr_scene(rrt, n_target=2500, tex_size=16),             48, 27, 2, 4, 7),
    ("pbr_depth_5",      lambda rrt, S: S.pbr_scene(rrt, n_target=2500, tex_size=16),             48, 27, 2, 5, 7),
    ("fuzz_soup_1",      lambda rrt, S: S.fuzz_scene(rrt, 1),                                     33, 17, 2, 8, 3),    # zero normals, z-normals
]
_branch_totals = {}


def _same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_wgsl_readings_agree_bit_for_bit(rrt, orc, case):
    """Radiance bit for bit (NaN = NaN) and rays / inner_steps / tri_tests / hits / texel_fetches equal."""
    import wgsl_scenes as S
    from oracle import pt_oracle_py as py
    name, make, w, h, spp, depth, stride = case
    sc = make(rrt, S)
    pixels = list(range(0, w * h, stride))
    mats = sc.materials_array()
    got, cnt = py.render_wgsl(sc.tris, sc.bvh_nodes, mats, sc.textures, sc.camera.uniform, w, h, spp, depth, pixels=pixels)
    ref, _, st = orc.render(sc.tris, sc.bvh_nodes, mats, sc.textures, sc.camera.uniform, w, h, spp, depth, pix_begin=0, pix_stride=stride,
                            cull=1, cull_margin=0.0, shading=1, want_rgba8=False)
    ref = ref.reshape(-1, 3)
    for p in pixels:
        assert _same_bits(got[p], ref[p]), (name, p, got[p], ref[p])
    for k in py.WGSL_COUNTERS:
        assert cnt[k] == st[k], (name, k, cnt[k], st[k])
    if depth > 1:
        assert cnt["rays"] > len(pixels) * spp
    if depth < 4:
        assert cnt["roulette_entered"] == 0                                 # roulette starts at the fourth hit, not before
    if depth == 4:
        assert cnt["roulette_entered"] > 0
    _branch_totals[name] = {k: cnt[k] for k in py.WGSL_BRANCHES}


def test_every_rare_branch_is_reached(rrt, orc):
    """Summed over the agreement cases above plus direct helper calls for the two measure-zero events, every branch counter of
    the reading is nonzero: the agreement is not vacuous on total internal reflection, the alternate basis axis, roulette ..."""
    import wgsl_scenes as S
    from oracle import pt_oracle_py as py
    F = np.float32
    for case in CASES:                                                      # run alone: fill in whatever has not been rendered yet
        if case[0] not in _branch_totals:
            name, make, w, h, spp, depth, stride = case
            sc = make(rrt, S)
            _, cnt = py.render_wgsl(sc.tris, sc.bvh_nodes, sc.materials_array(), sc.textures, sc.camera.uniform, w, h, spp, depth,
                                    pixels=list(range(0, w * h, stride)))
            _branch_totals[name] = {k: cnt[k] for k in py.WGSL_BRANCHES}
    total = {k: sum(t[k] for t in _branch_totals.values()) for k in py.WGSL_BRANCHES}
    # lensq == 0: a view vector along the normal, ve = (0, 0, 1), gives Vh.x = Vh.y = 0 exactly
    c = py.wgsl_counters()
    rng = [12345]
    ne = py.w_sample_ggx_vndf((F(0), F(0), F(1)), F(0.25), F(0.25), rng, c)
    assert c["lensq_zero"] == 1 and abs(float(py.length(ne)) - 1.0) < 1e-6
    # u_offset == (0, 0): both draws exactly 0.5, i.e. two consecutive xorshift outputs that round to 2^31 as f32.  The first
    # output x1 lies in [2^31 - 64, 2^31 + 128]; search those few states for one whose successor does too.
    def unstep(y):                                                         # inverse of one xorshift32 step
        t = y
        for _ in range(7):
            t = y ^ ((t << 5) & py.U32)
        y, t = t, t
        for _ in range(2):
            t = y ^ (t >> 17)
        y, t = t, t
        for _ in range(3):
            t = y ^ ((t << 13) & py.U32)
        return t
    assert py.xor_shift([unstep(0xDEADBEEF)]) == 0xDEADBEEF
    found = None
    for x1 in range(0x80000000 - 64, 0x80000000 + 129):
        st = [unstep(x1)]
        if py.rand_f32(st) == F(0.5) and py.rand_f32(st) == F(0.5):
            found = unstep(x1)
            break
    c2 = py.wgsl_counters()
    if found is not None:
        d = py.w_cosine_sample_hemisphere([found], c2)
    else:                                                                  # no such state: call the disk function directly
        d = py.w_concentric_sample_disk((F(0.5), F(0.5)), c2) + (F(1),)
    assert c2["u_offset_zero"] == 1 and float(d[0]) == 0.0 and float(d[1]) == 0.0
    total["lensq_zero"] += c["lensq_zero"]
    total["u_offset_zero"] += c2["u_offset_zero"]
    print("branch totals:", total)
    missing = [k for k in py.WGSL_BRANCHES if total[k] == 0]
    assert not missing, (missing, _branch_totals)
    # the C oracle takes the same decisions on the direct inputs
    t = orc.wgsl_vndf(np.array([[0, 0, 1]], np.float32), 0.25, 0.25, np.array([12345], np.uint32))
    assert _same_bits(t[0], ne)
    if found is not None:
        hc = orc.wgsl_cosine_hemisphere(np.array([found], np.uint32))
        assert _same_bits(hc[0], d)


def test_postprocess_second_reading(orc):
    """pp_compute.wgsl read a second time against orc.postprocess: a ramp, the neighbourhood of the 0.0031308 cutoff, 0, 1, values
    above 1, negatives, infinities and NaN, with and without a divisor."""
    from oracle import pt_oracle_py as py
    cut = np.float32(0.0031308)
    near = [cut]
    for _ in range(6):
        near = [np.nextafter(near[0], np.float32(0))] + near + [np.nextafter(near[-1], np.float32(1))]
    vals = np.concatenate([np.linspace(0, 1, 1201), np.linspace(0, 0.01, 300), near, [0.0, -0.0, 1.0, 1.0000001, 1.5, 7.25, 1e30, np.inf],
                           [-1e-9, -0.5, -3.0, -np.inf, np.nan, 1e-45, 1e-38, 0.9999999]]).astype(np.float32)
    vals = np.concatenate([vals, np.zeros((-len(vals)) % 3, np.float32)]).reshape(-1, 3)
    for div in (1.0, 3.0):
        want = orc.postprocess(vals.reshape(1, -1, 3) * np.float32(div), divisor=div)[0]
        got = py.postprocess_wgsl(vals * np.float32(div), divisor=div)
        assert np.array_equal(got, want[:, :3]), div
        assert (want[:, 3] == 65535).all()
