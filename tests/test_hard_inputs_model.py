"""CPU: the models of tests/tools/radiance_model.py and tests/tools/bake_model.py alone, on the inputs of tests/tools/hard_inputs.py.
tests/test_gpu_radiance_hard.py and tests/test_gpu_bake_hard.py compare the kernels with these models at the safe cull margin and on
hard rays and points; here the models are held to what those comparisons rely on, so that no GPU test passes for lack of cases:
the one-ray oracle entries with a margin are the old ones at margin 0, every class of input is there and falls on both sides of the
kernel's guard, few rows are NaN, the rows at margin 2^-7 are the reference traversal's, and the step counts of the three arms all
differ -- which is what lets a counter comparison see a margin that was dropped.  The same for tests/tools/probe_model.py on the hard
probes of tests/test_gpu_probe_hard.py: every class is there, a third of them fail the origin clauses of the guard and a sixth pass,
a quarter have a path that hits and a quarter one that escapes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import bake_model as B  # noqa: E402
import hard_inputs as H  # noqa: E402
import probe_model as PM  # noqa: E402
import radiance_model as R  # noqa: E402
import test_gpu_bake as TB  # noqa: E402
import test_gpu_radiance as TR  # noqa: E402

REF, CULL = 0, 1
SAFE = H.CULL_MARGIN_SAFE
ARMS = ((REF, 0.0), (CULL, 0.0), (CULL, SAFE))
N_POOL = 384                                     # the pool prefix of test_safe_margin_on_the_product_scenes
INNER = R.COUNTERS.index("inner_steps")

_cases = {}


def _case(rrt, orc, kind):
    """(host-built Scene, R.Model, the pool of tests/test_gpu_radiance.py, the hard rays and their tags)"""
    if kind not in _cases:
        sc = TR._build_scene(rrt, kind)
        hard, tags = H.hard_rays(sc.tris, H.eye_for(sc.tris, kind), seed=H.RAY_SEED)
        _cases[kind] = (sc, R.Model(orc, sc), R.make_rays(sc.tris, TR.POOL, seed=TR.POOL_SEED), hard, tags)
    return _cases[kind]


# ---- the oracle's entries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cornell", "helmet"])
def test_margin_entries_at_margin_0_are_the_old_entries(rrt, orc, kind):
    _, m, pool, _, _ = _case(rrt, orc, kind)
    lib = m.lib
    args = (m.tris.ctypes.data, m.tris.nbytes // 112, m.nodes.ctypes.data, m.nodes.nbytes // 32, m.mats.ctypes.data, m.mats.nbytes // 80, m.tex_array,
            len(m.texs))
    F3 = C.c_float * 3
    for cull in (0, 1):
        for i in range(300):
            o, d = F3(*[float(x) for x in pool["origin"][i]]), F3(*[float(x) for x in pool["direction"][i]])
            seed = int(pool["reserved"][i])
            a, b, sa, sb, ca, cb = F3(), F3(), C.c_uint32(seed), C.c_uint32(seed), (C.c_uint64 * 5)(), (C.c_uint64 * 5)()
            lib.orc_trace_ray(*args, C.byref(o), C.byref(d), 8, C.byref(sa), cull, orc.LIBM_GLIBC235, C.byref(a))
            lib.orc_trace_ray_m(*args, C.byref(o), C.byref(d), 8, C.byref(sb), cull, C.c_float(0.0), orc.LIBM_GLIBC235, C.byref(b), C.byref(cb))
            assert bytes(a) == bytes(b) and sa.value == sb.value and cb[0] >= 1, (cull, i)
            sa, sb = C.c_uint32(seed), C.c_uint32(seed)
            lib.orc_trace_ray_wgsl(*args, C.byref(o), C.byref(d), 8, C.byref(sa), cull, orc.LIBM_GLIBC235, C.byref(a), C.byref(ca))
            lib.orc_trace_ray_wgsl_m(*args, C.byref(o), C.byref(d), 8, C.byref(sb), cull, C.c_float(0.0), orc.LIBM_GLIBC235, C.byref(b), C.byref(cb))
            assert bytes(a) == bytes(b) and sa.value == sb.value and list(ca) == list(cb), (cull, i)


# ---- the generators -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cornell", "helmet", "wgsl_pbr"])
def test_every_class_of_hard_ray_is_there_on_both_sides_of_the_guard(rrt, orc, kind):
    _, m, _, hard, tags = _case(rrt, orc, kind)
    assert sorted(tags.tolist()) == sorted(H.RAY_CLASSES) and len(set(tags.tolist())) == len(tags) == 147
    safe = H.ray_safe(hard)
    assert 3 * int((~safe).sum()) >= len(hard) and 6 * int(safe.sum()) >= len(hard), (int(safe.sum()), len(hard))
    by = dict(zip(tags.tolist(), safe.tolist()))
    for axis in "xyz":                                                              # each boundary of the guard, from both sides
        assert by[f"d{axis}=2^-60"] and not by[f"d{axis}=2^-61"] and by[f"d{axis}=2"] and not by[f"d{axis}=next(2)"]
        assert by[f"o{axis}=2^40"] and not by[f"o{axis}=next(2^40)"] and by[f"o{axis}=2^-70"] and not by[f"o{axis}=2^-71"]
        assert not by[f"d{axis}=0"] and not by[f"d{axis}=1e-42"] and not by[f"o{axis}=1e-42"]
    assert H.ray_safe(hard, tiny_axes=7).sum() <= safe.sum()
    for s in H.HARD_SEEDS:
        assert s in hard["reserved"]
    first = m.first_hits(hard)                                                      # the aimed rays see the scene: the hard seeds get used
    aimed = np.array([t.startswith(("vertex", "edge")) for t in tags])
    assert 2 * int(first[aimed].sum()) >= int(aimed.sum())
    assert all(first[hard["reserved"] == s].all() for s in H.HARD_SEEDS)
    assert len(np.resize(np.flatnonzero(~safe), 64)) == 64 and int((~safe).sum()) >= 48


def test_every_class_of_hard_point_is_there(rrt, orc):
    base = TB._base_scene(rrt, "helmet")
    tris, special = H.with_special_triangles(base.tris)
    pts, tags = H.hard_points(tris, special)
    assert set(tags.tolist()) == set(H.POINT_CLASSES)
    assert int((tags == "none").sum()) >= 5 and pts["prim"][tags == "none"].tolist() == [B.NONE] * int((tags == "none").sum())
    for i in range(len(H.UV_SPECIALS)):
        assert int((tags == f"uv{i}").sum()) == 2
    nrm, pos = tris["vertices"]["normal"][special], tris["vertices"]["position"][special]
    assert not nrm[0].any() and np.isnan(nrm[1]).all(axis=1).sum() == 1 and np.isnan(nrm[1]).any(axis=1).sum() == 1 and np.all(nrm[2] == np.float32(1e30)) and np.all(np.abs(nrm[3]) == np.float32(1e-30))
    assert not np.cross(pos[4, 1] - pos[4, 0], pos[4, 2] - pos[4, 0]).any() and np.any(pos[4, 1] != pos[4, 0])
    for s in H.ZERO_SEEDS:                                                          # the formula gives 0 at g * stride = 0, and 1 is used
        assert (987612486 * ((s + 87636354) & B.M32)) & B.M32 == 0 and B.sample_seed(s, 0, H.HARD_STRIDE) == 1
    g = H.HARD_FIRST_SAMPLE + 1                                                     # ... and only at the second sample of first_sample = 5
    assert g * H.HARD_STRIDE > B.M32 and B.sample_seed(H.LATE_ZERO_SEED, g, H.HARD_STRIDE) == 1
    assert (987612486 * ((H.LATE_ZERO_SEED + ((g * H.HARD_STRIDE) & B.M32) + 87636354) & B.M32)) & B.M32 == 0
    assert all(B.sample_seed(H.LATE_ZERO_SEED, k, H.HARD_STRIDE) != 1 for k in (0, 1, 2, 5, 7))
    junk = pts[np.char.startswith(tags, "prim_junk")]
    assert np.all(junk["prim"] != B.NONE) and np.all((junk["prim"] & np.uint32(H.PRIM_JUNK)) == H.PRIM_JUNK)
    tri = pts["prim"][pts["prim"] != B.NONE] & B.TRI_MASK
    assert 0 in tri and len(tris) - 1 in tri and 0xFFFFFFFF in pts["seed"]


# ---- the radiance model on the pool prefix and on the hard list ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shadings", [("cornell", (0, 1)), ("helmet", (0, 1)), ("wgsl_pbr", (1, 0))])
def test_radiance_model_rows_few_nans_and_the_safe_margin_is_the_reference(rrt, orc, kind, shadings):
    _, m, pool, hard, _ = _case(rrt, orc, kind)
    with np.errstate(all="ignore"):
        for shading in shadings:
            for name, rays in (("pool", pool[:N_POOL]), ("hard", hard)):
                out = {arm: m.trace(rays, 3, 8, shading=shading, cull=arm[0], margin=arm[1]) for arm in ARMS}
                for arm in ARMS:
                    H.few_nan_rows(out[arm])
                    if kind != "wgsl_pbr":
                        assert H.nan_rows(out[arm]["sum"]) == 0, (kind, shading, name, arm)
                assert H.same_bits_or_both_nan(out[ARMS[2]]["sum"], out[ARMS[0]]["sum"]), (kind, shading, name, H.bad_rows(out[ARMS[2]]["sum"], out[ARMS[0]]["sum"]))
                assert np.array_equal(out[ARMS[2]]["state"], out[ARMS[0]]["state"])
                if kind == "helmet":                                                # what makes the counter comparison bite
                    steps = [int(out[arm]["counters"][:, INNER].sum()) for arm in ARMS]
                    assert len(set(steps)) == 3 and steps[0] > steps[2] > steps[1], (shading, name, steps)


# ---- the gather model on the hard points ---------------------------------------------------------------------------------------------------
def _host_scene(rrt, kind, special):
    """(host-built Scene, the caller's array): the triangles permuted, with the special triangles where asked"""
    base = TB._base_scene(rrt, kind)
    tris, idx = (H.with_special_triangles(base.tris) if special else (base.tris, None))
    perm = np.random.default_rng(11).permutation(len(tris))
    caller = np.ascontiguousarray(tris[perm])
    where = None if idx is None else np.array([int(np.flatnonzero(perm == k)[0]) for k in idx])
    return rrt.Scene.from_arrays(caller.copy(), base.materials, base.textures), caller, where


@pytest.mark.parametrize("kind,special", [("cornell", False), ("helmet", True), ("wgsl_pbr", False)])
def test_gather_model_rows_few_nans_and_the_safe_margin_is_the_reference(rrt, orc, kind, special):
    sc, caller, where = _host_scene(rrt, kind, special)
    if where is None:
        pts = TB._random_points(caller, 96, TB.POINT_SEED)
    else:
        hard, _ = H.hard_points(caller, where)
        pts, _, _ = H.interleave(hard, TB._random_points(caller, 96, TB.POINT_SEED))
    g = B.Gather(orc, sc, caller)
    for shading in (0, 1):
        for first_sample in (0, H.HARD_FIRST_SAMPLE):
            out = {arm: g.run(pts, 3, 4, shading=shading, cull=arm[0], margin=arm[1], first_sample=first_sample, stride=H.HARD_STRIDE) for arm in ARMS}
            for arm in ARMS:
                H.few_nan_rows(out[arm])
                none = pts["prim"] == B.NONE
                assert np.array_equal(out[arm]["counters"][none][:, [0, 3, 4]], np.tile([3, 0, 0], (int(none.sum()), 1)))
            assert H.same_bits_or_both_nan(out[ARMS[2]]["sum"], out[ARMS[0]]["sum"]), (kind, shading, first_sample)
            if kind == "helmet":
                steps = [int(out[arm]["counters"][:, INNER].sum()) for arm in ARMS]
                assert len(set(steps)) == 3, (shading, first_sample, steps)


# ---- the bake model on the hard probes ------------------------------------------------------------------------------------------------------
_probe_cases = {}


def _probe_case(rrt, orc, kind):
    """(host-built Scene of tests/test_gpu_probe.py's triangles in its order, PM.Bake, the hard probes and their tags)"""
    if kind not in _probe_cases:
        tris, mats, texs = PM.case_scene(rrt, kind)
        sc = rrt.Scene.from_arrays(np.ascontiguousarray(tris[np.random.default_rng(11).permutation(len(tris))]), mats, texs)
        pr, tags = H.hard_probes(sc.tris, sc.bvh_nodes, H.PROBE_SEED)
        _probe_cases[kind] = (sc, PM.Bake(orc, sc), pr, tags)
    return _probe_cases[kind]


@pytest.mark.parametrize("kind", ["cornell", "helmet", "wgsl_pbr"])
def test_every_class_of_hard_probe_is_there_on_both_sides_of_the_guard(rrt, orc, kind):
    sc, _, pr, tags = _probe_case(rrt, orc, kind)
    assert tags.tolist() == H.PROBE_CLASSES and len(set(tags.tolist())) == len(pr) == 63
    safe = H.origin_safe(pr)
    assert 3 * int((~safe).sum()) >= len(pr) and 6 * int(safe.sum()) >= len(pr), (int(safe.sum()), len(pr))
    by = dict(zip(tags.tolist(), safe.tolist()))
    pos = dict(zip(tags.tolist(), pr["position"]))
    for a, axis in enumerate("xyz"):                                                # each boundary of the origin clauses, from both sides
        assert by[f"p{axis}=2^40"] and not by[f"p{axis}=next(2^40)"] and by[f"p{axis}=2^-70"] and not by[f"p{axis}=2^-71"]
        assert by[f"p{axis}=0"] and by[f"p{axis}=-0"] and not by[f"p{axis}=1e-42"] and not by[f"p{axis}=nan"] and not by[f"p{axis}=+inf"]
        assert np.signbit(pos[f"p{axis}=-0"][a]) and pos[f"p{axis}=-0"][a] == 0 and not np.signbit(pos[f"p{axis}=0"][a])
        others = [b for b in range(3) if b != a]
        assert np.all(np.isfinite(pos[f"p{axis}=nan"][others])) and np.isnan(pos[f"p{axis}=nan"][a])
    assert by["p=0"] and not by["p=2^-71"] and not pr["position"][tags == "p=0"].any()
    assert not H.origin_safe(pr, tiny_axes=7)[np.char.startswith(tags, "p") & (np.char.endswith(tags, "=0") | np.char.endswith(tags, "=-0"))].any()
    for s in H.HARD_SEEDS + H.ZERO_SEEDS + (H.LATE_ZERO_SEED,):
        assert s in pr["seed"][np.char.startswith(tags, "on_")]
    # on geometry: bit for bit on a vertex, on a plane of an inner node, on a corner of the bounds
    P = sc.tris["vertices"]["position"].reshape(-1, 3)
    for t in tags[np.char.startswith(tags, "on_vertex")]:
        assert np.any(np.all(P == pos[t], axis=1)), t
    inner = sc.bvh_nodes[sc.bvh_nodes["num_tris"] == 0]
    planes = np.concatenate([inner["bounds_min"], inner["bounds_max"]])
    for t in tags[np.char.startswith(tags, "on_node_plane")]:
        assert any(np.any(planes[:, a] == pos[t][a]) for a in range(3)), t
    lo, hi = P.min(0), P.max(0)
    for t in tags[np.char.startswith(tags, "on_corner")]:
        assert np.all((pos[t] == lo) | (pos[t] == hi)), t


@pytest.mark.parametrize("kind,shadings", [("cornell", (0,)), ("helmet", (0, 1)), ("wgsl_pbr", (1,))])
def test_probe_model_on_the_hard_probes_few_nans_hits_and_escapes(rrt, orc, kind, shadings):
    _, m, pr, _ = _probe_case(rrt, orc, kind)
    for shading in shadings:
        for first_sample in (0, H.HARD_FIRST_SAMPLE):
            out = {arm: m.run(pr, 3, 8, shading=shading, cull=arm[0], margin=arm[1], first_sample=first_sample, stride=H.HARD_STRIDE) for arm in ARMS}
            for arm in ARMS:
                H.few_nan_rows(out[arm])
                assert 4 * int(out[arm]["hit"].any(axis=1).sum()) >= len(pr)                  # a quarter of the probes have a path that hits
                assert 4 * int((~out[arm]["hit"]).any(axis=1).sum()) >= len(pr)               # a quarter have one that escapes
                assert np.abs(np.linalg.norm(out[arm]["dirs"].astype(np.float64), axis=2) - 1).max() < 1e-6
                rays = H.probe_rays(pr, out[arm]["dirs"])                                       # unit directions pass their clauses: the origin decides
                assert np.array_equal(H.ray_safe(rays), np.repeat(H.origin_safe(pr), 3))
            assert H.same_bits_or_both_nan(out[ARMS[2]]["sum"], out[ARMS[0]]["sum"]), (kind, shading, first_sample)
    # the streams: both zero seeds run on stream 1 at first_sample 0, the late one at the second sample of HARD_FIRST_SAMPLE
    assert all(B.sample_seed(s, 0, H.HARD_STRIDE) == 1 for s in H.ZERO_SEEDS)
    assert B.sample_seed(H.LATE_ZERO_SEED, H.HARD_FIRST_SAMPLE + 1, H.HARD_STRIDE) == 1


def test_tiny_plane_probes_leave_the_fast_path_for_the_planes_alone(rrt, orc):
    from test_gpu_radiance_hard import _tiny_plane_scene
    sc = _tiny_plane_scene(rrt)
    pr = H.tiny_plane_probes()
    assert len(pr) == 45 and len(set(pr["seed"].tolist())) == 45
    out = PM.Bake(orc, sc).run(pr, 3, 8)
    rays = H.probe_rays(pr, out["dirs"])
    only = (H.ray_safe(rays, 0) & ~H.ray_safe(rays, 5)).reshape(len(pr), 3).all(axis=1)
    assert int(only.sum()) >= 12, int(only.sum())
    safe = H.ray_safe(rays, 5)
    assert 4 * int(safe.sum()) >= len(rays) and 4 * int((~safe).sum()) >= len(rays)
    H.few_nan_rows(out)
    assert 4 * int(out["hit"].sum()) >= out["hit"].size
