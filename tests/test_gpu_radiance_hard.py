"""GPU: mipt_query_radiance / mipt_query_radiance_device (pt_trace_rays_kernel) where tests/test_gpu_radiance.py does not go: at the
cull margin the product runs (MIPT_CULL_MARGIN_SAFE, the wrappers' default), with all five counters in both shadings, and on the
hard rays of tests/tools/hard_inputs.py -- the caller's first segment on both sides of every boundary of ray_safe, read again for
every sample after scatter segments that pass the guard.  The radiance rows at the safe margin ARE the reference traversal's (held
on the model alone by tests/test_hard_inputs_model.py), so only the counters can show a margin that was dropped on the way to the
kernel: they are compared in every arm.  NaNs compare as NaNs (H.differing), everything else bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import hard_inputs as H  # noqa: E402
import launch_thresholds as LT  # noqa: E402
import radiance_model as R  # noqa: E402
from test_gpu_radiance import CULL, KEYS, POOL, REF, _call, _case, _dev  # noqa: E402

pytestmark = pytest.mark.gpu

SAFE = H.CULL_MARGIN_SAFE
ARMS = ((REF, 0.0), (CULL, 0.0), (CULL, SAFE))
_models, _hard = {}, {}


def _hard_rays(rrt, orc, kind):
    if kind not in _hard:
        sc = _case(rrt, orc, kind)[0]
        _hard[kind] = H.hard_rays(sc.tris, H.eye_for(sc.tris, kind), seed=H.RAY_SEED)
    return _hard[kind]


def _model(rrt, orc, kind, which, n, samples, depth, shading, arm):
    """the model's output for the hard list (which = "hard") or the first n pool rays ("pool"), once per key; few NaN rows asserted"""
    key = (kind, which, n, samples, depth, shading, arm)
    if key not in _models:
        _, m, pool, _ = _case(rrt, orc, kind)
        rays = _hard_rays(rrt, orc, kind)[0] if which == "hard" else pool[:n]
        with np.errstate(all="ignore"):
            out = m.trace(rays, samples, depth, shading=shading, cull=arm[0], margin=arm[1])
        H.few_nan_rows(out)
        _models[key] = out
    return _models[key]


def _check(rrt, sc, rays, want_rows, want_counters, samples, depth, shading, arm, what, entries=(False, True), d_rays=None):
    """both entries, product and COUNT builds: the rows, and on the COUNT build all five counters"""
    from rust_ray_tracing_amd import _lib as L
    for device in entries:
        for flags in (0, L.FLAG_COUNT):
            rc, got, st = _call(rrt, sc, rays, samples, depth, shading, arm[0], flags, device, cull_margin=arm[1], d_rays=d_rays)
            assert rc == 0 and st["stack_overflows"] == 0 and st["pixels"] == len(rays), (what, arm, device, flags, rc, st)
            assert H.same_bits_or_both_nan(got, want_rows), (what, arm, device, flags, H.bad_rows(got, want_rows))
            if flags:
                assert {k: st[k] for k in KEYS} == dict(zip(KEYS, want_counters.sum(0).tolist())), (what, arm, device, st)


# ---- hard rays, alone, mixed into every wave, and as one whole wave ---------------------------------------------------------------------
@pytest.mark.parametrize("kind,shading", [("helmet", 0), ("helmet", 1), ("cornell", 0), ("wgsl_pbr", 1)])
def test_hard_rays(rrt, orc, kind, shading):
    sc, _, pool, _ = _case(rrt, orc, kind)
    hard, tags = _hard_rays(rrt, orc, kind)
    samples, depth = 3, 8
    safe = H.ray_safe(hard)
    assert 3 * int((~safe).sum()) >= len(hard) and 6 * int(safe.sum()) >= len(hard)
    n_pool = 4 * len(hard)
    mixed, at, rest = H.spread(hard, pool)
    wave = np.resize(np.flatnonzero(~safe), 64)                                    # 64 guard-failing rays: one whole wave on the IEEE quotient
    block = np.concatenate([pool[:64], hard[wave], pool[64:128]])
    steps = []
    for arm in ARMS:
        mh = _model(rrt, orc, kind, "hard", len(hard), samples, depth, shading, arm)
        mp = _model(rrt, orc, kind, "pool", n_pool, samples, depth, shading, arm)
        steps.append(int(mh["counters"][:, 1].sum()))
        _check(rrt, sc, hard, mh["mean"], mh["counters"], samples, depth, shading, arm, (kind, "alone"))
        rows, cnt = np.zeros((len(mixed), 3), np.float32), np.zeros((len(mixed), 5), np.int64)
        rows[at], rows[rest], cnt[at], cnt[rest] = mh["mean"], mp["mean"], mh["counters"], mp["counters"]
        _check(rrt, sc, mixed, rows, cnt, samples, depth, shading, arm, (kind, "spread"))
        rows = np.concatenate([mp["mean"][:64], mh["mean"][wave], mp["mean"][64:128]])
        cnt = np.concatenate([mp["counters"][:64], mh["counters"][wave], mp["counters"][64:128]])
        _check(rrt, sc, block, rows, cnt, samples, depth, shading, arm, (kind, "wave"))
    if kind == "helmet":
        assert len(set(steps)) == 3, steps                                          # the three arms are three different amounts of work


# ---- a scene whose planes switch the zero-origin clause of the guard off on two axes -----------------------------------------------------
def _tiny_plane_scene(rrt):
    """the lattice of tests/test_gpu_more.py::test_exact_division_guard_cases, moved by (1e-30, 0, 2e-35): planes through 0 on x become
    planes at 1e-30 (DevScene::tiny_axes bit 0), every z plane that was 0 sits at 2e-35 (bit 2)"""
    from rust_ray_tracing_amd import TRIANGLE
    from rust_ray_tracing_amd.synth import material
    rng = np.random.default_rng(77)
    n = 300
    c = np.round(rng.standard_normal((n, 1, 3)) * 3)
    p = c + np.round(rng.standard_normal((n, 3, 3)) * 1.5)
    p[: n // 3, :, 0] = 0.0
    p[n // 3: 2 * n // 3, :, 1] = 0.0
    t = np.zeros(n, dtype=TRIANGLE)
    nrm = rng.standard_normal((n, 3, 3))
    t["vertices"]["normal"] = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    mats = [material(base=(0.7, 0.6, 0.5), emission=(0.0, 0.0, 0.0)), material(base=(0.9, 0.9, 0.9), emission=(2.0, 1.5, 1.0))]
    t["material_id"] = rng.integers(0, 2, n)
    t["vertices"]["position"] = (p + np.array([1e-30, 0.0, 2e-35])).astype(np.float32)
    return rrt.Scene.from_arrays(t, mats, [])


def test_hard_rays_on_a_scene_with_tiny_planes(rrt, orc):
    sc = _tiny_plane_scene(rrt)
    planes = np.abs(np.concatenate([sc.bvh_nodes["bounds_min"], sc.bvh_nodes["bounds_max"]]))
    tiny = [bool(np.any((planes[:, k] != 0) & (planes[:, k] < 2.0 ** -76))) for k in range(3)]
    assert tiny == [True, False, True]                                              # tiny_axes = 0b101, restated from the nodes
    sc.upload(0)
    rng = np.random.default_rng(5)
    dirs = rng.normal(size=(6, 3)).astype(np.float32)
    dirs[:, 2] = np.abs(dirs[:, 2]) + np.float32(1.0)                               # towards the lattice from z = -7
    dirs /= np.abs(dirs).max(axis=1, keepdims=True)
    o = []
    for value in (0.0, 2.0 ** -71, 2.0 ** -70):
        for axis in range(3):
            oo = np.float32([0.5, -2.0, -7.0]); oo[axis] = value; o.append(oo)
        o.append(np.float32([value, -2.0, value])); o.append(np.float32([value, value, -7.0]))
    o = np.repeat(np.stack(o), len(dirs), axis=0)
    rays = np.zeros(len(o), dtype=R.RAY)
    rays["origin"], rays["direction"] = o, np.tile(dirs, (len(o) // len(dirs), 1))
    rays["reserved"] = R.default_seeds(len(o), first=300)
    safe = H.ray_safe(rays, tiny_axes=5)
    assert 4 * int(safe.sum()) >= len(rays) and 4 * int((~safe).sum()) >= len(rays)
    assert int((H.ray_safe(rays, 0) & ~safe).sum()) >= 12                           # rays only the scene's tiny planes take off the fast path
    m = R.Model(orc, sc)
    assert 4 * int(m.first_hits(rays).sum()) >= len(rays)
    for arm in ((REF, 0.0), (CULL, SAFE)):
        want = m.trace(rays, 3, 8, cull=arm[0], margin=arm[1])
        H.few_nan_rows(want)
        _check(rrt, sc, rays, want["mean"], want["counters"], 3, 8, 0, arm, "tiny planes")


# ---- the margin the product runs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shading", [("cornell", 0), ("cornell", 1), ("helmet", 0), ("helmet", 1), ("wgsl_pbr", 1), ("wgsl_pbr", 0)])
def test_safe_margin_on_the_product_scenes(rrt, orc, kind, shading):
    sc, _, pool, first = _case(rrt, orc, kind)
    n, samples, depth, arm = 384, 3, 8, (CULL, SAFE)
    want = _model(rrt, orc, kind, "pool", n, samples, depth, shading, arm)
    R.conditions(want, first[:n])
    _check(rrt, sc, pool[:n], want["mean"], want["counters"], samples, depth, shading, arm, kind)
    got, st = sc.query_radiance(pool[:n], seeds=pool["reserved"][:n], samples=samples, max_ray_depth=depth, traversal=CULL, shading=shading)
    assert R.same_bits(got, want["mean"]) and st["pixels"] == n                     # the wrapper's default margin is that margin
    got, _ = sc.query_radiance(_dev(pool[:n]), samples=samples, max_ray_depth=depth, traversal=CULL, shading=shading)
    assert R.same_bits(got.cpu().numpy(), want["mean"])


# ---- hard rays among the rays that refill lanes in the middle of other lanes' traversals ------------------------------------------------
def test_hard_rays_refill_lanes_mid_traversal(rrt, orc):
    from rust_ray_tracing_amd import _lib as L
    kind, shading, arm, samples, depth = "cornell", 0, (CULL, SAFE), 2, 5
    n_cu = LT.device_n_cu()
    n = LT.mid(n_cu)
    LT.check_mid(n_cu, n)
    sc, _, pool, _ = _case(rrt, orc, kind)
    hard, _ = _hard_rays(rrt, orc, kind)
    mh = _model(rrt, orc, kind, "hard", len(hard), samples, depth, shading, arm)
    mp = _model(rrt, orc, kind, "pool", POOL, samples, depth, shading, arm)
    unit, at, rest = H.splice(pool, hard, 19)                                       # 19: coprime to 64, so the hard rays visit every lane
    rows, cnt = np.zeros((len(unit), 3), np.float32), np.zeros((len(unit), 5), np.int64)
    rows[at], rows[rest], cnt[at], cnt[rest] = mh["mean"], mp["mean"], mh["counters"], mp["counters"]
    idx = (7 * np.arange(n, dtype=np.int64) + 3) % len(unit)
    assert len(np.unique(np.flatnonzero(np.isin(idx, at)) % 64)) == 64             # a hard ray starts in every lane position
    rays = np.ascontiguousarray(unit[idx])
    d_rays = _dev(rays)
    want_rows, want_cnt = rows[idx], cnt[idx].sum(0)
    for device in (False, True):
        for flags in (0, L.FLAG_COUNT):
            rc, got, st = _call(rrt, sc, rays, samples, depth, shading, arm[0], flags, device, d_rays=d_rays, cull_margin=arm[1])
            assert rc == 0 and st["pixels"] == n and st["stack_overflows"] == 0
            assert H.same_bits_or_both_nan(got, want_rows), (device, flags, H.bad_rows(got, want_rows))
            if flags:
                assert {k: st[k] for k in KEYS} == dict(zip(KEYS, want_cnt.tolist())), (device, st)
