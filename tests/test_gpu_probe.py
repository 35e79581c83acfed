"""GPU: mipt_probe_bake / mipt_probe_irradiance and their _device forms (csrc/probe.hip, csrc/mipt_probe.cpp) against the models of
tests/tools/probe_model.py: the bake as a Python loop over the oracle's one-ray entries with the basis and the 27 ordered sums in
numpy f32, the lookup as a numpy f32 restatement.  Every word is compared on the bits, with a sentinel behind the output.  Scenes are
built on the device from a shuffled triangle array and their tree is mirrored for the oracle; the scenes and probes are those
tests/test_probe_model.py (CPU) holds the model alone to its conditions on."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import launch_thresholds as LT  # noqa: E402
import probe_model as PM  # noqa: E402
import radiance_model as R  # noqa: E402

pytestmark = pytest.mark.gpu

REF, CULL = 0, 1
SAFE = 0.0078125                               # MIPT_CULL_MARGIN_SAFE
SENTINEL = 0x7FA5A5A5                          # a NaN pattern no coefficient and no irradiance has
KEYS = R.COUNTERS
PERIOD = 1031                                  # the long probe lists repeat with this period: the model runs once per period


# ---- scenes, probes, the model ---------------------------------------------------------------------------------------------------------
def _from_triangles(rrt, caller, mats, texs=()):
    """a resident Scene built on the device with its tree mirrored; the tree's order is asserted not to be the caller's"""
    caller = np.ascontiguousarray(caller).copy()
    sc = rrt.Scene.from_arrays(caller, mats, texs, build_bvh=False)
    sc.upload_from_triangles(0, fetch_bvh=True)
    assert len(caller) >= 12 and not np.array_equal(sc._tri_order, np.arange(len(caller)))
    return sc, caller


_scenes, _models = {}, {}


def _case(rrt, orc, kind):
    """(resident device-built Scene, PM.Bake, the caller's triangles, PM.N_PROBES probes) -- made once per kind, left unchanged"""
    if kind not in _scenes:
        tris, mats, texs = PM.case_scene(rrt, kind)
        rng = np.random.default_rng(11)
        sc, caller = _from_triangles(rrt, tris[rng.permutation(len(tris))], mats, texs)
        _scenes[kind] = (sc, PM.Bake(orc, sc), caller, PM.case_probes(caller))
    return _scenes[kind]


def _model(rrt, orc, kind, samples, depth, shading=0, cull=0, margin=0.0, first_sample=0, stride=None, probes=None, tag=None):
    key = (kind, samples, depth, shading, cull, margin, first_sample, stride, tag)
    if key not in _models:
        _, m, _, pr = _case(rrt, orc, kind)
        pr = pr if probes is None else probes
        out = m.run(pr, samples, depth, shading=shading, cull=cull, margin=margin, first_sample=first_sample, stride=stride)
        if probes is None:
            PM.conditions(out, PM.PLANTED_NAN)
        _models[key] = out
    return _models[key]


def _dev(probes):
    import torch
    return torch.from_numpy(np.ascontiguousarray(probes).view(np.int32).reshape(-1, 4).copy()).cuda()


def _bake(rrt, sc, probes, samples, depth, shading=0, traversal=REF, flags=0, device=False, first_sample=0, stride=None, handle=None, lib=None,
          d_out=None, extra=5, cull_margin=0.0, stream=None, d_probes=None):
    """One call of the C entry with a sentinel behind the output -> (rc, sh [n, 9, 3] f32, stats dict); the sentinel is asserted"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = lib or rrt.load()
    n = len(probes)
    opt = L.MiptProbeBakeOptions()
    opt.samples, opt.max_ray_depth, opt.traversal, opt.cull_margin, opt.shading, opt.flags = samples, depth, traversal, cull_margin, shading, flags
    opt.first_sample, opt.sample_stride = first_sample, (n if stride is None else stride)
    st = L.MiptStats()
    h = handle if handle is not None else sc._handle
    if device:
        d_p = _dev(probes) if d_probes is None else d_probes
        if d_out is None:
            d_out = torch.full((n * 27 + extra,), SENTINEL, dtype=torch.int32, device="cuda")
        rc = lib.mipt_probe_bake_device(h, d_p.data_ptr(), n, C.byref(opt), d_out.data_ptr(), stream, C.byref(st))
        torch.cuda.synchronize()
        out = d_out.cpu().numpy().view(np.uint32).reshape(-1)
    else:
        out = np.full(n * 27 + extra, SENTINEL, dtype=np.uint32)
        p = np.ascontiguousarray(probes)
        rc = lib.mipt_probe_bake(h, L.ptr(p), n, C.byref(opt), L.ptr(out), C.byref(st))
    assert np.all(out[n * 27:] == SENTINEL), "written past n * 27 floats"
    return rc, out[: n * 27].view(np.float32).reshape(n, 9, 3), st.as_dict()


def _bad_rows(got, want):
    g = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), -1)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(len(want), -1)
    bad = np.flatnonzero((g != w).any(axis=1))
    return len(bad), [(int(i), g[i][:6].tolist(), w[i][:6].tolist()) for i in bad[:3]]


def _counters_match(st, model, n_paths):
    return {k: st[k] for k in KEYS} == dict(zip(KEYS, model["counters"].sum(0).tolist())) and st["pixels"] == n_paths


# ---- bake: model parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", [(REF, 0.0), (CULL, SAFE)])
@pytest.mark.parametrize("kind,shading", [("cornell", 0), ("cornell", 1), ("helmet", 0), ("helmet", 1), ("wgsl_pbr", 1), ("wgsl_pbr", 0)])
def test_bake_model_parity(rrt, orc, kind, shading, arm):
    from rust_ray_tracing_amd import _lib as L
    sc, _, _, pr = _case(rrt, orc, kind)
    assert len(pr) == 65 and np.isnan(pr["position"][PM.I_NAN, 0]) and np.isinf(pr["position"][PM.I_INF, 1]) and pr["seed"][PM.I_MAX] == 0xFFFFFFFF
    for samples in (1, 3, 64):
        want = _model(rrt, orc, kind, samples, 4, shading, arm[0], arm[1])
        assert np.any(want["sum"][:, 1:] != 0)
        for device in (False, True):
            for flags, key in ((0, "mean"), (L.FLAG_SUM, "sum"), (L.FLAG_COUNT, "mean")):
                if samples == 64 and flags == L.FLAG_SUM and not device:
                    continue                                                               # the sum at 64 samples: the device entry alone
                rc, got, st = _bake(rrt, sc, pr, samples, 4, shading, arm[0], flags, device, cull_margin=arm[1])
                assert rc == 0 and PM.same_bits(got, want[key]), (kind, shading, arm, samples, device, flags, _bad_rows(got, want[key]))
                assert st["kernel_ms"] > 0 and st["stack_overflows"] == 0 and st["pixels"] == len(pr) * samples
                if flags == L.FLAG_COUNT:
                    assert _counters_match(st, want, len(pr) * samples), (kind, shading, arm, samples, device, st, want["counters"].sum(0))


def test_bake_index_independence(rrt, orc):
    sc, _, _, pr = _case(rrt, orc, "helmet")
    want = _model(rrt, orc, "helmet", 3, 4)["mean"]
    n = len(pr)
    for order in (np.arange(n)[::-1], np.roll(np.arange(n), 23)):
        for device in (False, True):
            rc, got, _ = _bake(rrt, sc, pr[order], 3, 4, device=device)                    # the stride stays n: the same streams
            assert rc == 0 and PM.same_bits(got, want[order]), (device, _bad_rows(got, want[order]))
    rc, got, _ = _bake(rrt, sc, pr[:30], 3, 4, stride=n)                                   # fewer probes, the same stride
    assert rc == 0 and PM.same_bits(got, want[:30])


def test_bake_accumulate_splits_the_sum(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    sc, _, _, pr = _case(rrt, orc, "helmet")
    n = len(pr)
    whole = _model(rrt, orc, "helmet", 8, 4)
    rc, one, _ = _bake(rrt, sc, pr, 8, 4, flags=L.FLAG_SUM, device=True)
    assert rc == 0 and PM.same_bits(one, whole["sum"])
    for split in ((4, 4), (1, 5, 2)):
        d_acc = torch.zeros((n * 27 + 5,), dtype=torch.float32, device="cuda").view(torch.int32)
        d_acc[n * 27:] = SENTINEL
        first = 0
        for k in split:
            rc, got, _ = _bake(rrt, sc, pr, k, 4, flags=L.FLAG_SUM | L.FLAG_ACCUM, device=True, first_sample=first, d_out=d_acc)
            assert rc == 0
            first += k
        assert PM.same_bits(got, whole["sum"]), (split, _bad_rows(got, whole["sum"]))
    # the sums go on from what the buffer held
    d_acc = torch.full((n * 27 + 5,), 2.5, dtype=torch.float32, device="cuda").view(torch.int32)
    d_acc[n * 27:] = SENTINEL
    rc, got, _ = _bake(rrt, sc, pr, 1, 4, flags=L.FLAG_SUM | L.FLAG_ACCUM, device=True, d_out=d_acc)
    s1 = _model(rrt, orc, "helmet", 1, 4)["sum"]
    assert rc == 0 and PM.same_bits(got, np.float32(2.5) + s1)
    # the wrapper: accumulate_into, positions and seeds apart
    pos = torch.from_numpy(pr["position"].copy()).cuda()
    acc = torch.zeros((n, 9, 3), dtype=torch.float32, device="cuda")
    for first in (0, 4):
        out, _ = sc.bake_probes(pos, seeds=pr["seed"], samples=4, max_ray_depth=4, first_sample=first, accumulate_into=acc)
        assert out is acc
    assert PM.same_bits(acc.cpu().numpy(), whole["sum"])
    # refused on the host entry, the output untouched
    lib = rrt.load()
    opt = L.MiptProbeBakeOptions()
    opt.samples, opt.max_ray_depth, opt.sample_stride, opt.flags = 2, 4, n, L.FLAG_SUM | L.FLAG_ACCUM
    out = np.zeros((n, 27), np.float32)
    assert lib.mipt_probe_bake(sc._handle, L.ptr(np.ascontiguousarray(pr)), n, C.byref(opt), L.ptr(out), None) == L.ERR_INVALID_ARG
    assert "mipt_probe_bake_device" in lib.mipt_last_error().decode() and not out.any()


def test_bake_first_sample_and_stride_wrap(rrt, orc):
    sc, _, _, pr = _case(rrt, orc, "cornell")
    base = _model(rrt, orc, "cornell", 3, 4)["sum"]
    for first, stride in ((5, 1000), (0xFFFFFFFE, 3), (2, 1), (7, 0x80000001)):
        want = _model(rrt, orc, "cornell", 3, 4, first_sample=first, stride=stride)
        assert not PM.same_bits(want["sum"], base)
        for device in (False, True):
            rc, got, _ = _bake(rrt, sc, pr, 3, 4, device=device, first_sample=first, stride=stride)
            assert rc == 0 and PM.same_bits(got, want["mean"]), (first, stride, device, _bad_rows(got, want["mean"]))
    # the wrapper: sample_stride None = the number of probes; numpy positions go through the host entry
    got, st = sc.bake_probes(pr["position"], seeds=pr["seed"], samples=3, max_ray_depth=4, cull_margin=0.0)
    assert got.shape == (65, 9, 3) and PM.same_bits(got, _model(rrt, orc, "cornell", 3, 4)["mean"]) and st["pixels"] == 3 * len(pr)
    got, _ = sc.bake_probes(pr["position"], samples=1, max_ray_depth=4, sum=True)          # the default seeds: the _seeds rule
    mine = pr.copy()
    mine["seed"] = rrt.Scene.radiance_default_seeds(len(pr))
    assert PM.same_bits(got, _model(rrt, orc, "cornell", 1, 4, probes=mine, tag="default seeds")["sum"])


# ---- bake: past the lanes in flight, chunk boundaries -------------------------------------------------------------------------------------
def _periodic(rrt, orc, n):
    """n probes that repeat with PERIOD, on cornell: (the PERIOD distinct ones, the index of each of the n)"""
    _, _, caller, _ = _case(rrt, orc, "cornell")
    pr = PM.case_probes(caller, n=PERIOD, seed=21)
    pr["seed"] = 11 * np.arange(PERIOD, dtype=np.uint32) + 5
    return pr, np.arange(n) % PERIOD


def test_bake_past_the_lanes_in_flight(rrt, orc):
    """lanes_cap + 4 099 probes at one sample: every lane of the ray-generation kernel takes a second path, and the projection
    kernel's nine lanes a probe refill nine times."""
    import torch
    sc, _, _, _ = _case(rrt, orc, "cornell")
    cap = LT.lanes_cap(LT.device_n_cu())
    n = cap + 4099
    pr, index = _periodic(rrt, orc, n)
    want = _model(rrt, orc, "cornell", 1, 2, stride=n, probes=pr, tag="period 1")
    PM.conditions(want, PM.PLANTED_NAN)
    d_p = _dev(pr)[torch.from_numpy(index).cuda()].contiguous()
    rc, got, st = _bake(rrt, sc, np.empty(n, dtype=PM.PROBE), 1, 2, device=True, d_probes=d_p)
    assert rc == 0 and st["pixels"] == n
    named = [0, cap - 1, cap, cap + 1, n - 1]
    assert all(PM.same_bits(got[i], want["mean"][index[i]]) for i in named), [(i, PM.same_bits(got[i], want["mean"][index[i]])) for i in named]
    assert PM.same_bits(got, want["mean"][index]), _bad_rows(got, want["mean"][index])


def test_bake_across_a_chunk_boundary(rrt, orc):
    """Case A: 2^22 + 65 paths at three samples a probe: the chunk boundary lies INSIDE a probe's samples (2^22 is no multiple of 3),
    so its 27 sums cross in a carry slot; every probe is held to the model."""
    import torch
    sc, _, _, _ = _case(rrt, orc, "cornell")
    samples = 3
    n = ((1 << 22) + 65 + samples - 1) // samples
    assert n * samples >= (1 << 22) + 65 and (1 << 22) % samples != 0
    pr, index = _periodic(rrt, orc, n)
    want = _model(rrt, orc, "cornell", samples, 2, stride=n, probes=pr, tag="period 3")
    d_p = _dev(pr)[torch.from_numpy(index).cuda()].contiguous()
    rc, got, st = _bake(rrt, sc, np.empty(n, dtype=PM.PROBE), samples, 2, device=True, d_probes=d_p)
    assert rc == 0 and st["pixels"] == n * samples
    straddler = (1 << 22) // samples
    assert straddler * samples < (1 << 22) < (straddler + 1) * samples
    named = [straddler - 1, straddler, straddler + 1, n - 1]
    assert all(PM.same_bits(got[i], want["mean"][index[i]]) for i in named), [(i, PM.same_bits(got[i], want["mean"][index[i]])) for i in named]
    assert PM.same_bits(got, want["mean"][index]), _bad_rows(got, want["mean"][index])


def test_bake_probes_longer_than_a_chunk(rrt, orc):
    """Case B: three probes of 2^22 + 2^21 + 7 samples each at depth 1: whole chunks inside one probe and two straddles at different
    offsets.  Against the same entry in SUM | ACCUM calls of at most 2^21 samples: 2^21 divides a chunk, so no probe of such a call
    crosses one, and such calls are on the path the small cases hold to the model."""
    import torch
    from rust_ray_tracing_amd import _lib as L
    sc, _, _, pr = _case(rrt, orc, "cornell")
    three = pr[[0, 1, 2]].copy()
    per = (1 << 22) + (1 << 21) + 7
    assert per > (1 << 22) and (per % (1 << 22)) != ((2 * per) % (1 << 22)) and (1 << 22) % (1 << 21) == 0
    d_p = _dev(three)
    rc, whole, st = _bake(rrt, sc, three, per, 1, flags=L.FLAG_SUM, device=True, d_probes=d_p, stride=3)
    assert rc == 0 and st["pixels"] == 3 * per
    d_acc = torch.zeros((3 * 27 + 5,), dtype=torch.float32, device="cuda").view(torch.int32)
    d_acc[3 * 27:] = SENTINEL
    first = 0
    while first < per:
        k = min(1 << 21, per - first)
        rc, parts, _ = _bake(rrt, sc, three, k, 1, flags=L.FLAG_SUM | L.FLAG_ACCUM, device=True, d_probes=d_p, stride=3, first_sample=first, d_out=d_acc)
        assert rc == 0
        first += k
    assert np.all(np.isfinite(whole)) and np.all(whole[:, 0] > 0) and not PM.same_bits(whole[0], whole[1])
    assert PM.same_bits(whole, parts), _bad_rows(whole, parts)


# ---- bake: scene state ----------------------------------------------------------------------------------------------------------------
def test_bake_follows_refit_and_rebuild(rrt, orc):
    from rust_ray_tracing_amd import _lib as L
    tris, mats, texs = PM.case_scene(rrt, "cornell")
    sc, caller = _from_triangles(rrt, tris[np.random.default_rng(3).permutation(len(tris))], mats, texs)
    pr = PM.case_probes(caller)
    before = PM.Bake(orc, sc).run(pr, 2, 4)
    rc, got, _ = _bake(rrt, sc, pr, 2, 4)
    assert rc == 0 and PM.same_bits(got, before["mean"])
    for mode in (L.UPDATE_REFIT, L.UPDATE_REBUILD):
        new = caller.copy()
        new["vertices"]["position"] = new["vertices"]["position"] * np.float32(0.75 if mode == L.UPDATE_REFIT else 1.25)
        if mode == L.UPDATE_REBUILD:
            new["vertices"]["position"] = new["vertices"]["position"][::-1].copy()        # other positions: another tree
        sc.tris = np.ascontiguousarray(new[sc._tri_order])                                 # update_device scatters the mirror back to the caller's order
        sc.update_device(mode)
        caller = new
        after = PM.Bake(orc, sc).run(pr, 2, 4, shading=1, cull=1, margin=SAFE)
        PM.conditions(after, PM.PLANTED_NAN)
        assert not PM.same_bits(after["mean"], before["mean"])
        for device in (False, True):
            rc, got, _ = _bake(rrt, sc, pr, 2, 4, 1, CULL, device=device, cull_margin=SAFE)
            assert rc == 0 and PM.same_bits(got, after["mean"]), (mode, device, _bad_rows(got, after["mean"]))
        before = after


def test_bake_on_a_mesh_scene(rrt, orc):
    tris, mats, texs = PM.case_scene(rrt, "cornell")
    v = tris["vertices"]
    n = len(tris)
    sc = rrt.Scene.from_mesh(positions=v["position"].reshape(-1, 3), normals=v["normal"].reshape(-1, 3),
                             tex_coords=np.stack([v["tex_coord_x"], v["tex_coord_y"]], axis=-1).reshape(-1, 2),
                             indices=np.arange(n * 3, dtype=np.uint32), parts=[(0, 12, 0), (12, n - 12, 3)], materials=mats, textures=texs)
    expanded = sc.expand_mesh().copy()
    sc.upload_from_mesh(0)
    plain = rrt.Scene.from_arrays(expanded, mats, texs)                                    # the same triangles with a tree of their own, for the oracle
    pr = PM.case_probes(expanded)
    want = PM.Bake(orc, plain).run(pr, 3, 4)
    PM.conditions(want, PM.PLANTED_NAN)
    for device in (False, True):
        rc, got, _ = _bake(rrt, sc, pr, 3, 4, device=device)
        assert rc == 0 and PM.same_bits(got, want["mean"]), (device, _bad_rows(got, want["mean"]))


def test_bake_on_a_replica_handle(rrt, orc):
    from rust_ray_tracing_amd import _lib as L
    mt = L.load_multitest()
    sc, _, caller, pr = _case(rrt, orc, "cornell")
    tris, mats, texs = PM.case_scene(rrt, "cornell")
    host = rrt.Scene.from_arrays(caller, mats, texs, build_bvh=False)
    d = host.desc()
    multi = C.c_void_p()
    assert mt.mipt_multi_create_from_triangles(C.byref(d), (C.c_int * 2)(0, 0), 2, C.byref(multi)) == 0, mt.mipt_last_error()
    try:
        want = _model(rrt, orc, "cornell", 3, 4)["mean"]
        for rank in (0, 1):
            h = mt.mipt_multi_scene(multi, rank)
            for device in (False, True):
                rc, got, _ = _bake(rrt, None, pr, 3, 4, device=device, handle=h, lib=mt)
                assert rc == 0 and PM.same_bits(got, want), (rank, device, _bad_rows(got, want))
    finally:
        mt.mipt_multi_destroy(multi)


def test_bake_on_a_side_stream_and_the_wrapper(rrt, orc):
    import torch
    sc, _, _, pr = _case(rrt, orc, "wgsl_pbr")
    want = _model(rrt, orc, "wgsl_pbr", 3, 4, 1, CULL, SAFE)["mean"]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pos = torch.from_numpy(pr["position"].copy()).cuda()                               # produced on the side stream: the bake is ordered after it
        rc, got, _ = _bake(rrt, sc, pr, 3, 4, 1, CULL, device=True, cull_margin=SAFE, stream=side.cuda_stream)
        dev, st = sc.bake_probes(pos, seeds=pr["seed"], samples=3, max_ray_depth=4, traversal=CULL, shading=1)      # the wrapper's default margin
        dev2, _ = sc.bake_probes(pos, seeds=pr["seed"], samples=3, max_ray_depth=4, traversal=CULL, shading=1, stream=side.cuda_stream)
    side.synchronize()
    assert rc == 0 and PM.same_bits(got, want)
    assert dev.is_cuda and dev.shape == (65, 9, 3) and PM.same_bits(dev.cpu().numpy(), want) and PM.same_bits(dev2.cpu().numpy(), want)
    assert st["pixels"] == 65 * 3


def _render(rrt, sc):
    r = rrt.Renderer.new(rrt.RendererOptions(samples=1, max_ray_depth=3, output_image_dimensions=(32, 24), output_image_path="/dev/null"))
    return r.render_buffers(sc)[0].view(np.uint32).copy()


def test_device_entry_refusals_leave_the_scene_rendering(rrt, orc):
    import torch
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import synth
    lib = rrt.load()
    sc, _, _, pr = _case(rrt, orc, "cornell")
    cam = synth.make_scene("cornell")[3]
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    before = _render(rrt, sc)
    n = 64
    opt = L.MiptProbeBakeOptions()
    opt.samples, opt.max_ray_depth, opt.sample_stride = 2, 4, n
    d_out = torch.zeros((n, 27), dtype=torch.float32, device="cuda")
    d_p = _dev(pr[:n])
    h_buf = np.zeros(n * 27 * 4 + 16, dtype=np.uint8)
    p_ptr = h_buf.ctypes.data + (-h_buf.ctypes.data) % 16
    f = lib.mipt_probe_bake_device
    for args, msg in (((sc._handle, d_p.data_ptr(), n, C.byref(opt), p_ptr, None, None), "mipt_probe_bake_device: d_sh is not device memory of the scene's device 0"),
                      ((sc._handle, p_ptr, n, C.byref(opt), d_out.data_ptr(), None, None), "mipt_probe_bake_device: d_probes is not device memory of the scene's device 0"),
                      ((sc._handle, d_p.data_ptr() + 4, n - 1, C.byref(opt), d_out.data_ptr(), None, None), "mipt_probe_bake_device: d_probes must be 16-byte aligned"),
                      ((sc._handle, d_p.data_ptr(), n, C.byref(opt), d_out.data_ptr() + 2, None, None), "mipt_probe_bake_device: d_sh must be 4-byte aligned"),
                      ((sc._handle, d_p.data_ptr(), n, C.byref(opt), d_p.data_ptr() + 16 * (n - 1), None, None), "mipt_probe_bake_device: d_probes overlaps d_sh")):
        assert f(*args) == L.ERR_INVALID_ARG, msg
        assert lib.mipt_last_error().decode() == msg, lib.mipt_last_error()
    g = L.MiptProbeGrid()
    g.spacing[:], g.dims[:] = (1.0, 1.0, 1.0), (2, 2, 2)
    d_sh = torch.zeros((8, 27), dtype=torch.float32, device="cuda")
    d_pts = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    d_e = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    for fields, msg in ((dict(sh=p_ptr), "mipt_probe_irradiance_device: sh is not device memory"),
                        (dict(irradiance=p_ptr), "mipt_probe_irradiance_device: irradiance is not device memory of sh's device 0"),
                        (dict(valid=p_ptr), "mipt_probe_irradiance_device: valid is not device memory of sh's device 0"),
                        (dict(irradiance=d_pts.data_ptr() + 12), "mipt_probe_irradiance_device: irradiance overlaps position")):
        b = L.MiptProbeIrradianceBuffers()
        b.sh, b.position, b.normal, b.irradiance = d_sh.data_ptr(), d_pts.data_ptr(), d_pts.data_ptr(), d_e.data_ptr()
        for k, v in fields.items():
            setattr(b, k, v)
        assert lib.mipt_probe_irradiance_device(C.byref(g), n, C.byref(b), None) == L.ERR_INVALID_ARG, msg
        assert lib.mipt_last_error().decode() == msg, lib.mipt_last_error()
    torch.cuda.synchronize()
    assert torch.count_nonzero(d_out).item() == 0 and torch.count_nonzero(d_e).item() == 0 and not h_buf.any()
    assert np.array_equal(_render(rrt, sc), before)                                        # the scene renders bit-exactly afterwards
    rc, got, _ = _bake(rrt, sc, pr, 3, 4, device=True)
    assert rc == 0 and PM.same_bits(got, _model(rrt, orc, "cornell", 3, 4)["mean"])


# ---- lookup ---------------------------------------------------------------------------------------------------------------------------
def _lookup(rrt, grid, sh, P, N, valid=None, clamp=False, device=False, extra=4):
    """One call of the C entry with a sentinel behind the output -> irradiance [n, 3] f32; the sentinel is asserted"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    origin, spacing, dims = grid
    g = L.MiptProbeGrid()
    g.origin[:], g.spacing[:], g.dims[:], g.flags = origin, spacing, dims, (L.PROBE_CLAMP if clamp else 0)
    n = len(P)
    b = L.MiptProbeIrradianceBuffers()
    sh, P, N = (np.ascontiguousarray(a, dtype=np.float32) for a in (sh, P, N))
    if device:
        keep = [torch.from_numpy(a).cuda() for a in (sh, P, N)] + ([torch.from_numpy(np.ascontiguousarray(valid)).cuda()] if valid is not None else [])
        d_out = torch.full((n * 3 + extra,), SENTINEL, dtype=torch.int32, device="cuda")
        b.sh, b.position, b.normal, b.irradiance = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), d_out.data_ptr()
        b.valid = keep[3].data_ptr() if valid is not None else None
        rc = lib.mipt_probe_irradiance_device(C.byref(g), n, C.byref(b), None)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy().view(np.uint32)
    else:
        out = np.full(n * 3 + extra, SENTINEL, dtype=np.uint32)
        v = None if valid is None else np.ascontiguousarray(valid)
        b.sh, b.position, b.normal, b.irradiance = sh.ctypes.data, P.ctypes.data, N.ctypes.data, out.ctypes.data
        b.valid = None if v is None else v.ctypes.data
        rc = lib.mipt_probe_irradiance(C.byref(g), n, C.byref(b), 0)
    assert rc == 0, lib.mipt_last_error()
    assert np.all(out[n * 3:] == SENTINEL), "written past n * 3 floats"
    return out[: n * 3].view(np.float32).reshape(n, 3)


def _valid_plane(dims):
    """4 x 3 x 2: cell (0, 0, 0) wholly invalid, cell (2, 1, 0) with the single valid corner (3, 2, 1); smaller grids: two of three"""
    n = int(np.prod(dims))
    if tuple(dims) != (4, 3, 2):
        return (np.arange(n) % 3 != 1).astype(np.uint8)
    v = np.ones(n, dtype=np.uint8)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                v[(dz * 3 + dy) * 4 + dx] = 0
                v[(dz * 3 + 1 + dy) * 4 + 2 + dx] = 0
    v[(1 * 3 + 2) * 4 + 3] = 7                                                              # any non-zero byte
    return v


@pytest.mark.parametrize("dims", PM.LOOKUP_DIMS)
def test_lookup_model_parity(rrt, dims):
    grid, sh, P, N = PM.lookup_case(dims, 1000, 5)
    o, s = np.float32(PM.LOOKUP_ORIGIN), np.float32(PM.LOOKUP_SPACING)
    valid = _valid_plane(dims)
    if tuple(dims) == (4, 3, 2):
        P[900:910] = o + s * (np.float32((0.5, 0.5, 0.5)) + np.random.default_rng(1).uniform(-0.4, 0.4, (10, 3)).astype(np.float32))   # inside the invalid cell
        P[910:920] = o + s * (np.float32((2.5, 1.5, 0.5)) + np.random.default_rng(2).uniform(-0.4, 0.4, (10, 3)).astype(np.float32))   # one valid corner
        m = PM.lookup(sh, grid, P, N, valid)
        assert not m[900:910].any() and m[910:920].all()
    for v in (None, valid):
        for clamp in (False, True):
            want = PM.lookup(sh, grid, P, N, v, clamp)
            assert not np.any(np.isnan(want)) and (clamp or np.any(want < 0)) and np.any(want > 0)
            for device in (False, True):
                got = _lookup(rrt, grid, sh, P, N, v, clamp, device)
                assert PM.same_bits(got, want), (dims, v is not None, clamp, device, _bad_rows(got, want))


def test_lookup_skips_a_nan_probe_behind_a_zero_weight(rrt):
    grid, sh, _, N = PM.lookup_case((4, 3, 2), 64, 4)
    sh[5] = np.nan                                                                          # probe (1, 1, 0)
    pts = PM.grid_positions(*grid)
    P = pts[[4, 6, 1, 9, 17, 3, 11, 23]]                # on its five neighbours along x, y and z -- its weight there is exactly 0 -- and far away
    want = PM.lookup(sh, grid, P, N[: len(P)])
    assert not np.any(np.isnan(want))
    for device in (False, True):
        got = _lookup(rrt, grid, sh, P, N[: len(P)], device=device)
        assert PM.same_bits(got, want), (device, _bad_rows(got, want))


def test_lookup_past_the_lanes_in_flight(rrt):
    import torch
    cap = LT.lanes_cap(LT.device_n_cu())
    n = cap + 4099
    grid, sh, P0, N0 = PM.lookup_case((4, 3, 2), PERIOD, 6)
    index = np.arange(n) % PERIOD
    want = PM.lookup(sh, grid, P0, N0, _valid_plane((4, 3, 2)), True)
    got = _lookup(rrt, grid, sh, P0[index], N0[index], _valid_plane((4, 3, 2)), True, device=True)
    named = [0, cap - 1, cap, cap + 1, n - 1]
    assert all(PM.same_bits(got[i], want[index[i]]) for i in named), named
    assert PM.same_bits(got, want[index]), _bad_rows(got, want[index])
    # the wrapper on tensors: stream-ordered on torch's current stream, and on arrays
    t = [torch.from_numpy(a).cuda() for a in (sh, P0, N0)]
    out = rrt.probe_irradiance(t[0], grid, t[1], t[2], valid=torch.from_numpy(_valid_plane((4, 3, 2)) != 0).cuda(), clamp=True)
    assert out.is_cuda and PM.same_bits(out.cpu().numpy(), want)
    assert PM.same_bits(rrt.Scene.probe_irradiance(sh, grid, P0, N0, valid=_valid_plane((4, 3, 2)), clamp=True), want)


# ---- bake, then lookup ------------------------------------------------------------------------------------------------------------------
def test_a_box_of_emitters_gives_pi_times_the_emission(rrt, orc):
    """A closed box whose six walls emit E, depth 1: every path brings back exactly E, so the band-0 sum is N equal terms and the
    irradiance of the one-probe grid is pi * E plus what the (noisy) higher bands add, which is taken from the model's own values.
    Tolerance: the (N + 3) 2^-23 of the ordered sum plus 16 * 2^-24 for the lookup's 12 products and 8 additions, of the sum of the
    magnitudes of the terms."""
    import torch
    emission = (0.75, 0.5, 0.25)
    tris, mats = PM.box_scene(emission)
    sc = rrt.Scene.from_arrays(tris, mats, [])
    sc.upload(0)
    n = 256
    pr = np.zeros(1, dtype=PM.PROBE)
    pr["position"][0], pr["seed"][0] = (0.125, -0.25, 0.375), 12345
    want = PM.Bake(orc, sc).run(pr, n, 1)
    assert want["hit"].all() and PM.same_bits(want["radiance"], np.broadcast_to(np.float32(emission), (1, n, 3)))
    rc, sh, _ = _bake(rrt, sc, pr, n, 1, device=True)
    assert rc == 0 and PM.same_bits(sh, want["mean"])
    grid = ((0.125, -0.25, 0.375), (1.0, 1.0, 1.0), (1, 1, 1))
    rng = np.random.default_rng(8)
    N = rng.normal(0, 1, (50, 3))
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
    P = rng.uniform(-0.9, 0.9, (50, 3)).astype(np.float32)
    got = rrt.probe_irradiance(torch.from_numpy(sh).cuda(), grid, torch.from_numpy(P).cuda(), torch.from_numpy(N).cuda()).cpu().numpy().astype(np.float64)
    assert PM.same_bits(got.astype(np.float32), PM.lookup(sh, grid, P, N))
    Y = PM.basis64(N)                                                                       # [50, 9]
    A = np.array([np.pi] + [2 * np.pi / 3] * 3 + [np.pi / 4] * 5)
    terms = (A * Y)[:, :, None] * want["mean"][0].astype(np.float64)[None, :, :]           # [50, 9, 3]
    expect = np.pi * np.float64(emission)[None, :] + terms[:, 1:].sum(axis=1)
    tol = ((n + 3) * 2.0 ** -23 + 16 * 2.0 ** -24) * (np.pi * np.float64(emission)[None, :] + np.abs(terms[:, 1:]).sum(axis=1))
    assert np.all(np.abs(got - expect) <= tol), np.abs((got - expect) / tol).max()
