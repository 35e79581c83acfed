"""-m gpu: the three copies of the traversal step (pt_kernel.hip, ray_query.hip, first_hit.hip) on every form of a stack entry and on
the trees of the BVH corpus, against the models.

A pop decodes an inner pair, an inline leaf (1 <= n <= 63) or the child-ref form (n >= 64: (a, n) read again from the pair record,
`which` = 0 for the entry written after the d1 > d2 swap, 1 for the one written without it); a root leaf takes no entry.
tests/tools/traverse_cases.py makes scenes whose one large leaf is the pair's first child, its second child or the root, at 62 ... 65,
300 and 3 000 triangles, with materials that make a hit on the wrong triangle of the leaf visible, and rays that stack the leaf, enter
it directly, miss it and stop inside it; tests/test_traverse_cases_model.py proves on the CPU that they do.  The corpus trees add leaves
of hundreds of coincident triangles deep in a real tree, zero-area triangles, boxes of signed zeros and denormal widths, and a tree of
74 levels whose stack passes the 16 LDS entries.  Here:

* ray_query_kernel: every scene, closest hit and occlusion, three arms, counting and product build, host entry everywhere and device
  entry on the m = 64 scenes and `spiral` -- against query_model (hits bit for bit, NaNs as NaNs, five counters);
* first_hit_kernel: all eight buffers against features_model.frame from two cameras, one of which stacks the leaf while the other
  enters it; one explicit-motion call against motion_model (the MOTION instantiations' copy of the pop);
* the trace kernels: orc.render, reference and safely culled traversal, six counters, single view and a batch of the two cameras;
* pt_trace_rays_kernel: radiance_model.Model.trace on the ray families.

Every comparison is bit for bit; every output starts as poison and has a sentinel behind it.  Each test prints the model's seconds and
the device calls' seconds apart.  DESIGN section 21 ("Forms of a stack entry") names the test that pops each form in each loop."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import features_model as F  # noqa: E402
import motion_model as M  # noqa: E402
import query_model as Q  # noqa: E402
import radiance_model as R  # noqa: E402
import traverse_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu

SAFE = 0.0078125
REF, CULL = 0, 1
ARMS = [(REF, 0.0), (CULL, 0.0), (CULL, SAFE)]               # tests/test_gpu_query.py ARMS
TWO_ARMS = [ARMS[0], ARMS[2]]                               # the reference and the safely culled traversal
FRAME = (24, 16)                                            # first hit: 3 x 2 tiles of 8 x 8
TRACE_FRAME, TRACE_SPP, TRACE_DEPTH = (40, 24), 2, 4
POISON = 0x7FA5A5A5
TRACE_COUNTERS = ("rays", "inner_steps", "tri_tests", "hits", "texel_fetches", "max_stack")     # tests/test_gpu_parity.py


def _arm_kw(arm):
    return dict(cull=arm[0] == CULL, margin=arm[1])


def _resident(rrt, orc, m, shape):
    c = T.leaf_case(rrt, orc, m, shape)
    c["sc"].upload(0)                                        # the host builder's tree; a second call returns the same handle
    return c


_corpus = {}


def _corpus_scene(rrt, name):
    """the corpus entry resident through the device builder, tree and order fetched: (Scene, rays); the model runs on that tree, which
    tests/test_gpu_bvh_corpus.py holds to the oracle's"""
    if name not in _corpus:
        tris, rays = T.corpus_input(name)
        sc = rrt.Scene.from_arrays(np.array(tris), T.materials(), build_bvh=False)
        sc.upload_from_triangles(0, fetch_bvh=True)
        assert sc._tri_order is not None and sc.info()["built_on_device"] == 1
        _corpus[name] = (sc, rays)
    return _corpus[name]


# ---- queries ------------------------------------------------------------------------------------------------------------------------
def _check_queries(rrt, orc, sc, rays, occ_rays, entries, label):
    from test_gpu_query import _big_query, _dev, _nan_canonical
    lib = orc.load()
    t_model = t_dev = 0.0
    for arm in ARMS:
        for anyhit in (False, True):
            r = np.ascontiguousarray(occ_rays if anyhit else rays)
            t0 = time.perf_counter()
            hits, occ, per, _ = T.trace(lib, sc.tris, sc.bvh_nodes, r, anyhit=anyhit, tri_order=sc._tri_order, **_arm_kw(arm))
            t_model += time.perf_counter() - t0
            assert per["stack_overflows"].sum() == 0
            sums = T.totals(per, len(r))
            t0 = time.perf_counter()
            d_rays = _dev(r) if True in entries else None
            for device in entries:
                for count in (True, False):                                      # the counting twin, then the product build
                    got, st = _big_query(rrt, sc, r, d_rays, len(r), arm, anyhit, count, device)
                    if anyhit:
                        assert np.array_equal(got, occ), (label, arm, device, count, np.flatnonzero(got != occ)[:8])
                    else:
                        g, w = _nan_canonical(got), _nan_canonical(hits)
                        assert np.array_equal(g, w), (label, arm, device, count, [(int(i), g[i].tolist(), w[i].tolist())
                                                                                 for i in np.flatnonzero((g != w).any(axis=1))[:4]])
                    assert st["stack_overflows"] == 0 and st["kernel_ms"] > 0
                    if count:
                        assert {k: st[k] for k in Q.COUNTERS} == sums, (label, arm, anyhit, device, st, sums)
                    else:
                        assert st["rays"] == 0 and st["tri_tests"] == 0
            t_dev += time.perf_counter() - t0
    print(f"{label}: {len(rays)} rays, model {t_model:.2f} s, device calls {t_dev:.2f} s")


@pytest.mark.parametrize("shape", T.SHAPES)
@pytest.mark.parametrize("m", T.LEAF_SIZES + (T.LEAF_SIZE_BIG,))
def test_queries_on_leaf_forms(rrt, orc, m, shape):
    c = _resident(rrt, orc, m, shape)
    rays = c["rays"]
    occ_rays = rays if shape != "root" else Q.occlusion_t_max(rays, c["ref"][0])   # family (d) carries the t_max of a left / right scene
    _check_queries(rrt, orc, c["sc"], rays, occ_rays, (False, True) if m == 64 else (False,), f"queries-{m}-{shape}")


@pytest.mark.parametrize("name", T.CORPUS)
def test_queries_on_corpus_trees(rrt, orc, name):
    sc, rays = _corpus_scene(rrt, name)
    with np.errstate(all="ignore"):
        closest = T.trace(orc.load(), sc.tris, sc.bvh_nodes, rays, tri_order=sc._tri_order)[0]
        _check_queries(rrt, orc, sc, rays, Q.occlusion_t_max(rays, closest), (False, True) if name == "spiral" else (False,), f"queries-{name}")


# ---- first hit ---------------------------------------------------------------------------------------------------------------------
def _check_features(rrt, orc, sc, cams, entries, label, sky=True):
    from test_gpu_features import _features, _same
    t_model = t_dev = 0.0
    for arm in TWO_ARMS:
        t0 = time.perf_counter()
        frames = [F.frame(orc, sc, cam, FRAME[0], FRAME[1], 0, tri_order=sc._tri_order, **_arm_kw(arm))[:2] for cam in cams]
        t_model += time.perf_counter() - t0
        want = {k: np.stack([f[0][k] for f in frames]) for k in F.NAMES}
        counters = {k: sum(f[1][k] for f in frames) for k in F.COUNTERS[:-1] + ("pixels",)}
        counters["max_stack"] = max(f[1]["max_stack"] for f in frames)
        assert (want["prim"] != Q.NONE).sum() >= 16 and (not sky or (want["prim"] == Q.NONE).any())
        t0 = time.perf_counter()
        for device in entries:
            for count in (True, False):
                got, st = _features(rrt, sc._handle, cams, FRAME, 0, arm, device=device, count=count)
                assert not _same(got, want), (label, arm, device, count, _same(got, want))
                assert st["stack_overflows"] == 0 and st["pixels"] == counters["pixels"]
                if count:
                    assert {k: st[k] for k in counters} == counters, (label, arm, device, st, counters)
                else:
                    assert st["rays"] == 0 and st["tri_tests"] == 0
        t_dev += time.perf_counter() - t0
    print(f"{label}: {len(cams)} views of {FRAME[0]}x{FRAME[1]}, model {t_model:.2f} s, device calls {t_dev:.2f} s")


def _camera_events(orc, c, cams):
    """per camera: (pixels whose ray pops the bunch, pixels whose ray enters it directly), on features_model.camera_rays"""
    sc, out = c["sc"], []
    for cam in cams:
        rays = F.camera_rays(orc, sc, cam, FRAME[0], FRAME[1], 0)[0]
        popped, entered, _ = T.leaf_events(T.trace(orc.load(), sc.tris, sc.bvh_nodes, rays)[3], c["node"])
        out.append((int(popped.sum()), int(entered.sum())))
    return out


@pytest.mark.parametrize("shape", T.SHAPES)
@pytest.mark.parametrize("m", [63, 64, 65, 300])
def test_first_hit_on_leaf_forms(rrt, orc, m, shape):
    c = _resident(rrt, orc, m, shape)
    sc = c["sc"]
    cams = T.leaf_cameras(sc.tris, sc.bvh_nodes, m)
    ev = _camera_events(orc, c, cams)
    if shape == "root":
        assert all(e == (0, FRAME[0] * FRAME[1]) for e in ev)                     # every pixel starts in the leaf
    else:
        assert ev[0][0] >= 8 and ev[1][1] >= 8, ev                                # one camera stacks the bunch, the other enters it
    _check_features(rrt, orc, sc, cams, (False, True) if m == 64 else (False,), f"first-hit-{m}-{shape}")


@pytest.mark.parametrize("name", ["size513_copies", "spiral_small"])
def test_first_hit_on_corpus_trees(rrt, orc, name):
    sc, _ = _corpus_scene(rrt, name)
    tris = T.corpus_input(name)[0]
    core = name if name in T.CORE_VIEW else None             # every pixel down all the levels into the core; the soup with sky around it
    cams = [T.corpus_camera(tris, through_core=core)] + ([T.corpus_camera(tris, at_first=True)] if "copies" in name else [])
    _check_features(rrt, orc, sc, cams, (False,), f"first-hit-{name}", sky=core is None)


def test_motion_pops_the_child_ref_form(rrt, orc):
    """first_hit_kernel's MOTION instantiations: the explicit previous positions of the m = 64 left scene from both cameras"""
    from test_gpu_motion import _motion
    c = _resident(rrt, orc, 64, "left")
    sc = c["sc"]
    cams = T.leaf_cameras(sc.tris, sc.bvh_nodes, 64)
    assert _camera_events(orc, c, cams)[0][0] >= 8
    prev = np.array(sc.tris)
    prev["vertices"]["position"] += np.random.default_rng(9).normal(0.0, 0.05, prev["vertices"]["position"].shape).astype(np.float32)
    for arm in TWO_ARMS:
        t0 = time.perf_counter()
        want = np.stack([M.frame(orc, sc, cam, FRAME[0], FRAME[1], 0, prev, **_arm_kw(arm)) for cam in cams])
        t1 = time.perf_counter()
        assert (want != 0).any(axis=-1).sum() >= 16
        for device in (False, True):
            got, _ = _motion(rrt, sc._handle, cams, FRAME, prev, 0, arm, device=device)
            assert M.same_bits(got, want), (arm, device)
        print(f"motion-64-left {arm}: model {t1 - t0:.2f} s, device calls {time.perf_counter() - t1:.2f} s")


# ---- the trace kernels ---------------------------------------------------------------------------------------------------------------
def _render(rrt, handle, cams, arm, flags):
    """mipt_render (one camera) or mipt_render_batch (several) into poisoned buffers with a sentinel behind them
    -> (hdr [V,H,W,3] float32, rgba [V,H,W,4] uint8, stats)"""
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    w, h = TRACE_FRAME
    n = len(cams) * w * h
    opt = rrt.make_options(w, h, TRACE_SPP, TRACE_DEPTH, traversal=arm[0], flags=flags, cull_margin=arm[1])
    hdr = np.full(n * 3 + 1, POISON, dtype=np.uint32)
    rgba = np.full(n * 4 + 4, 0x5A, dtype=np.uint8)
    st = L.MiptStats()
    table = np.ascontiguousarray(np.stack([np.asarray(cam, dtype=L.CAMERA).reshape(()) for cam in cams]))
    if len(cams) == 1:
        rc = lib.mipt_render(handle, L.ptr(table), C.byref(opt), L.ptr(hdr), L.ptr(rgba), C.byref(st))
    else:
        rc = lib.mipt_render_batch(handle, L.ptr(table), len(cams), C.byref(opt), L.ptr(hdr), L.ptr(rgba), C.byref(st))
    assert rc == 0, lib.mipt_last_error()
    assert hdr[-1] == POISON and np.all(rgba[-4:] == 0x5A) and not np.any(hdr[:-1] == POISON)
    return hdr[:-1].view(np.float32).reshape(len(cams), h, w, 3), rgba[:-4].reshape(len(cams), h, w, 4), st.as_dict()


def _same_frame(a, b):
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _check_trace(rrt, orc, sc, cams, label, batch=False, min_stack=0):
    from rust_ray_tracing_amd import _lib as L
    w, h = TRACE_FRAME
    t_model = t_dev = 0.0
    for arm in TWO_ARMS:
        t0 = time.perf_counter()
        refs = [orc.render(sc.tris, sc.bvh_nodes, sc.materials_array(), [], cam, w, h, TRACE_SPP, TRACE_DEPTH, cull=arm[0], cull_margin=arm[1])
                for cam in cams]
        t_model += time.perf_counter() - t0
        assert all(r[2]["hits"] >= 16 and r[2]["hits"] < r[2]["rays"] and r[2]["max_stack"] >= min_stack for r in refs), label
        t0 = time.perf_counter()
        for v, cam in enumerate(cams):
            ref, ref_rgba, rst = refs[v]
            hdr, rgba, st = _render(rrt, sc._handle, [cam], arm, L.FLAG_COUNT)
            assert _same_frame(hdr[0], ref), (label, arm, v, int(np.sum(hdr[0].view(np.uint32) != ref.view(np.uint32))))
            assert np.array_equal(rgba[0], ref_rgba) and st["pixels"] == w * h and st["stack_overflows"] == 0
            assert {k: st[k] for k in TRACE_COUNTERS} == {k: rst[k] for k in TRACE_COUNTERS}, (label, arm, v, st, rst)
            hdr, rgba, st = _render(rrt, sc._handle, [cam], arm, 0)                # the product build
            assert _same_frame(hdr[0], ref) and np.array_equal(rgba[0], ref_rgba), (label, arm, v, "flags 0")
        if batch:
            for flags in (0, L.FLAG_COUNT):
                hdr, rgba, st = _render(rrt, sc._handle, cams, arm, flags)
                for v in range(len(cams)):
                    assert _same_frame(hdr[v], refs[v][0]) and np.array_equal(rgba[v], refs[v][1]), (label, arm, v, flags, "batch")
                assert st["pixels"] == len(cams) * w * h and st["stack_overflows"] == 0
                if flags:
                    for k in TRACE_COUNTERS[:-1]:
                        assert st[k] == sum(r[2][k] for r in refs), (label, arm, k)
                    assert st["max_stack"] == max(r[2]["max_stack"] for r in refs)
        t_dev += time.perf_counter() - t0
    print(f"{label}: {len(cams)} cameras at {w}x{h}, oracle {t_model:.2f} s, device calls {t_dev:.2f} s")


@pytest.mark.parametrize("m,shape", [(m, s) for m in (63, 64, 65, T.LEAF_SIZE_BIG) for s in ("left", "right")] + [(64, "root")])
def test_trace_on_leaf_forms(rrt, orc, m, shape):
    """single views from both cameras; on the m = 64 and m = 3 000 left scenes also one batch of the two.  A leaf of 3 000 keeps lanes
    in a leaf for thousands of iterations while others wait for a leaf phase: the schedule's worst mix, and the frame must not change."""
    c = _resident(rrt, orc, m, shape)
    sc = c["sc"]
    _check_trace(rrt, orc, sc, T.leaf_cameras(sc.tris, sc.bvh_nodes, m), f"trace-{m}-{shape}", batch=shape == "left" and m in (64, T.LEAF_SIZE_BIG))


@pytest.mark.parametrize("name", ["size2049_copies", "spiral"])
def test_trace_on_corpus_trees(rrt, orc, name):
    sc, _ = _corpus_scene(rrt, name)
    tris = T.corpus_input(name)[0]
    cams = [T.corpus_camera(tris, through_core=name if name in T.CORE_VIEW else None)] + ([T.corpus_camera(tris, at_first=True)] if "copies" in name else [])
    _check_trace(rrt, orc, sc, cams, f"trace-{name}", min_stack=17 if name == "spiral" else 4)


# ---- radiance queries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["left", "right"])
def test_radiance_queries_on_the_child_ref_form(rrt, orc, shape):
    from rust_ray_tracing_amd import _lib as L
    from test_gpu_radiance import _bad_rows, _call
    c = _resident(rrt, orc, 64, shape)
    sc = c["sc"]
    rays = np.array(c["rays"]).view(R.RAY)
    rays["reserved"] = R.default_seeds(len(rays))
    model = R.Model(orc, sc)
    samples, depth = 2, 3
    t_model = t_dev = 0.0
    for arm in TWO_ARMS:
        t0 = time.perf_counter()
        want = model.trace(rays, samples, depth, shading=0, cull=arm[0], margin=arm[1])
        counted = model.trace(rays, samples, depth, shading=1, cull=arm[0], margin=arm[1])
        t_model += time.perf_counter() - t0
        assert not np.any(np.isnan(want["mean"])) and (want["mean"] != 0).any(axis=1).sum() * 4 >= len(rays)
        t0 = time.perf_counter()
        for device in (False, True):
            for flags in (0, L.FLAG_COUNT):
                rc, got, st = _call(rrt, sc, rays, samples, depth, 0, arm[0], flags, device, cull_margin=arm[1])
                assert rc == 0 and R.same_bits(got, want["mean"]), (shape, arm, device, flags, _bad_rows(got, want["mean"]))
                assert st["stack_overflows"] == 0 and st["pixels"] == len(rays)
            rc, got, st = _call(rrt, sc, rays, samples, depth, 1, arm[0], L.FLAG_COUNT, device, cull_margin=arm[1])
            assert rc == 0 and R.same_bits(got, counted["mean"]), (shape, arm, device, "wgsl", _bad_rows(got, counted["mean"]))
            assert {k: st[k] for k in R.COUNTERS} == dict(zip(R.COUNTERS, counted["counters"].sum(0).tolist())), (shape, arm, device, st)
        t_dev += time.perf_counter() - t0
    print(f"radiance-64-{shape}: {len(rays)} rays, model {t_model:.2f} s, device calls {t_dev:.2f} s")
