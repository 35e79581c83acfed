"""-m gpu: resident indexed meshes -- mipt_scene_create_from_mesh, mipt_scene_set_transforms, mipt_scene_update_mesh_device,
mipt_scene_mesh_info (csrc/scene_mesh.hip).

The yardstick everywhere is the host restatement of the expansion rule (mipt_mesh_expand, itself pinned to the numpy model by
tests/test_mesh_host.py) fed to the plain-triangle entries: a mesh scene must be THAT scene -- layout bytes, tree, info, frame --
at create time and after every update, and errors must leave it untouched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mesh_model  # noqa: E402

FAMILIES = ["cornell", "helmet", "atrium", "dragon", "soup1", "soup17", "soup300d", "soup9000d"]


def _case(name):
    from test_gpu_scene_update import _case as case
    return case(name)


def _helpers():
    import test_gpu_scene_update as u
    return u


def _rot(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _mat4(lin, trans=(0.0, 0.0, 0.0)):
    m = np.zeros((4, 4), dtype=np.float32)
    m[:3, :3] = np.asarray(lin, dtype=np.float64).T
    m[3, :3] = trans
    m[3, 3] = 1.0
    return m.reshape(16)


def _pose(n_parts, seed, spread):
    """parts moving apart (spread > 0) or through each other (spread ~ 0 with rotations): small rotations, scales and offsets"""
    rng = np.random.default_rng(seed)
    out = []
    for p in range(n_parts):
        lin = _rot(rng) if p % 3 == 0 else np.eye(3)
        lin = np.eye(3) + 0.15 * (lin - np.eye(3))
        if p % 4 == 1:
            lin = lin @ np.diag([1.0, 1.25, 0.8])
        if p % 5 == 2:
            lin = lin @ np.diag([1.0, 1.0, -1.0])                  # a mirror
        out.append(_mat4(lin, rng.normal(0, spread, 3)))
    return np.stack(out)


def _mesh_scene(rrt, name, min_parts=6, shared=False, transforms=None, empty_parts=1, upload=True, fetch_bvh=False):
    tris, mats, texs, cam = _case(name)
    mesh, perm = mesh_model.mesh_from_triangles(tris, min_parts, shared=shared, empty_parts=empty_parts)
    sc = rrt.Scene.from_mesh(materials=mats, textures=texs, transforms=transforms, **mesh)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    if upload:
        sc.upload_from_mesh(0, fetch_bvh=fetch_bvh)
    return sc, (mats, texs, cam)


def _plain_scene(rrt, tris, mats, texs, cam, fetch_bvh=False):
    sc = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)
    sc.upload_from_triangles(0, fetch_bvh=fetch_bvh)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    return sc


def _expand_host(rrt, sc, transforms="own"):
    """mipt_mesh_expand of sc's mesh (with other transforms if given) without touching sc"""
    tmp = rrt.Scene()
    tmp.mesh = dict(sc.mesh)
    if not isinstance(transforms, str):
        tmp._set_mesh_transforms(transforms)
    return tmp.expand_mesh().copy()


def _bvh(rrt, handle, n):
    from rust_ray_tracing_amd import _lib as L
    nodes = np.zeros(2 * n, dtype=L.NODE)
    order = np.zeros(n, dtype=np.uint32)
    cnt = C.c_uint32()
    assert rrt.load().mipt_scene_get_bvh(handle, L.ptr(nodes), len(nodes), C.byref(cnt), L.ptr(order)) == 0
    return nodes[: cnt.value].copy(), order


def _same_scene(rrt, a, b, what, frames=True):
    """layout bytes + hash, tree, info size fields, one counted frame"""
    u = _helpers()
    la, lb = u._layout(rrt, a._handle), u._layout(rrt, b._handle)
    assert la[0].size == lb[0].size and la[1].size == lb[1].size, what + ": sizes"
    assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1]) and la[2] == lb[2], what + ": layout bytes differ"
    ia, ib = a.info(), b.info()
    for k in ("n_tris", "n_nodes", "n_pair_records", "max_leaf", "geometry_bytes", "built_on_device"):
        assert ia[k] == ib[k], (what, k)
    na, oa = _bvh(rrt, a._handle, ia["n_tris"])
    nb, ob = _bvh(rrt, b._handle, ib["n_tris"])
    assert na.tobytes() == nb.tobytes() and np.array_equal(oa, ob), what + ": mipt_scene_get_bvh differs"
    if frames:
        fa, pa, sa = u._render(rrt, a)
        fb, pb, sb = u._render(rrt, b)
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and np.array_equal(pa, pb), what + ": frame differs"
        for k in ("rays", "inner_steps", "tri_tests", "hits", "texel_fetches", "max_stack"):
            assert sa[k] == sb[k], (what, k)
    return la


@pytest.mark.parametrize("name", FAMILIES)
def test_create_from_mesh_is_create_from_expanded_triangles(rrt, name):
    """(5)"""
    for shared, with_xf in ((False, False), (False, True), (True, True)):
        probe, _ = _mesh_scene(rrt, name, shared=shared, upload=False)
        xf = _pose(len(probe.mesh["parts"]), 31, 0.3).reshape(-1, 4, 4) if with_xf else None
        sc, (mats, texs, cam) = _mesh_scene(rrt, name, shared=shared, transforms=xf)
        ref = _plain_scene(rrt, _expand_host(rrt, sc), mats, texs, cam)
        _same_scene(rrt, sc, ref, f"{name} shared={shared} transforms={with_xf}")
        mi = sc.mesh_info()
        m = sc.mesh
        assert mi["n_tris"] == len(ref.tris) and mi["n_parts"] == len(m["parts"]) and mi["has_transforms"] == int(with_xf)
        assert mi["n_positions"] == len(m["positions"]) and mi["n_indices"] == m["indices"].size
        assert mi["index_streams"] == (1 if shared else 3) and mi["expanded_bytes"] == 112 * len(ref.tris)
        arrays = sum(a.nbytes for k, a in m.items() if a is not None and k != "transforms")
        assert arrays <= mi["array_bytes"] <= arrays + 400 * len(m["parts"]) + 64 and mi["hbm_bytes"] == mi["array_bytes"] + mi["expanded_bytes"]
        sc.release()
        ref.release()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["cornell", "helmet", "atrium", "dragon", "soup300d"])
def test_set_transforms_equals_update_triangles(rrt, orc, name, mode):
    """(6) three poses; REFIT compares with a plain scene REFITTED the same way (the record order is the original tree's)"""
    from rust_ray_tracing_amd import _lib as L
    u = _helpers()
    lib = rrt.load()
    sc, (mats, texs, cam) = _mesh_scene(rrt, name, min_parts=8)
    first = u._layout(rrt, sc._handle)
    ref = _plain_scene(rrt, _expand_host(rrt, sc), mats, texs, cam)
    n_parts = len(sc.mesh["parts"])
    for step, (seed, spread) in enumerate(((41, 0.6), (42, 0.02), (43, 1.5))):
        xf = _pose(n_parts, seed, spread)
        inf = sc.set_transforms(xf, mode)
        assert inf["n_tris"] == len(ref.tris) and inf["build_ms"] > 0.0 and inf["upload_ms"] >= 0.0
        assert sc.mesh_info()["has_transforms"] == 1
        new = _expand_host(rrt, sc)
        assert lib.mipt_scene_update_triangles(ref._handle, L.ptr(new), len(new), mode, None) == 0, lib.mipt_last_error()
        _same_scene(rrt, sc, ref, f"{name} mode {mode} pose {step}")
        nodes, order = _bvh(rrt, sc._handle, len(new))
        u._oracle_check(rrt, orc, sc, new[order], nodes)
    # back to no transforms: the original triangles; a REBUILD restores the first layout byte for byte
    sc.set_transforms(None, mode)
    assert sc.mesh_info()["has_transforms"] == 0
    new = _expand_host(rrt, sc)
    assert lib.mipt_scene_update_triangles(ref._handle, L.ptr(new), len(new), mode, None) == 0
    last = _same_scene(rrt, sc, ref, f"{name} mode {mode} back to none")
    if mode == 1:
        assert np.array_equal(last[0], first[0]) and np.array_equal(last[1], first[1]) and last[2] == first[2]


def test_host_mirror_follows_updates(rrt, orc):
    """Scene.set_transforms keeps tris / bvh_nodes describing the device (fetch_bvh), in both modes"""
    u = _helpers()
    sc, _ = _mesh_scene(rrt, "helmet", min_parts=5, fetch_bvh=True)
    u._oracle_check(rrt, orc, sc, sc.tris, sc.bvh_nodes)
    for mode, seed in ((0, 1), (1, 2), (0, 3)):
        sc.set_transforms(_pose(len(sc.mesh["parts"]), seed, 0.4), mode)
        u._oracle_check(rrt, orc, sc, sc.tris, sc.bvh_nodes)


@pytest.mark.parametrize("mode", [0, 1])
def test_update_mesh_device_equals_the_host_route(rrt, mode):
    """(7) torch tensors: positions only, normals only, transforms only, all three; on a side stream after queued work"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    probe, _ = _mesh_scene(rrt, "atrium", min_parts=8, upload=False)
    n_parts = len(probe.mesh["parts"])
    sc, (mats, texs, cam) = _mesh_scene(rrt, "atrium", min_parts=8, transforms=_pose(n_parts, 5, 0.1).reshape(-1, 4, 4))
    ref = _plain_scene(rrt, _expand_host(rrt, sc), mats, texs, cam)
    rng = np.random.default_rng(8)
    host = dict(sc.mesh)
    side = torch.cuda.Stream()
    for step, what in enumerate((("positions",), ("normals",), ("transforms",), ("positions", "normals", "transforms"))):
        args, keep = {}, {}
        if "positions" in what:
            host["positions"] = (host["positions"] + rng.normal(0, 0.02, host["positions"].shape)).astype(np.float32)
        if "normals" in what:
            host["normals"] = (-host["normals"]).astype(np.float32)
        if "transforms" in what:
            host["transforms"] = _pose(n_parts, 60 + step, 0.5)
        use_side = step % 2 == 1
        with torch.cuda.stream(side if use_side else torch.cuda.current_stream()):
            busy = torch.ones(1 << 22, device="cuda:0")
            for _ in range(8):                                       # queued work the update must come after
                busy = busy * 1.0001
            for k in what:
                args[k] = torch.from_numpy(host[k]).to("cuda:0")
                keep[k] = args[k].clone()
            inf = sc.update_mesh_device(mode=mode, stream=side if use_side else None, **args)
        assert inf["upload_ms"] == 0.0 and inf["build_ms"] > 0.0
        torch.cuda.synchronize()
        for k in what:
            assert torch.equal(args[k], keep[k]), f"the device entry modified {k}"
        tmp = rrt.Scene()
        tmp.mesh = dict(host)
        new = tmp.expand_mesh()
        assert lib.mipt_scene_update_triangles(ref._handle, L.ptr(new), len(new), mode, None) == 0, lib.mipt_last_error()
        _same_scene(rrt, sc, ref, f"mode {mode} step {step} {what}")
    # what became resident is what the next transform-only update expands
    host["transforms"] = _pose(n_parts, 99, 0.2)
    sc.set_transforms(host["transforms"], mode)
    tmp = rrt.Scene()
    tmp.mesh = dict(host)
    new = tmp.expand_mesh()
    assert lib.mipt_scene_update_triangles(ref._handle, L.ptr(new), len(new), mode, None) == 0
    _same_scene(rrt, sc, ref, "resident arrays after device updates")


def test_bad_position_index_at_create(rrt):
    """(8) detected by the expansion kernel; nothing is left behind and the next create works"""
    from rust_ray_tracing_amd import _lib as L
    u = _helpers()
    lib = rrt.load()
    sc, (mats, texs, cam) = _mesh_scene(rrt, "helmet", upload=False)
    good = sc.mesh["indices"].copy()
    for entry in (0, good.size // 2, good.size - 1):
        sc.mesh["indices"] = good.copy()
        sc.mesh["indices"][entry] = len(sc.mesh["positions"])
        d, md = sc.desc(), sc.mesh_desc()
        h = C.c_void_p(0x1234)
        rc = lib.mipt_scene_create_from_mesh(C.byref(d), C.byref(md), 0, C.byref(h))
        msg = lib.mipt_last_error().decode()
        assert rc == L.ERR_INVALID_ARG and h.value is None and f"index entry {entry} " in msg, msg
    sc.mesh["indices"] = good
    sc.upload_from_mesh(0)
    ref = _plain_scene(rrt, _expand_host(rrt, sc), mats, texs, cam)
    _same_scene(rrt, sc, ref, "create after failed creates")


def test_errors_leave_a_live_scene_untouched(rrt):
    """(8)"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    u = _helpers()
    lib = rrt.load()
    sc, (mats, texs, cam) = _mesh_scene(rrt, "helmet", min_parts=6)
    n_parts = len(sc.mesh["parts"])
    h = sc._handle
    before = u._layout(rrt, h)
    f0, _, _ = u._render(rrt, sc)
    tris = _expand_host(rrt, sc)
    d_tris = torch.from_numpy(tris.view(np.uint8).copy()).to("cuda:0")
    ok_pose = _pose(n_parts, 70, 0.3)

    def untouched(what):
        assert u._layout(rrt, h)[2] == before[2], what
        f, _, _ = u._render(rrt, sc)
        assert np.array_equal(f.view(np.uint32), f0.view(np.uint32)), what
        assert sc.mesh_info()["has_transforms"] == 0, what

    def still_works():
        assert lib.mipt_scene_set_transforms(h, L.ptr(ok_pose), n_parts, 0, None) == 0, lib.mipt_last_error()
        assert u._layout(rrt, h)[2] != before[2]
        assert lib.mipt_scene_set_transforms(h, None, n_parts, 1, None) == 0, lib.mipt_last_error()
        untouched("restored")

    big = ok_pose.copy()
    big[1, 12] = 3e12                                               # a translation beyond 2^40
    nonfinite = ok_pose.copy()
    nonfinite[2, 0] = np.inf
    for mode in (0, 1):
        for label, xf in (("2^40", big),) + ((("inf", nonfinite),) if mode == 0 else ()):   # (BVH::build is not fed infinities)
            rc = lib.mipt_scene_set_transforms(h, L.ptr(xf), n_parts, mode, None)
            assert rc == L.ERR_SCENE_LIMIT and b"2^40" in lib.mipt_last_error(), (label, rc, lib.mipt_last_error())
            untouched(label)
            still_works()
        d_xf = torch.from_numpy(big).to("cuda:0")
        assert lib.mipt_scene_update_mesh_device(h, None, None, d_xf.data_ptr(), mode, None, None) == L.ERR_SCENE_LIMIT
        untouched("device entry 2^40")
    for call, words in ((lambda: lib.mipt_scene_update_triangles(h, L.ptr(tris), len(tris), 0, None), b"scene owns a mesh"),
                        (lambda: lib.mipt_scene_update_triangles_device(h, d_tris.data_ptr(), len(tris), 0, None, None), b"scene owns a mesh"),
                        (lambda: lib.mipt_scene_update_triangles(h, L.ptr(tris), len(tris), 1, None), b"scene owns a mesh"),
                        (lambda: lib.mipt_scene_set_transforms(h, L.ptr(ok_pose), n_parts + 1, 0, None), b"parts"),
                        (lambda: lib.mipt_scene_set_transforms(h, L.ptr(ok_pose), n_parts, 2, None), b"neither")):
        assert call() == L.ERR_INVALID_ARG and words in lib.mipt_last_error(), lib.mipt_last_error()
        untouched(words)
    still_works()
    # every mesh call on a plain scene
    plain = _plain_scene(rrt, tris, mats, texs, cam)
    p_before = u._layout(rrt, plain._handle)[2]
    mi = L.MiptMeshInfo()
    for call in (lambda: lib.mipt_scene_set_transforms(plain._handle, L.ptr(ok_pose), n_parts, 0, None),
                 lambda: lib.mipt_scene_update_mesh_device(plain._handle, None, None, None, 0, None, None),
                 lambda: lib.mipt_scene_mesh_info(plain._handle, C.byref(mi))):
        assert call() == L.ERR_INVALID_ARG and b"has no mesh" in lib.mipt_last_error(), lib.mipt_last_error()
    assert u._layout(rrt, plain._handle)[2] == p_before
    assert lib.mipt_scene_update_triangles(plain._handle, L.ptr(tris), len(tris), 0, None) == 0     # plain scenes behave as before


def test_sequence_neither_drifts_nor_leaks(rrt):
    """(9) 40 transform updates on the atrium, every fifth a REBUILD"""
    import torch
    u = _helpers()
    sc, (mats, texs, cam) = _mesh_scene(rrt, "atrium", min_parts=16)
    n_parts = len(sc.mesh["parts"])
    sc.set_transforms(_pose(n_parts, 500, 0.2), 0)
    sc.set_transforms(_pose(n_parts, 501, 0.2), 1)
    sc.set_transforms(_pose(n_parts, 502, 0.2), 0)                  # the state measured below: a REFIT last, its plan cached
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for i in range(40):
        xf = _pose(n_parts, 600 + i, 0.25)
        sc.set_transforms(xf, 1 if i % 5 == 4 else 0)
    last = xf
    fresh, _ = _mesh_scene(rrt, "atrium", min_parts=16, transforms=last.reshape(-1, 4, 4))
    _same_scene(rrt, sc, fresh, "after 40 updates (the last one a REBUILD)")
    fresh.release()
    sc.set_transforms(last, 0)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    geom = sc.info()["geometry_bytes"]
    assert free0 - free1 < geom, f"{(free0 - free1) / 2**20:.1f} MiB more in use after 41 updates (geometry: {geom / 2**20:.1f} MiB)"


def test_batch_render_of_a_mesh_scene(rrt):
    """(10) mipt_render_batch on a mesh scene after a transform update == four mipt_render calls"""
    from rust_ray_tracing_amd import _lib as L
    sc, (mats, texs, cam) = _mesh_scene(rrt, "atrium", min_parts=8)
    sc.set_transforms(_pose(len(sc.mesh["parts"]), 77, 0.3), 0)
    r = rrt.Renderer.new(rrt.RendererOptions(samples=2, max_ray_depth=6, output_image_dimensions=(64, 36), output_image_path="/dev/null"))
    cams = [rrt.Camera(position=(cam[0][0] + 0.5 * i, cam[0][1], cam[0][2] - 0.25 * i), pitch=cam[1] + 2.0 * i, yaw=cam[2] - 5.0 * i) for i in range(4)]
    for c in cams:
        c.update_view()
    hdr, rgba, st = r.render_buffers_batch(sc, cams, flags=L.FLAG_COUNT)
    rays = 0
    for i, c in enumerate(cams):
        sc.camera = c
        f, p, s = r.render_buffers(sc, flags=L.FLAG_COUNT)
        assert np.array_equal(hdr[i].view(np.uint32), f.view(np.uint32)) and np.array_equal(rgba[i], p), f"view {i}"
        rays += s["rays"]
    assert st["rays"] == rays
