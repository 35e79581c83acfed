"""-m gpu: the texel pool and the two material tables of a scene, read back from every kind of handle the library makes --
mipt_scene_create, mipt_scene_create_from_triangles, mipt_scene_create_from_mesh, and every rank's replica of mipt_multi_create /
mipt_multi_create_from_triangles with 2 and 3 logical ranks (libmipt_multitest.so) -- for texture lists from none over pools of one
to four texels (smaller than the 16 bytes a replica copies at least) to textures of 9 MB and of 17.6 MB with a 1x1 texture placed
behind them.  The uploader (scene_device.hip StagedUploader) sends a copy below two of its 8 MiB chunks straight through hipMemcpy
unless its pinned ring is up already, and the panel's triangles are far too few to bring it up: so the 9 MB texture is one plain
copy, and it is the 17.6 MB one that goes through the ring -- two whole chunks and a ragged third -- with the 1x1 behind it taking
the ring as well, as a chunk of four bytes.

For every handle: the pool is the caller's textures concatenated in order; both material tables are what the caller's materials and
the textures' prefix-sum offsets, widths and heights say, byte for byte, hence equal across all handles; and a small frame rendered
on the handle equals the oracle's bits.  After everything is destroyed, free device memory is back within MEMORY_SLACK -- a bound
that only a gross leak exceeds: every scene here is 192 triangles.  The two large lists are held to a bound that means something
for them: less than ONE of their texel pools may be missing, so a pool that any one handle or replica kept would show."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))

import mesh_model  # noqa: E402
import uv_panel as P  # noqa: E402

# texture lists as (height, width).  "large": 9 MB, one plain copy; "ring": 17.6 MB >= two 8 MiB chunks, so through the pinned ring
LISTS = {
    "none": (),
    "1x1": ((1, 1),),
    "1x1x3": ((1, 1), (1, 1), (1, 1)),
    "1x3": ((1, 3),),
    "2x2": ((2, 2),),
    "four": ((5, 3), (1, 1), (7, 2), (16, 16)),
    "large": ((1500, 1500), (1, 1)),
    "ring": ((2100, 2100), (1, 1)),
}
FRAME = (16, 12, 2, 3)                                                            # width, height, samples, depth
MEMORY_SLACK = 200000 * 112        # bytes: what test_failed_calls_give_their_memory_back allows (one array of its 200 000 triangles)

DEV_MATERIAL = np.dtype([("base", "<f4", 3), ("base_off", "<u4"), ("emis", "<f4", 3), ("emis_off", "<u4"), ("base_w", "<u4"), ("base_h", "<u4"),
                         ("emis_w", "<u4"), ("emis_h", "<u4"), ("pad", "<u4", 4)])
DEV_MATERIAL_FULL = np.dtype([("base", "<f4", 3), ("transmission", "<f4"), ("emission", "<f4", 3), ("ior", "<f4"), ("roughness", "<f4"),
                              ("metallic", "<f4"), ("transparency", "<f4"), ("pad0", "<u4"), ("tex", "<u4", (6, 3)), ("pad1", "<u4", 2)])
assert DEV_MATERIAL.itemsize == 64 and DEV_MATERIAL_FULL.itemsize == 128
SLOTS = ("base_color_tex_id", "transparency_tex_id", "roughness_tex_id", "metallic_tex_id", "emission_tex_id", "normal_tex_id")
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def mt(rrt):
    from rust_ray_tracing_amd import _lib as L
    return L.load_multitest()


def _expected_tables(mats, texs):
    """the two tables from the caller's arrays: descriptor = (prefix-sum offset, width, height) of the texture, zeros for no texture"""
    sizes = [t.shape[0] * t.shape[1] for t in texs]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    desc = lambda tid: (0, 0, 0) if tid == NONE else (int(offs[tid]), texs[tid].shape[1], texs[tid].shape[0])  # noqa: E731
    a, b = np.zeros(len(mats), dtype=DEV_MATERIAL), np.zeros(len(mats), dtype=DEV_MATERIAL_FULL)
    for i, m in enumerate(mats):
        a[i]["base"], a[i]["emis"] = m["base_color"], m["emission"]
        a[i]["base_off"], a[i]["base_w"], a[i]["base_h"] = desc(int(m["base_color_tex_id"]))
        a[i]["emis_off"], a[i]["emis_w"], a[i]["emis_h"] = desc(int(m["emission_tex_id"]))
        b[i]["base"], b[i]["emission"] = m["base_color"], m["emission"]
        for k in ("transmission", "ior", "roughness", "metallic", "transparency"):
            b[i][k] = m[k]
        for s, slot in enumerate(SLOTS):
            b[i]["tex"][s] = desc(int(m[slot]))
    return a, b


def _read(diag, handle, which, n_bytes):
    out = np.full(n_bytes + 4, 0xA5, dtype=np.uint8)
    if n_bytes:
        assert diag.mipt_diag_scene_read(handle, which, out.ctypes.data, n_bytes) == 0
    assert diag.mipt_diag_scene_read(handle, which, out.ctypes.data, n_bytes + 1) == -1      # the payload, not the padded allocation
    assert (out[n_bytes:] == 0xA5).all()
    return out[:n_bytes]


def _check_handle(rrt, diag, lib, handle, what, pool, tables, cam, ref, ref_rgba):
    from rust_ray_tracing_amd import _lib as L
    sizes = (C.c_uint64 * 3)()
    assert diag.mipt_diag_scene_tables(handle, C.byref(sizes)) == 0
    assert list(sizes) == [pool.nbytes, tables[0].nbytes, tables[1].nbytes], (what, list(sizes))
    got = _read(diag, handle, 2, pool.nbytes)
    if not np.array_equal(got, pool.view(np.uint8)):
        bad = int(np.flatnonzero(got.view(np.uint32) != pool)[0])
        raise AssertionError(f"{what}: texel pool differs from the caller's textures, first at texel {bad} of {pool.size}")
    assert np.array_equal(_read(diag, handle, 3, tables[0].nbytes), tables[0].view(np.uint8).reshape(-1)), f"{what}: 64-B material table"
    assert np.array_equal(_read(diag, handle, 4, tables[1].nbytes), tables[1].view(np.uint8).reshape(-1)), f"{what}: 128-B material table"
    w, h, spp, depth = FRAME
    o = rrt.make_options(w, h, spp, depth)
    hdr, rgba = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 4), np.uint8)
    assert lib.mipt_render(handle, L.ptr(cam), C.byref(o), L.ptr(hdr), L.ptr(rgba), None) == 0, (what, lib.mipt_last_error())
    same = (hdr.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(hdr) & np.isnan(ref))
    assert same.all() and np.array_equal(rgba, ref_rgba), f"{what}: the frame differs from the oracle's"


def _run_list(rrt, orc, mt, shapes, multis, with_mesh=True):
    """every handle of one texture list; multis: (ranks, from_triangles) pairs"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib, diag = rrt.load(), rrt.load_diag()
    tris, mats, texs, cam = P.panel(shapes)
    tris = tris[np.argsort(tris["material_id"], kind="stable")]                 # a mesh part has one material: its expansion is this order
    host = rrt.Scene.from_arrays(tris, mats, texs)                              # tree built on the host
    host.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    camera = host.camera.uniform
    w, h, spp, depth = FRAME
    ref, ref_rgba, rst = orc.render(host.tris, host.bvh_nodes, host.materials_array(), host.textures, camera, w, h, spp, depth)
    assert rst["hits"] > 0 and (rst["texel_fetches"] > 0) == (len(shapes) > 0)
    pool = np.concatenate([np.ascontiguousarray(t).view(np.uint32).reshape(-1) for t in host.textures]) if shapes else np.zeros(0, np.uint32)
    tables = _expected_tables(host.materials_array(), host.textures)
    dev = rrt.Scene.from_arrays(tris, mats, texs, build_bvh=False)               # tree built on the device, from the same triangle order
    mesh, perm = mesh_model.mesh_from_triangles(tris)
    assert np.array_equal(perm, np.arange(len(tris)))
    msh = rrt.Scene.from_mesh(materials=mats, textures=texs, **mesh)

    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    args = (pool, tables, camera, ref, ref_rgba)
    try:
        _check_handle(rrt, diag, lib, host.upload(0), "mipt_scene_create", *args)
        _check_handle(rrt, diag, lib, dev.upload_from_triangles(0), "mipt_scene_create_from_triangles", *args)
        if with_mesh:
            _check_handle(rrt, diag, lib, msh.upload_from_mesh(0), "mipt_scene_create_from_mesh", *args)
    finally:
        host.release(); dev.release(); msh.release()
    for ranks, from_triangles in multis:
        d = (dev if from_triangles else host).desc()
        ids, hm = (C.c_int * ranks)(*([0] * ranks)), C.c_void_p()
        create = mt.mipt_multi_create_from_triangles if from_triangles else mt.mipt_multi_create
        assert create(C.byref(d), ids, ranks, C.byref(hm)) == 0, (ranks, from_triangles, mt.mipt_last_error())
        try:
            assert mt.mipt_multi_device_count(hm) == ranks
            for r in range(ranks):
                hs = mt.mipt_multi_scene(hm, r)
                assert hs
                _check_handle(rrt, diag, mt, C.c_void_p(hs), f"rank {r} of {ranks}, from_triangles={from_triangles}", *args)
        finally:
            mt.mipt_multi_destroy(hm)
    torch.cuda.synchronize()
    lost = free0 - torch.cuda.mem_get_info(0)[0]
    bound = min(MEMORY_SLACK, pool.nbytes) if pool.nbytes >= (8 << 20) else MEMORY_SLACK
    print(f"{len(shapes)} textures, pool {pool.nbytes / 2**20:.1f} MiB: {lost / 2**20:.2f} MiB less free device memory than before (bound {bound / 2**20:.1f})")
    assert lost < bound, f"{lost / 2**20:.1f} MiB less free device memory after every handle was destroyed (bound {bound / 2**20:.1f} MiB)"


@pytest.fixture(scope="module")
def warm(rrt, orc, mt):
    """every kind of call once, so that what a process pays once (streams, kernels, the libraries' device state) is paid before a
    test measures free memory"""
    try:
        _run_list(rrt, orc, mt, LISTS["2x2"], [(2, False), (2, True)])
    except AssertionError as e:
        if "free device memory" not in str(e):
            raise
    return True


@pytest.mark.parametrize("name", [k for k in LISTS if k not in ("large", "ring")])
def test_pool_and_tables_on_every_handle(rrt, orc, mt, warm, name):
    _run_list(rrt, orc, mt, LISTS[name], [(2, False), (3, False), (2, True), (3, True)])


def test_pool_with_a_9_mb_texture_and_one_behind_it(rrt, orc, mt, warm):
    """1500 x 1500 texels = 9 MB, below the uploader's ring threshold: one plain copy, and the 1x1 lands 9 000 000 bytes into the pool.
    Single-GPU creates and one 2-rank replica set."""
    _run_list(rrt, orc, mt, LISTS["large"], [(2, False)], with_mesh=False)


def test_pool_with_a_texture_across_ring_chunks(rrt, orc, mt, warm):
    """2100 x 2100 texels = 17 640 000 bytes, above the threshold of two 8 MiB chunks: the texture crosses two chunk boundaries of the
    pinned ring and ends in a ragged third chunk; the 1x1 behind it goes through the ring too.  Any chunk placed or sized wrongly
    shows in the pool's read-back, which names the first differing texel."""
    _run_list(rrt, orc, mt, LISTS["ring"], [(2, False)], with_mesh=False)
