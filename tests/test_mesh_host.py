"""CPU: the mesh expansion rule on the host (mipt_mesh_expand) against its numpy float32 model (tests/tools/mesh_model.py), the
geometry the rule promises against float64, and the argument checks of the mesh entry points, which run before any device call."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mesh_model  # noqa: E402

MESH = ("mipt_mesh_expand", "mipt_scene_create_from_mesh", "mipt_scene_set_transforms", "mipt_scene_update_mesh_device", "mipt_scene_mesh_info")
FAMILIES = ["cornell", "helmet", "atrium", "dragon", "soup1", "soup17", "soup300d", "soup9000d"]


def _case(name):
    from test_gpu_scene_update import _case as case
    return case(name)


def _desc(mesh, transforms=None):
    from rust_ray_tracing_amd import _lib as L

    def pn(a):
        return (None, 0) if a is None else (L.ptr(a), len(a))

    d = L.MiptMeshDesc()
    d.positions, d.n_positions = pn(mesh["positions"])
    d.normals, d.n_normals = pn(mesh["normals"])
    d.tex_coords, d.n_tex_coords = pn(mesh["tex_coords"])
    idx = mesh["indices"]
    d.indices, d.n_indices = L.ptr(idx), idx.size
    d.normal_indices = pn(mesh.get("normal_indices"))[0]
    d.tex_coord_indices = pn(mesh.get("tex_coord_indices"))[0]
    d.parts, d.n_parts = pn(mesh["parts"])
    t = None if transforms is None else np.ascontiguousarray(transforms, dtype=np.float32)
    d.transforms = None if t is None else L.ptr(t)
    d._keep = (mesh, t)
    return d


def _expand(rrt, mesh, transforms=None):
    from rust_ray_tracing_amd import _lib as L
    d = _desc(mesh, transforms)
    out = np.zeros(d.n_indices // 3, dtype=L.TRIANGLE)
    n = C.c_uint32()
    rc = rrt.load().mipt_mesh_expand(C.byref(d), L.ptr(out), len(out), C.byref(n))
    assert rc == 0, rrt.load().mipt_last_error()
    assert n.value == len(out)
    return out


def _model(mesh, transforms=None):
    return mesh_model.expand(mesh["positions"], mesh["normals"], mesh["tex_coords"], mesh["indices"], mesh["parts"],
                             mesh.get("normal_indices"), mesh.get("tex_coord_indices"), transforms)


def _same_bytes(a, b, what, nan_is_nan=False):
    """nan_is_nan: a NaN the arithmetic PRODUCES has no defined sign or payload (IEEE 754 leaves both to the implementation): such
    words only have to be NaN on both sides.  Only the crafted-vertex test feeds NaN / infinity into a transform."""
    a, b = np.ascontiguousarray(a).view(np.uint32).reshape(-1, 28).copy(), np.ascontiguousarray(b).view(np.uint32).reshape(-1, 28).copy()
    assert a.shape == b.shape, what
    if nan_is_nan:
        for w in (a, b):
            w[:, :24][np.isnan(w[:, :24].view(np.float32))] = 0x7FC00000
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)} words differ, first: triangle {bad[0][0]} word {bad[0][1]}: {a[tuple(bad[0])]:#x} != {b[tuple(bad[0])]:#x}")


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _mat4(lin, trans=(0.0, 0.0, 0.0)):
    """Mat4f data[col][row] from a 3x3 (row-major maths convention: p' = lin @ p) and a translation"""
    m = np.zeros((4, 4), dtype=np.float32)
    m[:3, :3] = np.asarray(lin, dtype=np.float64).T
    m[3, :3] = trans
    m[3, 3] = 1.0
    return m.reshape(16)


def test_mesh_symbols_declared_exported_and_bound(rrt):
    from rust_ray_tracing_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mipt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mipt_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = rrt.load()
    for s in MESH:
        assert s in declared and s in exported and s in L.EXPORTS, s
        assert getattr(lib, s).restype is C.c_int and getattr(lib, s).argtypes is not None, s
    assert lib.mipt_abi_version() == 4
    assert C.sizeof(L.MiptMeshDesc) == 104 and L.MESH_PART.itemsize == 16 and C.sizeof(L.MiptMeshInfo) == 56
    assert C.sizeof(L.MiptSceneDesc) == 64 and C.sizeof(L.MiptUpdateInfo) == 48         # existing structs keep their sizes


def test_dedup_is_np_unique_by_bit_pattern():
    rng = np.random.default_rng(3)
    rows = rng.integers(0, 4, (200001, 3)).astype(np.float32)
    rows[::7, 1] = -0.0
    rows[5::11, 2] = np.nan
    rows.view(np.uint32)[9::13, 0] = 0x7FC00001                   # a second NaN payload
    u, inv = mesh_model._dedup(rows)                              # the key-sort path
    u2, inv2 = np.unique(rows.view(np.uint32), axis=0, return_inverse=True)
    assert np.array_equal(u.view(np.uint32), u2) and np.array_equal(inv, inv2.reshape(-1))
    assert np.array_equal(u.view(np.uint32)[inv], rows.view(np.uint32))
    assert len(np.unique(u.view(np.uint32)[:, 1])) > len(np.unique(u[:, 1][~np.isnan(u[:, 1])]))   # -0.0 and 0.0 both kept


@pytest.mark.parametrize("name", FAMILIES)
def test_round_trip(rrt, name):
    """(1) expand(mesh_from_triangles(tris)) == tris[perm], separate and shared index streams, with empty parts mixed in"""
    tris = _case(name)[0]
    for shared in (False, True):
        for min_parts, empty in ((1, 0), (7, 3)):
            mesh, perm = mesh_model.mesh_from_triangles(tris, min_parts, shared=shared, empty_parts=empty)
            parts = mesh["parts"]
            assert len(parts) >= min(min_parts, len(tris)) + empty and int(parts["n_tris"].sum()) == len(tris)
            assert (parts["n_tris"] == 0).sum() >= empty
            got = _expand(rrt, mesh)
            _same_bytes(got, tris[perm], f"{name} shared={shared} parts={len(parts)}")
            _same_bytes(_model(mesh), tris[perm], f"{name}: the numpy model")
    if name == "dragon":
        assert len(mesh_model.mesh_from_triangles(tris)[0]["positions"]) < len(tris)     # vertex reuse: the point of an indexed mesh


def _transform_sets(rng, n_parts):
    sets = {}
    sets["identity"] = np.stack([_mat4(np.eye(3)) for _ in range(n_parts)])
    sets["rigid"] = np.stack([_mat4(_rotation(rng), rng.uniform(-3, 3, 3)) for _ in range(n_parts)])
    sets["scale"] = np.stack([_mat4(np.diag(rng.uniform(0.25, 4.0, 3)) @ _rotation(rng), rng.uniform(-1, 1, 3)) for _ in range(n_parts)])
    sets["mirror"] = np.stack([_mat4(_rotation(rng) @ np.diag([1.0, -1.0, 1.0]), rng.uniform(-1, 1, 3)) for _ in range(n_parts)])
    sing = np.stack([_mat4(_rotation(rng) @ np.diag([1.0, 0.0, 2.0])) for _ in range(n_parts)])
    sing[0] = 0.0                                                  # the zero matrix: every cofactor is zero, n' = c = 0
    sets["singular"] = sing
    junk = rng.normal(0, 2, (n_parts, 16)).astype(np.float32)     # row 3 is ignored whatever it holds
    sets["general"] = junk
    return sets


@pytest.mark.parametrize("name", ["cornell", "helmet", "atrium", "soup300d"])
def test_transforms_match_the_numpy_model(rrt, name):
    """(2) mipt_mesh_expand with transforms == the model, bit for bit"""
    tris = _case(name)[0]
    rng = np.random.default_rng(11)
    for shared in (False, True):
        mesh, _ = mesh_model.mesh_from_triangles(tris, 9, shared=shared, empty_parts=2)
        # zero normals, out-of-range normal / tex indices and UINT32_MAX
        mesh["normals"] = mesh["normals"].copy()
        mesh["normals"][:: max(1, len(mesh["normals"]) // 5)] = 0.0
        if not shared:
            mesh["normal_indices"] = mesh["normal_indices"].copy()
            mesh["tex_coord_indices"] = mesh["tex_coord_indices"].copy()
            mesh["normal_indices"][1::17] = len(mesh["normals"])
            mesh["normal_indices"][2::19] = 0xFFFFFFFF
            mesh["tex_coord_indices"][3::23] = 0xFFFFFFFF
            mesh["tex_coord_indices"][4::29] = len(mesh["tex_coords"]) + 5
        for label, xf in _transform_sets(rng, len(mesh["parts"])).items():
            _same_bytes(_expand(rrt, mesh, xf), _model(mesh, xf), f"{name} shared={shared} {label}")
        if not shared:
            got = _expand(rrt, mesh)
            v = got["vertices"].reshape(-1)
            assert np.all(v["normal"][1::17] == 0.0) and np.all(v["tex_coord_x"][3::23] == 0.0)
    # NULL arrays: every index is out of range
    bare = dict(mesh, normals=None, tex_coords=None)
    got = _expand(rrt, bare, _transform_sets(rng, len(mesh["parts"]))["rigid"])
    assert not got["vertices"]["normal"].any() and not got["vertices"]["tex_coord_x"].any() and not got["vertices"]["tex_coord_y"].any()


def test_identity_matrix_is_not_no_transform(rrt):
    """transforms = NULL copies bits; an identity-valued matrix does arithmetic: -0.0 becomes +0.0, a NaN or an infinity spreads"""
    from rust_ray_tracing_amd import _lib as L
    pos = np.array([[-0.0, 1.0, 2.0], [3.0, -0.0, 4.0], [np.nan, 5.0, np.inf]], dtype=np.float32)
    pos.view(np.uint32)[2, 0] = 0x7FC12345
    nrm = np.array([[-0.0, 0.0, 1.0]], dtype=np.float32)
    mesh = dict(positions=pos, normals=nrm, tex_coords=np.array([[-0.0, 0.5]], dtype=np.float32), indices=np.array([0, 1, 2], dtype=np.uint32),
                normal_indices=np.zeros(3, dtype=np.uint32), tex_coord_indices=np.zeros(3, dtype=np.uint32),
                parts=np.array([(0, 1, 4, 0)], dtype=L.MESH_PART))
    plain = _expand(rrt, mesh)
    assert np.array_equal(plain["vertices"]["position"][0].view(np.uint32), pos.view(np.uint32))
    assert plain["vertices"]["normal"][0, 0].view(np.uint32)[0] == 0x80000000 and plain["material_id"][0] == 4
    ident = _expand(rrt, mesh, _mat4(np.eye(3)).reshape(1, 16))
    _same_bytes(ident, _model(mesh, _mat4(np.eye(3)).reshape(1, 16)), "identity", nan_is_nan=True)
    p = ident["vertices"]["position"][0].view(np.uint32)
    assert p[0, 0] == 0x00000000 and plain["vertices"]["position"][0].view(np.uint32)[0, 0] == 0x80000000
    assert p[1, 1] == 0x00000000 and ident["vertices"]["position"][0][1, 2] == 4.0
    assert np.isnan(ident["vertices"]["position"][0][2]).all()                       # 0 * NaN, 0 * inf: the whole vertex is NaN now
    assert ident["vertices"]["normal"][0, 0].view(np.uint32)[0] == 0x00000000        # the normal's -0.0 as well
    assert ident["vertices"]["tex_coord_x"][0, 0].view(np.uint32) == 0x80000000      # tex coords are copied in both cases


def _sanity_mesh(rrt):
    """the synth dragon with every normal rescaled to a length in [0.5, 2]"""
    tris = _case("dragon")[0].copy()
    rng = np.random.default_rng(21)
    n = tris["vertices"]["normal"].astype(np.float64)
    ln = np.linalg.norm(n, axis=-1, keepdims=True)
    n = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), np.array([0.0, 1.0, 0.0])) * rng.uniform(0.5, 2.0, ln.shape)
    tris["vertices"]["normal"] = n.astype(np.float32)
    return tris


def test_normal_length_is_kept(rrt):
    """(3a) |n'| == |n| to 2^-21 relative for invertible matrices with entries of magnitude <= 8: two sum-of-squares lengths, one
    division and one multiplication are a handful of half-ulp (2^-24) roundings, none with cancellation"""
    tris = _sanity_mesh(rrt)
    mesh, perm = mesh_model.mesh_from_triangles(tris, 12)
    rng = np.random.default_rng(22)
    mats = []
    while len(mats) < len(mesh["parts"]):
        a = rng.uniform(-8, 8, (3, 3))
        if abs(np.linalg.det(a)) > 1.0:
            mats.append(_mat4(a, rng.uniform(-8, 8, 3)))
    got = _expand(rrt, mesh, np.stack(mats))
    l0 = np.linalg.norm(tris[perm]["vertices"]["normal"].astype(np.float64), axis=-1)
    l1 = np.linalg.norm(got["vertices"]["normal"].astype(np.float64), axis=-1)
    assert l0.min() >= 0.49 and l0.max() <= 2.01
    rel = np.abs(l1 - l0) / l0
    print(f"normal length: max relative error {rel.max():.3e} (bound {2.0 ** -21:.3e})")
    assert rel.max() <= 2.0 ** -21


def test_mirror_keeps_the_normal_on_its_side(rrt):
    """(3b) an orthogonal mirror (a reflection times a rotation; the cofactor matrix is -M in real arithmetic): the transformed
    normal stays on the side of the moved triangle's geometric normal cross(e1', e2') that it had before"""
    tris = _sanity_mesh(rrt)
    mesh, perm = mesh_model.mesh_from_triangles(tris, 12)
    rng = np.random.default_rng(23)
    mats = np.stack([_mat4(_rotation(rng) @ np.diag([1.0, 1.0, -1.0]) @ _rotation(rng), rng.uniform(-4, 4, 3)) for _ in mesh["parts"]])
    for m in mats:
        assert np.linalg.det(m.reshape(4, 4)[:3, :3].astype(np.float64)) < 0
    got = _expand(rrt, mesh, mats)

    def side(t):
        p = t["vertices"]["position"].astype(np.float64)
        g = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        n = t["vertices"]["normal"].astype(np.float64)
        d = np.einsum("tcj,tj->tc", n, g)
        return d, np.linalg.norm(n, axis=-1) * np.linalg.norm(g, axis=-1)[:, None]

    d0, scale0 = side(tris[perm])
    d1, _ = side(got)
    keep = np.abs(d0) > 1e-3 * scale0
    dropped = 1.0 - keep.mean()
    print(f"mirror: {dropped * 100:.3f} % of {keep.size} corners within 0.06 degrees of the surface")
    assert dropped < 0.01
    assert np.array_equal(np.sign(d1[keep]), np.sign(d0[keep]))


def _tiny_mesh(L):
    return dict(positions=np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32), normals=None, tex_coords=None,
                indices=np.array([0, 1, 2, 1, 2, 3], dtype=np.uint32), parts=np.array([(0, 1, 0, 0), (1, 1, 0, 0)], dtype=L.MESH_PART))


def test_mesh_expand_argument_errors(rrt):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    out = np.zeros(2, dtype=L.TRIANGLE)
    n = C.c_uint32()

    def call(mesh, cap=2, xf=None):
        d = _desc(mesh, xf)
        return lib.mipt_mesh_expand(C.byref(d), L.ptr(out), cap, C.byref(n)), lib.mipt_last_error().decode()

    assert lib.mipt_mesh_expand(None, L.ptr(out), 2, None) == L.ERR_INVALID_ARG
    base = _tiny_mesh(L)
    assert call(base)[0] == 0 and n.value == 2
    rc, msg = call(base, cap=1)
    assert rc == L.ERR_INVALID_ARG and "room for 1" in msg and n.value == 2
    for entry in (0, 3, 5):                                         # a position index out of range: first, middle, last entry
        m = dict(base, indices=base["indices"].copy())
        m["indices"][entry] = 4
        rc, msg = call(m)
        assert rc == L.ERR_INVALID_ARG and f"index entry {entry} " in msg and "position index 4" in msg, msg
        with pytest.raises(ValueError, match=f"entry {entry}$"):
            _model(m)
    m = dict(base, indices=np.array([0, 0xFFFFFFFF, 2, 1, 9, 3], dtype=np.uint32))
    assert "index entry 1 " in call(m)[1]                           # the first one found
    assert call(dict(base, positions=None))[0] == L.ERR_INVALID_ARG
    rc, msg = call(dict(base, indices=base["indices"][:5].copy()))
    assert rc == L.ERR_INVALID_ARG and "multiple of 3" in msg
    rc, msg = call(dict(base, indices=np.zeros(0, dtype=np.uint32), parts=np.zeros(1, dtype=L.MESH_PART)))
    assert rc == L.ERR_INVALID_ARG and "no triangles" in msg


PART_ERRORS = [
    ("gap", [(0, 1, 0, 0), (2, 0, 0, 0)], "tile"),
    ("overlap", [(0, 2, 0, 0), (1, 1, 0, 0)], "tile"),
    ("short", [(0, 1, 0, 0)], "tile"),
    ("long", [(0, 1, 0, 0), (1, 2, 0, 0)], "tile"),
    ("out of order", [(1, 1, 0, 0), (0, 1, 0, 0)], "tile"),
    ("reserved", [(0, 1, 0, 0), (1, 1, 0, 9)], "reserved"),
]


def test_create_from_mesh_argument_errors_without_a_device(rrt):
    """(4) refused with a message before any device call; *out stays NULL"""
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    mats = np.array([rrt.material_default(), rrt.material_default()])
    sd = L.MiptSceneDesc(None, 0, None, 0, L.ptr(mats), 2, None, 0)
    base = _tiny_mesh(L)

    def call(mesh, scene_desc=sd):
        d = _desc(mesh)
        h = C.c_void_p(0x1234)
        rc = lib.mipt_scene_create_from_mesh(C.byref(scene_desc), C.byref(d), 0, C.byref(h))
        assert h.value is None
        return rc, lib.mipt_last_error().decode()

    h = C.c_void_p()
    d = _desc(base)
    assert lib.mipt_scene_create_from_mesh(None, C.byref(d), 0, C.byref(h)) == L.ERR_INVALID_ARG
    assert lib.mipt_scene_create_from_mesh(C.byref(sd), None, 0, C.byref(h)) == L.ERR_INVALID_ARG
    assert lib.mipt_scene_create_from_mesh(C.byref(sd), C.byref(d), 0, None) == L.ERR_INVALID_ARG
    assert "null argument" in lib.mipt_last_error().decode()
    for key in ("positions", "parts"):
        rc, msg = call(dict(base, **{key: None}))
        assert rc == L.ERR_INVALID_ARG and "null" in msg, key
    dn = _desc(base)
    dn.indices = None
    assert lib.mipt_scene_create_from_mesh(C.byref(sd), C.byref(dn), 0, C.byref(h)) == L.ERR_INVALID_ARG
    rc, msg = call(dict(base, indices=base["indices"][:4].copy()))
    assert rc == L.ERR_INVALID_ARG and "multiple of 3" in msg
    rc, msg = call(dict(base, indices=np.zeros(0, dtype=np.uint32), parts=np.zeros(1, dtype=L.MESH_PART)))
    assert rc == L.ERR_INVALID_ARG and "no triangles" in msg
    for name, parts, word in PART_ERRORS:
        rc, msg = call(dict(base, parts=np.array(parts, dtype=L.MESH_PART)))
        assert rc == L.ERR_INVALID_ARG and word in msg, (name, msg)
    rc, msg = call(dict(base, parts=np.array([(0, 1, 0, 0), (1, 1, 2, 0)], dtype=L.MESH_PART)))
    assert rc == L.ERR_INVALID_ARG and "material_id 2 >= n_materials 2" in msg
    big = dict(base, indices=np.zeros(3 * ((1 << 25) + 1), dtype=np.uint32), parts=np.array([(0, (1 << 25) + 1, 0, 0)], dtype=L.MESH_PART))
    rc, msg = call(big)
    assert rc == L.ERR_SCENE_LIMIT and "2^25" in msg
    bad_tex = mats.copy()
    bad_tex["base_color_tex_id"][1] = 3                             # a texture the scene does not have
    rc, msg = call(base, L.MiptSceneDesc(None, 0, None, 0, L.ptr(bad_tex), 2, None, 0))
    assert rc == L.ERR_INVALID_ARG, msg


@pytest.mark.parametrize("which", ["mipt_scene_set_transforms", "mipt_scene_update_mesh_device"])
def test_update_argument_errors_without_a_device(rrt, which):
    """(4) checks that need no look at the scene run first: the handle below is opaque and never dereferenced"""
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    xf = np.zeros((2, 16), dtype=np.float32)
    handle = C.c_void_p(0x1000)

    def call(scene, mode):
        if which == "mipt_scene_set_transforms":
            return lib.mipt_scene_set_transforms(scene, L.ptr(xf), 2, mode, None)
        return lib.mipt_scene_update_mesh_device(scene, None, None, L.ptr(xf), mode, None, None)

    assert call(None, 0) == L.ERR_INVALID_ARG and "null scene" in lib.mipt_last_error().decode()
    for mode in (2, 7, 0xFFFFFFFF):
        assert call(handle, mode) == L.ERR_INVALID_ARG
        assert "neither MIPT_UPDATE_REFIT nor MIPT_UPDATE_REBUILD" in lib.mipt_last_error().decode()
    info = L.MiptMeshInfo()
    assert lib.mipt_scene_mesh_info(None, C.byref(info)) == L.ERR_INVALID_ARG
    assert lib.mipt_scene_mesh_info(handle, None) == L.ERR_INVALID_ARG


def test_well_formed_create_fails_loudly_without_a_device(rrt):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device path is exercised on the CPU-only box")
    from rust_ray_tracing_amd import _lib as L
    tris, mats, texs, _ = _case("cornell")
    mesh, _ = mesh_model.mesh_from_triangles(tris, 4)
    sc = rrt.Scene.from_mesh(materials=mats, textures=texs, **mesh)
    d, md = sc.desc(), sc.mesh_desc()
    h = C.c_void_p(0x1234)
    assert rrt.load().mipt_scene_create_from_mesh(C.byref(d), C.byref(md), 0, C.byref(h)) == L.ERR_HIP
    assert h.value is None
    with pytest.raises(rrt.MiptError):
        sc.upload_from_mesh(0)


def test_host_mirror_expand_mesh(rrt):
    tris, mats, texs, _ = _case("helmet")
    mesh, perm = mesh_model.mesh_from_triangles(tris, 5)
    sc = rrt.Scene.from_mesh(materials=mats, textures=texs, **mesh)
    _same_bytes(sc.expand_mesh(), tris[perm], "Scene.expand_mesh")
    rng = np.random.default_rng(5)
    xf = _transform_sets(rng, len(mesh["parts"]))["rigid"]
    sc2 = rrt.Scene.from_mesh(materials=mats, textures=texs, transforms=xf.reshape(-1, 4, 4), **mesh)
    _same_bytes(sc2.expand_mesh(), _model(mesh, xf), "Scene.expand_mesh with transforms")
    with pytest.raises(ValueError):
        rrt.Scene.from_mesh(materials=mats, transforms=xf[:2], **mesh)
    with pytest.raises(RuntimeError):
        sc.set_transforms(xf)                                       # not resident
