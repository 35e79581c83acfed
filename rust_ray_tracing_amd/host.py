"""Host-side mirror of the reference's Renderer / Scene API for the path-tracing hot path.

Names, argument meaning and error behaviour follow the reference
(src/renderer.rs:8-117, src/renderer/backend.rs:6-10, src/scene.rs:12-195):

* ``Renderer.new(options)`` validates like ``Renderer::new`` and returns ``None`` (after logging
  the reference's message) instead of raising;
* ``Renderer.render(scene)`` dispatches on ``options.backend``; the new arm is
  ``RendererBackend.MI355X`` which goes through the C ABI of libmipt.so;
* ``Scene.load(path)`` / ``Scene.set_camera(camera)`` / ``Camera.update_view()`` as in scene.rs.

Everything numerical happens behind the C ABI (include/mipt.h); this module only marshals.
"""
from __future__ import annotations

import ctypes as C
import enum
import math
import os
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib as L


def log_error(msg: str) -> None:  # log.rs:22-29
    print(f"[ERROR] {msg}", file=sys.stderr)


def log_info(msg: str) -> None:  # log.rs:2-9
    if os.environ.get("MIPT_LOG"):
        print(f"[INFO] {msg}", file=sys.stderr)


class RendererBackend(enum.Enum):  # renderer/backend.rs:6-10 + the new arm
    GPU = "GPU"        # the reference's wgpu backend: not part of this build
    CPU = "CPU"        # the reference's rayon backend: not part of this build (see oracle/ for tests)
    MI355X = "MI355X"  # this build: gfx950 megakernel behind the C ABI


@dataclass
class RendererOptions:  # renderer.rs:96-116
    samples: int = 1
    max_ray_depth: int = 6
    output_image_dimensions: Tuple[int, int] = (1920, 1080)
    output_image_path: Optional[str] = None
    backend: RendererBackend = RendererBackend.MI355X
    is_realtime: bool = False
    # MI355X-path extensions (MiptOptions)
    seed_mode: int = L.SEED_PIXEL_STREAM
    # the CPU backend's own un-culled traversal (ray.rs:69-81): the reference by construction, and what the parity tests compare
    # counter for counter with the oracle.  Production use: TRAVERSAL_CULLED with CULL_MARGIN_SAFE -- same frame, 1.7x faster
    # (the C++ mirror include/mipt_host.hpp and the Rust binding default to it).
    traversal: int = L.TRAVERSAL_REFERENCE
    cull_margin: float = L.CULL_MARGIN_SAFE
    shading: int = L.SHADING_CPU          # SHADING_WGPU: the wgpu shader's material model (rt_compute.wgsl)
    device_id: int = 0


@dataclass
class Camera:  # scene.rs:169-195
    pitch: float = 0.0
    yaw: float = 0.0
    position: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    uniform: np.ndarray = field(default_factory=lambda: np.zeros((), dtype=L.CAMERA))

    def update_view(self) -> None:
        pos = (C.c_float * 3)(*[float(x) for x in self.position])
        out = np.zeros((), dtype=L.CAMERA)
        L.check(L.load().mipt_camera_from_pose(C.byref(pos), C.c_float(self.pitch), C.c_float(self.yaw), L.ptr(out)),
                "mipt_camera_from_pose")
        self.uniform = out


def material_default() -> np.ndarray:  # scene.rs:148-167
    m = np.zeros((), dtype=L.MATERIAL)
    L.load().mipt_material_default(L.ptr(m))
    return m


@dataclass
class Texture:  # texture.rs:3-10
    width: int
    height: int
    hash: int
    pixel_data: np.ndarray          # (height, width, 4) uint8, rows as Texture::load stores them (flipv applied)

    @staticmethod
    def load(path: str) -> Optional["Texture"]:  # texture.rs:13-31 (None + log line when the file is missing / undecodable)
        lib = L.load()
        img = C.c_void_p()
        desc = L.MiptTexture()
        h = C.c_uint32()
        if lib.mipt_texture_load(os.fsencode(path), C.byref(img), C.byref(desc), C.byref(h)) != 0:
            log_error(lib.mipt_last_error().decode())
            return None
        try:
            px = np.ctypeslib.as_array(C.cast(desc.rgba8, C.POINTER(C.c_uint8)), (desc.height, desc.width, 4)).copy()
            return Texture(int(desc.width), int(desc.height), int(h.value), px)
        finally:
            lib.mipt_texture_free(img)


# -- what the wrappers of Scene and Renderer share -------------------------------------------------
def _is_torch(a) -> bool:
    return type(a).__module__.split(".")[0] == "torch"


def _stream_arg(stream, device):
    """the raw hipStream_t of ``stream``: a torch stream, a raw handle or None = torch's current stream on ``device``"""
    if stream is None:
        import torch
        return torch.cuda.current_stream(device).cuda_stream
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else stream


def _camera_table(cams, who=None) -> np.ndarray:
    """the contiguous CAMERA table of a list of Camera (or CAMERA records); ``who``: the caller an empty list is refused for"""
    if who and not cams:
        raise ValueError(f"{who}: no cameras")
    return np.ascontiguousarray(np.stack([np.asarray(c.uniform if isinstance(c, Camera) else c, dtype=L.CAMERA).reshape(()) for c in cams]))


def _views(lead):
    """(V, H, W) of a plane's leading shape [V,H,W] or [H,W]"""
    return ((1,) + lead) if len(lead) == 2 else lead


def _check_planes(anchor_name, anchor, family, table, flat=False, required=(), missing=""):
    """The planes of one image-space call: all numpy arrays or all tensors like ``anchor``, the plane whose kind and device the
    others follow.  ``table``: (name, plane or None, expected shape, ids?) rows, the anchor's own among them -- an ids plane is
    uint32 as an array and int32 as a tensor (the same bits), any other float32.  ``flat``: a plane may have any shape of that many
    values with that last dimension ([H*W,3] for [H,W,3]).  A None plane is left out, unless its name is in ``required``: then
    ``missing`` says why not.  -> (torch?, {name: contiguous array, or the tensor}); ValueError naming the plane otherwise."""
    torch_in = _is_torch(anchor)
    planes = {}
    for name, a, want, ids in table:
        if a is None:
            if name in required:
                raise ValueError(f"{name}: {missing}")
            continue
        if _is_torch(a) != torch_in:
            raise ValueError(f"{name}: {family} must all be numpy arrays or all torch tensors")
        if torch_in:
            import torch
            if a.dtype != (torch.int32 if ids else torch.float32) or not a.is_cuda or a.device != anchor.device:
                raise ValueError(f"{name}: expected a {'int32' if ids else 'float32'} tensor on {anchor_name}'s device {anchor.device}")
        else:
            a = np.asarray(a)
            if a.dtype != (np.uint32 if ids else np.float32):
                raise ValueError(f"{name}: expected uint32; got {a.dtype}" if ids else f"{name}: expected float32; got {a.dtype}")
        shape = tuple(a.shape)
        if (math.prod(shape) != math.prod(want) or shape[-1:] != want[-1:]) if flat else shape != want:
            raise ValueError(f"{name}: expected shape {want}; got {shape}")
        if torch_in and not a.is_contiguous():              # a copy here would run on torch's current stream, not on `stream`
            raise ValueError(f"{name}: expected a contiguous tensor")
        planes[name] = a if torch_in else np.ascontiguousarray(a)
    return torch_in, planes


def _fill(bufs, **planes) -> list:
    """the addresses of ``planes`` (arrays or tensors; None = left NULL) into the fields of a ...Buffers struct of those names;
    -> the planes given, which is what the call then touches"""
    given = [(name, a) for name, a in planes.items() if a is not None]
    for name, a in given:
        setattr(bufs, name, a.data_ptr() if _is_torch(a) else a.ctypes.data)
    return [a for _, a in given]


def _stream_ordered(dev, stream, tensors, need=None):
    """What a device entry that runs stream-ordered needs from torch: -> (the raw stream, the workspace).  ``tensors``: every tensor
    the entry reads or writes (None entries are skipped); ``need``: the bytes of its workspace, a torch tensor of 16-byte rows -- an
    impossible size is the library's to refuse --, None = the entry has none."""
    import torch
    workspace = None if need is None else torch.empty((max(int(need), 16) // 16, 4), dtype=torch.float32, device=dev)
    raw = _stream_arg(stream, dev)
    # the passes are queued, not finished: tell torch's allocator that `stream` still uses these blocks
    s = torch.cuda.ExternalStream(raw, device=dev) if raw else torch.cuda.default_stream(dev)
    for t in list(tensors) + [workspace]:
        if t is not None:
            t.record_stream(s)
    return raw, workspace


class Scene:  # scene.rs:12-19
    """tris / materials / textures / bvh / camera.  ``materials`` is name -> Material in id order."""

    def __init__(self):
        self.tris: np.ndarray = np.zeros(0, dtype=L.TRIANGLE)
        self.materials: Dict[str, np.ndarray] = {}
        self.textures: List[np.ndarray] = []      # each (h, w, 4) uint8, rows as Texture::load stores them
        self.bvh_nodes: np.ndarray = np.zeros(0, dtype=L.NODE)
        self.camera = Camera()
        self._handle: Optional[C.c_void_p] = None
        self._handle_device = -1
        self._tri_order: Optional[np.ndarray] = None   # fetch_bvh: tris = (the device's input order)[_tri_order]
        self.mesh: Optional[dict] = None               # from_mesh: the indexed arrays behind MiptMeshDesc
        self._tracks_motion = False                    # track_motion: the resident mesh keeps its previous generation

    # -- construction ------------------------------------------------------------------------
    @staticmethod
    def load(path: str, build_bvh: bool = True) -> Optional["Scene"]:  # scene.rs:22-36
        """``build_bvh=False``: OBJ::load + From<OBJ> without the BVH::build at scene.rs:80 (mipt_obj_load_triangles) -- triangles in file
        order for ``upload_from_triangles``, which builds the tree on the GPU."""
        lib = L.load()
        obj = C.c_void_p()
        rc = (lib.mipt_obj_load if build_bvh else lib.mipt_obj_load_triangles)(os.fsencode(path), C.byref(obj))
        if rc != 0:
            log_error(lib.mipt_last_error().decode())
            return None
        try:
            desc = L.MiptSceneDesc()
            names = C.POINTER(C.c_char_p)()
            L.check(lib.mipt_obj_get(obj, C.byref(desc), C.byref(names)), "mipt_obj_get")
            sc = Scene()
            sc.tris = np.ctypeslib.as_array(C.cast(desc.tris, C.POINTER(C.c_uint8)), (desc.n_tris * 112,)).copy().view(L.TRIANGLE)
            if desc.n_nodes:
                sc.bvh_nodes = np.ctypeslib.as_array(C.cast(desc.nodes, C.POINTER(C.c_uint8)), (desc.n_nodes * 32,)).copy().view(L.NODE)
            mats = np.ctypeslib.as_array(C.cast(desc.materials, C.POINTER(C.c_uint8)), (desc.n_materials * 80,)).copy().view(L.MATERIAL)
            for i in range(desc.n_materials):
                sc.materials[names[i].decode()] = mats[i].copy()
            for i in range(desc.n_textures):
                t = desc.textures[i]
                px = np.ctypeslib.as_array(C.cast(t.rgba8, C.POINTER(C.c_uint8)), (t.height, t.width, 4)).copy()
                sc.textures.append(px)
            return sc
        finally:
            lib.mipt_obj_free(obj)

    @staticmethod
    def from_arrays(tris: np.ndarray, materials, textures=(), build_bvh: bool = True, threads: int = 0) -> "Scene":
        """impl From<OBJ> for Scene (scene.rs:44-85) for already-expanded triangles."""
        sc = Scene()
        sc.tris = np.ascontiguousarray(tris, dtype=L.TRIANGLE).copy()
        if isinstance(materials, dict):
            sc.materials = {k: np.asarray(v, dtype=L.MATERIAL).reshape(()) for k, v in materials.items()}
        else:
            sc.materials = {f"material_{i}": np.asarray(m, dtype=L.MATERIAL).reshape(()) for i, m in enumerate(materials)}
        sc.textures = [np.ascontiguousarray(t, dtype=np.uint8) for t in textures]
        if build_bvh:
            sc.build_bvh(threads)
        return sc

    def build_bvh(self, threads: int = 0) -> None:  # BVH::build, bvh.rs:13-54
        n = len(self.tris)
        nodes = np.zeros(max(2 * n, 1), dtype=L.NODE)
        count = C.c_uint32(0)
        L.check(L.load().mipt_bvh_build(L.ptr(self.tris), n, L.ptr(nodes), len(nodes), C.byref(count), threads), "mipt_bvh_build")
        self.bvh_nodes = nodes[: count.value].copy()
        self._tri_order = None
        self.release()

    def build_bvh_device(self, device_id: int = 0) -> float:
        """BVH::build on the GPU (mipt_bvh_build_device); returns the device build time in ms."""
        n = len(self.tris)
        nodes = np.zeros(max(2 * n, 1), dtype=L.NODE)
        count = C.c_uint32(0)
        ms = C.c_double(0.0)
        L.check(L.load().mipt_bvh_build_device(L.ptr(self.tris), n, L.ptr(nodes), len(nodes), C.byref(count), device_id, C.byref(ms)),
                "mipt_bvh_build_device")
        self.bvh_nodes = nodes[: count.value].copy()
        self._tri_order = None
        self.release()
        return ms.value

    def set_camera(self, camera: Camera) -> None:  # scene.rs:38-41
        self.camera = camera
        self.camera.update_view()

    # -- device residency --------------------------------------------------------------------
    def materials_array(self) -> np.ndarray:
        return np.array([m for m in self.materials.values()], dtype=L.MATERIAL) if self.materials else np.zeros(0, dtype=L.MATERIAL)

    def desc(self):
        """MiptSceneDesc over this scene's arrays (keeps the backing arrays alive on the returned object)."""
        mats = np.ascontiguousarray(self.materials_array())
        texs = (L.MiptTexture * max(len(self.textures), 1))()
        for i, t in enumerate(self.textures):
            texs[i].width, texs[i].height, texs[i].rgba8 = t.shape[1], t.shape[0], t.ctypes.data
        d = L.MiptSceneDesc(L.ptr(self.tris), len(self.tris), L.ptr(self.bvh_nodes), len(self.bvh_nodes),
                            L.ptr(mats), len(mats), texs, len(self.textures))
        d._keep = (mats, texs)
        return d

    def upload(self, device_id: int = 0) -> C.c_void_p:
        if self._handle is not None and self._handle_device == device_id:
            return self._handle
        self.release()
        self._tri_order = None
        h = C.c_void_p()
        d = self.desc()
        L.check(L.load().mipt_scene_create(C.byref(d), device_id, C.byref(h)), "mipt_scene_create")
        self._handle, self._handle_device = h, device_id
        return h

    def host_layout(self):
        """TEST INFRASTRUCTURE (libmipt_diag.so, tests/cpp/host_layout.cpp): the geometry buffers as rounds 1-3 laid them out on the
        host from this Scene's triangles and nodes -- the byte-for-byte reference of the device layout kernels both entries now use.
        Returns (geom bytes, attr bytes, dict(n_pair_records, max_leaf, root_a, root_n))."""
        diag = L.load_diag()
        d = self.desc()
        sizes, info = (C.c_uint64 * 2)(), (C.c_uint32 * 4)()
        rc = diag.mipt_diag_host_layout(C.byref(d), None, 0, None, 0, C.byref(sizes), C.byref(info))
        if rc:
            raise RuntimeError(f"mipt_diag_host_layout failed with status {rc}")
        geom, attr = np.zeros(sizes[0], dtype=np.uint8), np.zeros(sizes[1], dtype=np.uint8)
        rc = diag.mipt_diag_host_layout(C.byref(d), geom.ctypes.data, sizes[0], attr.ctypes.data, sizes[1], C.byref(sizes), C.byref(info))
        if rc:
            raise RuntimeError(f"mipt_diag_host_layout failed with status {rc}")
        return geom, attr, dict(n_pair_records=int(info[0]), max_leaf=int(info[1]), root_a=int(info[2]), root_n=int(info[3]))

    def host_layout_fingerprint(self):
        """(hash of geom, hash of attr, bytes of geom, bytes of attr) of host_layout(), comparable with mipt_diag_scene_hash / _sizes."""
        geom, attr, _ = self.host_layout()
        diag = L.load_diag()
        hg, ha = C.c_uint64(), C.c_uint64()
        assert diag.mipt_diag_hash_words(geom.ctypes.data, geom.size // 4, C.byref(hg)) == 0
        assert diag.mipt_diag_hash_words(attr.ctypes.data, attr.size // 4, C.byref(ha)) == 0
        return int(hg.value), int(ha.value), int(geom.size), int(attr.size)

    def upload_from_triangles(self, device_id: int = 0, fetch_bvh: bool = False) -> C.c_void_p:
        """BVH::build + upload in ONE call, everything after the triangle copy on the GPU (mipt_scene_create_from_triangles): the
        scene's triangles go up in their current order, the tree is built and laid out in HBM.  With ``fetch_bvh`` the Scene is
        left as BVH::build leaves the reference's (bvh.rs:13-54): ``bvh_nodes`` filled and ``tris`` reordered."""
        self.release()
        self._tri_order = None
        h = C.c_void_p()
        d = self.desc()
        lib = L.load()
        L.check(lib.mipt_scene_create_from_triangles(C.byref(d), device_id, C.byref(h)), "mipt_scene_create_from_triangles")
        self._handle, self._handle_device = h, device_id
        if fetch_bvh:
            self._fetch_bvh(h)
        return h

    # -- resident indexed meshes (include/mipt.h "resident indexed meshes") --------------------
    @staticmethod
    def from_mesh(positions, normals, tex_coords, indices, parts, materials, textures=(), normal_indices=None, tex_coord_indices=None,
                  transforms=None) -> "Scene":
        """A scene held as an indexed mesh: ``positions`` [P,3], ``normals`` [N,3] or None, ``tex_coords`` [T,2] or None, ``indices``
        [M,3] (position index per corner; ``normal_indices`` / ``tex_coord_indices``: the OBJ model's separate streams, None = shared),
        ``parts`` as MESH_PART records or (first_tri, n_tris, material_id) rows, ``transforms`` [n_parts,4,4] (Mat4f data[col][row])
        or None.  Nothing is expanded here: ``expand_mesh`` does it on the host, ``upload_from_mesh`` on the GPU."""
        sc = Scene.from_arrays(np.zeros(0, dtype=L.TRIANGLE), materials, textures, build_bvh=False)

        def f32(a, width):
            return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, width))

        def u32(a):
            return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))

        p = np.asarray(parts)
        if p.dtype != L.MESH_PART:
            rows = np.asarray(parts, dtype=np.uint32).reshape(-1, 3)
            p = np.zeros(len(rows), dtype=L.MESH_PART)
            p["first_tri"], p["n_tris"], p["material_id"] = rows[:, 0], rows[:, 1], rows[:, 2]
        sc.mesh = dict(positions=f32(positions, 3), normals=f32(normals, 3), tex_coords=f32(tex_coords, 2), indices=u32(indices),
                       normal_indices=u32(normal_indices), tex_coord_indices=u32(tex_coord_indices), parts=np.ascontiguousarray(p),
                       transforms=None)
        sc._set_mesh_transforms(transforms)
        return sc

    def _set_mesh_transforms(self, transforms) -> None:
        if transforms is None:
            self.mesh["transforms"] = None
            return
        t = np.ascontiguousarray(np.asarray(transforms, dtype=np.float32).reshape(-1, 16))
        if len(t) != len(self.mesh["parts"]):
            raise ValueError(f"{len(t)} transforms for {len(self.mesh['parts'])} parts")
        self.mesh["transforms"] = t

    def mesh_desc(self):
        """MiptMeshDesc over this scene's mesh arrays (kept alive on the returned object)."""
        if self.mesh is None:
            raise RuntimeError("scene has no mesh (Scene.from_mesh)")
        m = self.mesh

        def pn(a):
            return (None, 0) if a is None else (L.ptr(a), len(a))

        d = L.MiptMeshDesc()
        d.positions, d.n_positions = pn(m["positions"])
        d.normals, d.n_normals = pn(m["normals"])
        d.tex_coords, d.n_tex_coords = pn(m["tex_coords"])
        d.indices, d.n_indices = pn(m["indices"])
        d.normal_indices = pn(m["normal_indices"])[0]
        d.tex_coord_indices = pn(m["tex_coord_indices"])[0]
        d.parts, d.n_parts = pn(m["parts"])
        d.transforms = pn(m["transforms"])[0]
        d._keep = dict(m)
        return d

    def expand_mesh(self) -> np.ndarray:
        """The expansion rule on the host (mipt_mesh_expand): fat triangles in the mesh's own order, also left in ``self.tris``
        (the tree, if any, is dropped)."""
        d = self.mesh_desc()
        out = np.zeros(d.n_indices // 3, dtype=L.TRIANGLE)
        n = C.c_uint32(0)
        L.check(L.load().mipt_mesh_expand(C.byref(d), L.ptr(out), len(out), C.byref(n)), "mipt_mesh_expand")
        self.tris = out[: n.value]
        self.bvh_nodes = np.zeros(0, dtype=L.NODE)
        self._tri_order = None
        return self.tris

    def upload_from_mesh(self, device_id: int = 0, fetch_bvh: bool = False) -> C.c_void_p:
        """mipt_scene_create_from_mesh: the mesh arrays go up once and stay resident, the GPU expands them and builds the tree.  With
        ``fetch_bvh`` the Scene is left as ``upload_from_triangles(fetch_bvh=True)`` leaves it (host expansion + the device's tree)."""
        self.release()
        self._tri_order = None
        h = C.c_void_p()
        d, md = self.desc(), self.mesh_desc()
        L.check(L.load().mipt_scene_create_from_mesh(C.byref(d), C.byref(md), device_id, C.byref(h)), "mipt_scene_create_from_mesh")
        self._handle, self._handle_device = h, device_id
        if fetch_bvh:
            self.expand_mesh()
            self._fetch_bvh(h)
        return h

    def _mesh_mirror(self, mode: int) -> None:
        """after an update of a mesh scene whose tree is mirrored here: tris / bvh_nodes describe the device again"""
        if len(self.bvh_nodes) == 0:
            return
        order = self._tri_order
        self.expand_mesh()
        if mode == L.UPDATE_REBUILD or order is None:
            self._fetch_bvh(self._handle)
        else:
            self.tris, self._tri_order = self.tris[order], order
            self.bvh_nodes = np.zeros(2 * len(self.tris), dtype=L.NODE)
            self._fetch_nodes(self._handle)

    def set_transforms(self, transforms, mode: int = L.UPDATE_REFIT) -> dict:
        """One 4x4 matrix per part from host memory (mipt_scene_set_transforms; None = back to no transforms), then REFIT / REBUILD.
        Returns MiptUpdateInfo as a dict."""
        if self._handle is None or self.mesh is None:
            raise RuntimeError("scene is not resident as a mesh (upload_from_mesh)")
        old = self.mesh["transforms"]
        self._set_mesh_transforms(transforms)
        t = self.mesh["transforms"]
        info = L.MiptUpdateInfo()
        rc = L.load().mipt_scene_set_transforms(self._handle, None if t is None else L.ptr(t), len(self.mesh["parts"]), mode, C.byref(info))
        if rc:
            self.mesh["transforms"] = old
        L.check(rc, "mipt_scene_set_transforms")
        self._mesh_mirror(mode)
        return info.as_dict()

    def update_mesh_device(self, positions=None, normals=None, transforms=None, mode: int = L.UPDATE_REFIT, stream=None) -> dict:
        """A deforming mesh from HBM (mipt_scene_update_mesh_device): each argument is a torch tensor on the scene's device (float32,
        contiguous; [P,3], [N,3], [n_parts,4,4]), a raw device pointer (int), or None = keep what is resident.  ``stream``: a torch
        stream, a raw hipStream_t or None = torch's current stream (the null stream without torch).  The host mirror of the mesh
        follows tensors (copied back); after raw pointers it is stale.  Returns MiptUpdateInfo as a dict."""
        if self._handle is None or self.mesh is None:
            raise RuntimeError("scene is not resident as a mesh (upload_from_mesh)")
        m = self.mesh
        want = {"positions": (len(m["positions"]), 3), "normals": (0 if m["normals"] is None else len(m["normals"]), 3), "transforms": (len(m["parts"]), 16)}
        ptrs, tensors = {}, {}
        for name, a in (("positions", positions), ("normals", normals), ("transforms", transforms)):
            if a is None or isinstance(a, int):
                ptrs[name] = a
                continue
            n, width = want[name]
            if str(a.dtype) != "torch.float32" or not a.is_contiguous() or a.numel() != n * width or not a.is_cuda:
                raise ValueError(f"{name}: expected a contiguous float32 device tensor of {n} x {width} values")
            ptrs[name], tensors[name] = a.data_ptr(), a
        try:
            stream = _stream_arg(stream, self._handle_device)
        except Exception:                                              # None without torch: the null stream
            stream = None
        info = L.MiptUpdateInfo()
        L.check(L.load().mipt_scene_update_mesh_device(self._handle, ptrs["positions"], ptrs["normals"], ptrs["transforms"], mode, stream, C.byref(info)),
                "mipt_scene_update_mesh_device")
        for name, a in tensors.items():
            m[name] = np.ascontiguousarray(a.detach().cpu().numpy().reshape(-1, want[name][1]))
        if len(tensors) == sum(v is not None for v in ptrs.values()):
            self._mesh_mirror(mode)
        return info.as_dict()

    def mesh_info(self) -> dict:
        """MiptMeshInfo of the resident mesh: counts, parts, whether transforms are applied, HBM held."""
        self._resident()
        inf = L.MiptMeshInfo()
        L.check(L.load().mipt_scene_mesh_info(self._handle, C.byref(inf)), "mipt_scene_mesh_info")
        return inf.as_dict()

    def track_motion(self, on: bool = True) -> None:
        """mipt_scene_track_motion: keep the previous generation of the resident mesh from now on (it starts equal to the current
        one), so that ``Renderer.render_motion`` can take it as its source; ``on=False`` frees it."""
        self._resident()
        L.check(L.load().mipt_scene_track_motion(self._handle, 1 if on else 0), "mipt_scene_track_motion")
        self._tracks_motion = bool(on)

    def _fetch_bvh(self, handle) -> None:
        n = len(self.tris)
        nodes = np.zeros(max(2 * n, 1), dtype=L.NODE)
        order = np.zeros(n, dtype=np.uint32)
        count = C.c_uint32(0)
        L.check(L.load().mipt_scene_get_bvh(handle, L.ptr(nodes), len(nodes), C.byref(count), L.ptr(order)), "mipt_scene_get_bvh")
        self.bvh_nodes = nodes[: count.value].copy()
        self.tris = self.tris[order]
        self._tri_order = order

    def update_device(self, mode: int = L.UPDATE_REFIT) -> dict:
        """New geometry for the resident scene (mipt_scene_update_triangles) and/or its multi-GPU handle (mipt_multi_update_triangles)
        from ``self.tris`` after the caller edited them -- materials, textures and workspace stay in HBM.  REFIT keeps the tree and
        recomputes its bounds; REBUILD runs BVH::build on the GPU.  The device wants the order of the array it was last built from:
        when ``fetch_bvh`` reordered ``self.tris`` into the tree's order, they are scattered back first.  Afterwards ``bvh_nodes``
        (and, after a REBUILD of a scene that has a tree here, ``tris``) describe the scene on the device again.  Returns
        MiptUpdateInfo as a dict (of the last handle updated)."""
        multi = getattr(self, "_multi", None)
        if self._handle is None and multi is None:
            raise RuntimeError("scene is not resident on a device")
        src = self.tris
        if self._tri_order is not None:
            src = np.empty_like(self.tris)
            src[self._tri_order] = self.tris
        src = np.ascontiguousarray(src, dtype=L.TRIANGLE)
        lib = L.load()
        info = L.MiptUpdateInfo()
        if self._handle is not None:
            L.check(lib.mipt_scene_update_triangles(self._handle, L.ptr(src), len(src), mode, C.byref(info)), "mipt_scene_update_triangles")
        if multi is not None:
            L.check(lib.mipt_multi_update_triangles(multi, L.ptr(src), len(src), mode, C.byref(info)), "mipt_multi_update_triangles")
        h = self._handle if self._handle is not None else lib.mipt_multi_scene(multi, 0)
        had_tree = len(self.bvh_nodes) > 0
        if mode == L.UPDATE_REBUILD:
            self.tris, self._tri_order = src, None
            if had_tree:
                self._fetch_bvh(h)                                     # the new tree, tris in its order
        elif self._tri_order is not None:
            self._fetch_nodes(h)                                       # the refit bounds
        elif had_tree:
            self.bvh_nodes = refit_nodes(self.bvh_nodes, self.tris)    # a host-built tree: the same fold on the host
        return info.as_dict()

    def _fetch_nodes(self, handle) -> None:
        nodes = np.zeros(len(self.bvh_nodes), dtype=L.NODE)
        count = C.c_uint32(0)
        L.check(L.load().mipt_scene_get_bvh(handle, L.ptr(nodes), len(nodes), C.byref(count), None), "mipt_scene_get_bvh")
        self.bvh_nodes = nodes[: count.value].copy()

    # -- ray queries (include/mipt.h "ray queries") ---------------------------------------------
    _is_torch = staticmethod(_is_torch)
    _stream_arg = staticmethod(_stream_arg)

    # what the wrappers of the entries that take a list of work items share (queries, radiance queries, baking)
    def _resident(self, handle=None):
        h = handle if handle is not None else self._handle
        if h is None:
            raise RuntimeError("scene is not resident on a device")
        return h

    @staticmethod
    def _seeds(seeds, n: int) -> np.ndarray:
        s = seeds.detach().cpu().numpy() if Scene._is_torch(seeds) else np.asarray(seeds)
        if s.shape != (n,) or s.dtype.kind not in "iu" or s.dtype.itemsize != 4:
            raise ValueError(f"seeds: expected {n} 32-bit integers")
        return np.ascontiguousarray(s).view(np.uint32)

    @staticmethod
    def _radiance_out(accumulate_into, n: int, device, what: str, tail=(3,)):
        """-> (the [n, 3] float32 result tensor of a device entry on ``device``, whether it is the caller's running sum); ``tail``:
        what follows n in its shape ((9, 3) for the probes' coefficients)"""
        import torch
        shape = (n,) + tuple(tail)
        if accumulate_into is None:
            return torch.empty(shape, dtype=torch.float32, device=device), False
        out = accumulate_into
        if not Scene._is_torch(out) or out.dtype != torch.float32 or out.shape != shape or out.device != device or not out.is_contiguous():
            raise ValueError(f"accumulate_into: expected a contiguous float32 tensor of shape ({', '.join(map(str, shape))}) on the {what}' device")
        return out, True

    @staticmethod
    def _traced(rc, f, out, st):
        """the tail of a call that traces: a stack overflow leaves the results written (stats["stack_overflows"] > 0)"""
        if rc != L.ERR_STACK:
            L.check(rc, f.__name__)
        return out, st.as_dict()

    @staticmethod
    def _query_rays(rays, t_max):
        """-> ("host", RAY array [n]) or ("device", float32 cuda tensor [n, 8]); ValueError for anything else."""
        if isinstance(rays, (tuple, list)) and len(rays) == 2:
            o, d = rays
            if Scene._is_torch(o) != Scene._is_torch(d):
                raise ValueError("rays: origins and directions must both be numpy arrays or both torch tensors")
            if Scene._is_torch(o):
                import torch
                if o.dtype != torch.float32 or d.dtype != torch.float32 or o.dim() != 2 or o.shape[1] != 3 or d.shape != o.shape or not o.is_cuda or d.device != o.device:
                    raise ValueError("rays: (origins, directions) must be float32 device tensors of shape (n, 3) on one device")
                n = o.shape[0]
                t = torch.full((n,), 1e30, dtype=torch.float32, device=o.device) if t_max is None else torch.as_tensor(t_max, dtype=torch.float32, device=o.device)
                if t.dim() == 0:
                    t = t.expand(n)
                if t.shape != (n,):
                    raise ValueError(f"t_max: expected a scalar or {n} values")
                return "device", torch.cat([o, t.reshape(n, 1), d, torch.zeros((n, 1), dtype=torch.float32, device=o.device)], dim=1).contiguous()
            o, d = np.asarray(o), np.asarray(d)
            if o.dtype != np.float32 or d.dtype != np.float32 or o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
                raise ValueError("rays: (origins, directions) must be float32 arrays of shape (n, 3)")
            t = np.float32(1e30) if t_max is None else np.asarray(t_max, dtype=np.float32)
            if t.ndim > 1 or (t.ndim == 1 and t.shape != (len(o),)):
                raise ValueError(f"t_max: expected a scalar or {len(o)} values")
            out = np.zeros(len(o), dtype=L.RAY)
            out["origin"], out["direction"], out["t_max"] = o, d, t
            return "host", out
        if t_max is not None:
            raise ValueError("t_max is given only with (origins, directions); an n x 8 array carries its own")
        if Scene._is_torch(rays):
            import torch
            if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_cuda or not rays.is_contiguous():
                raise ValueError("rays: expected a contiguous float32 device tensor of shape (n, 8)")
            return "device", rays
        a = np.asarray(rays)
        if a.dtype == L.RAY and a.ndim == 1:
            return "host", np.ascontiguousarray(a)
        if a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 8:
            return "host", np.ascontiguousarray(a).view(L.RAY).reshape(-1)
        raise ValueError("rays: expected an (n, 8) float32 array, a RAY record array, a float32 device tensor of shape (n, 8) or (origins, directions)")

    def _query(self, anyhit: bool, rays, t_max, traversal, cull_margin, count, handle, stream):
        """-> (raw result, stats dict).  Host rays: a HIT record array / uint8 array; device rays: an int32 tensor [n, 4] (the MiptHit
        words) / a uint8 tensor, on the rays' device."""
        where, r = self._query_rays(rays, t_max)
        h = self._resident(handle)
        opt = L.MiptQueryOptions()
        opt.traversal, opt.cull_margin, opt.flags = traversal, cull_margin, (L.FLAG_COUNT if count else 0)
        st = L.MiptStats()
        lib = L.load()
        n = len(r)
        if where == "host":
            out = np.zeros(n, dtype=np.uint8 if anyhit else L.HIT)
            # n == 0: the library returns before it reads either buffer, but refuses null pointers
            f = lib.mipt_query_occluded if anyhit else lib.mipt_query_closest
            rc = f(h, L.ptr(r) if n else C.c_void_p(16), n, C.byref(opt), L.ptr(out) if n else C.c_void_p(16), C.byref(st))
        else:
            import torch
            out = torch.empty((n,), dtype=torch.uint8, device=r.device) if anyhit else torch.empty((n, 4), dtype=torch.int32, device=r.device)
            f = lib.mipt_query_occluded_device if anyhit else lib.mipt_query_closest_device
            rc = f(h, r.data_ptr() if n else 16, n, C.byref(opt), out.data_ptr() if n else 16, self._stream_arg(stream, r.device), C.byref(st))
        return self._traced(rc, f, out, st)

    def query_closest(self, rays, t_max=None, traversal: int = L.TRAVERSAL_REFERENCE, cull_margin: float = L.CULL_MARGIN_SAFE,
                      count: bool = False, handle=None, stream=None):
        """Closest hit of every ray on the resident scene (mipt_query_closest / _device): what Ray::traverse_bvh finds with
        hit_info.distance starting at t_max.  ``rays``: an (n, 8) float32 array {origin, t_max, direction, 0} or RAY records (host
        entry); a contiguous float32 device tensor of shape (n, 8) (device entry on ``stream`` -- a torch stream, a raw hipStream_t or
        None = torch's current stream -- returning torch tensors); or ``(origins, directions)`` of shape (n, 3) with ``t_max`` a
        scalar or n values (None = 1e30).  Returns ({"t", "u", "v", "prim", "front_face", "hit"}, stats): prim is the triangle's
        index in the caller's order as int64, -1 for a miss (then t = 1e30, u = v = 0)."""
        raw, stats = self._query(False, rays, t_max, traversal, cull_margin, count, handle, stream)
        if isinstance(raw, np.ndarray):
            p = raw["prim"].astype(np.int64)
            hit = p != L.HIT_NONE
            return dict(t=raw["t"].copy(), u=raw["u"].copy(), v=raw["v"].copy(), prim=np.where(hit, p & L.HIT_TRI_MASK, -1),
                        front_face=hit & ((p & L.HIT_FRONT_FACE) != 0), hit=hit), stats
        import torch
        f = raw.view(torch.float32)
        p = raw[:, 3].to(torch.int64) & 0xFFFFFFFF
        hit = p != L.HIT_NONE
        return dict(t=f[:, 0].clone(), u=f[:, 1].clone(), v=f[:, 2].clone(), prim=torch.where(hit, p & L.HIT_TRI_MASK, torch.full_like(p, -1)),
                    front_face=hit & ((p & L.HIT_FRONT_FACE) != 0), hit=hit), stats

    def query_occluded(self, rays, t_max=None, traversal: int = L.TRAVERSAL_REFERENCE, cull_margin: float = L.CULL_MARGIN_SAFE,
                       count: bool = False, handle=None, stream=None):
        """Is anything in front of t_max on every ray (mipt_query_occluded / _device)?  Arguments as ``query_closest``.  Returns
        (bool array or tensor [n], stats)."""
        raw, stats = self._query(True, rays, t_max, traversal, cull_margin, count, handle, stream)
        return raw != 0, stats

    # -- radiance queries (include/mipt.h "radiance queries") -------------------------------------
    @staticmethod
    def radiance_default_seeds(n: int, first: int = 0) -> np.ndarray:
        """The seeds ``query_radiance`` gives rays first ... first + n - 1 when the caller brings none: the pixel formula of
        cpu.rs:28-29, 987612486 * (i + 87636354) mod 2^32, with 1 where that is 0 (a zero seed is a stuck xorshift stream)."""
        i = np.arange(first, first + n, dtype=np.uint64)
        s = ((np.uint64(987612486) * (i + np.uint64(87636354))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        s[s == 0] = 1
        return s

    def query_radiance(self, rays, seeds=None, samples: int = 1, max_ray_depth: int = 8, traversal: int = L.TRAVERSAL_REFERENCE,
                       cull_margin: float = L.CULL_MARGIN_SAFE, shading: int = 0, sum_only: bool = False, accumulate_into=None,
                       count: bool = False, handle=None, stream=None):
        """Path-traced radiance along every ray on the resident scene (mipt_query_radiance / _device): ``samples`` paths of at most
        ``max_ray_depth`` segments per ray on one xorshift stream that starts at the ray's seed, their mean (``sum_only``: their
        sum).  ``rays`` as for ``query_closest`` (t_max is not used).  ``seeds``: n uint32 values; None = ``radiance_default_seeds``
        -- except for an (n, 8) device tensor, whose last column is then the caller's seeds (int32 bits).  ``accumulate_into``: a
        float32 device tensor [n, 3] the call's sums are added to (device rays only; implies ``sum_only``; bring fresh seeds every
        call).  Returns (radiance [n, 3] float32 array or tensor, stats)."""
        where, r = self._query_rays(rays, None)
        h = self._resident(handle)
        n = len(r)
        given = seeds is not None
        if given:
            s = self._seeds(seeds, n)
        elif where == "host" or isinstance(rays, (tuple, list)):
            s, given = self.radiance_default_seeds(n), True
        opt = L.MiptRadianceOptions()
        opt.samples, opt.max_ray_depth, opt.traversal, opt.cull_margin, opt.shading = samples, max_ray_depth, traversal, cull_margin, shading
        opt.flags = (L.FLAG_COUNT if count else 0) | (L.FLAG_SUM if sum_only or accumulate_into is not None else 0)
        st = L.MiptStats()
        lib = L.load()
        if where == "host":
            if accumulate_into is not None:
                raise ValueError("accumulate_into needs device rays: the running sum lives in a device tensor")
            r = r.copy()                                       # the caller's array keeps its last column
            r["reserved"] = s
            out = np.zeros((n, 3), dtype=np.float32)
            f = lib.mipt_query_radiance
            rc = f(h, L.ptr(r) if n else C.c_void_p(16), n, C.byref(opt), L.ptr(out) if n else C.c_void_p(16), C.byref(st))
        else:
            import torch
            if given:
                if r is rays:
                    r = r.clone()
                r[:, 7] = torch.from_numpy(s.view(np.int32)).to(r.device).view(torch.float32)
            out, accum = self._radiance_out(accumulate_into, n, r.device, "rays")
            opt.flags |= L.FLAG_ACCUM if accum else 0
            f = lib.mipt_query_radiance_device
            rc = f(h, r.data_ptr() if n else 16, n, C.byref(opt), out.data_ptr() if n else 16, self._stream_arg(stream, r.device), C.byref(st))
        return self._traced(rc, f, out, st)

    # -- baking (include/mipt.h "baking") ------------------------------------------------------------
    def bake_texels(self, width: int, height: int, stream=None, device: bool = False, handle=None):
        """The surface point behind every texel of a ``width`` x ``height`` lightmap atlas laid out by the scene's own UVs
        (mipt_bake_texels / _device).  Returns (points, info): SURFACE_POINT records [width * height], texel (x, y) at index
        y * width + x, seed = that index, prim = HIT_NONE where no triangle covers the texel centre; with ``device`` an int32 device
        tensor [width * height, 4] of the same words, made on ``stream`` (a torch stream, a raw hipStream_t or None = torch's current
        stream).  info: covered_texels, degenerate_tris, kernel_ms."""
        h = self._resident(handle)
        if not (isinstance(width, (int, np.integer)) and isinstance(height, (int, np.integer))) or width < 0 or height < 0 or width >= 1 << 32 or height >= 1 << 32:
            raise ValueError("width, height: expected two non-negative 32-bit integers")
        n = int(width) * int(height)
        info = L.MiptBakeTexelInfo()
        lib = L.load()
        if device:
            import torch
            dev = torch.device("cuda", self._handle_device if handle is None else torch.cuda.current_device())   # a foreign handle: the caller's current device
            out = torch.empty((n, 4), dtype=torch.int32, device=dev)
            f = lib.mipt_bake_texels_device
            rc = f(h, width, height, None, out.data_ptr() if n else 16, self._stream_arg(stream, dev), C.byref(info))
        else:
            out = np.zeros(n, dtype=L.SURFACE_POINT)
            f = lib.mipt_bake_texels
            rc = f(h, width, height, None, L.ptr(out) if n else C.c_void_p(16), C.byref(info))
        L.check(rc, f.__name__)
        return out, info.as_dict()

    @staticmethod
    def _bake_points(points, seeds):
        """-> ("host", SURFACE_POINT array [n]) or ("device", int32 cuda tensor [n, 4]); ValueError for anything else.  A dict is what
        ``query_closest`` returns; it needs ``seeds``."""
        if isinstance(points, dict):
            if seeds is None:
                raise ValueError("points: the hits of query_closest carry no seeds: give seeds")
            u, v, prim, front = points["u"], points["v"], points["prim"], points["front_face"]
            if Scene._is_torch(u):
                import torch
                p = torch.where(prim < 0, torch.full_like(prim, L.HIT_NONE), prim | (front.to(torch.int64) << 31))
                p = torch.where(p >= 1 << 31, p - (1 << 32), p).to(torch.int32)                 # the u32 word as int32 bits
                ub, vb = u.contiguous().view(torch.int32), v.contiguous().view(torch.int32)
                points = torch.stack([torch.zeros_like(ub), ub, vb, p], dim=1).contiguous()
            else:
                rec = np.zeros(len(u), dtype=L.SURFACE_POINT)
                rec["u"], rec["v"] = u, v
                pr = np.asarray(prim, dtype=np.int64)
                rec["prim"] = np.where(pr < 0, L.HIT_NONE, pr | (np.asarray(front, dtype=np.int64) << 31)).astype(np.uint32)
                points = rec
        if Scene._is_torch(points):
            import torch
            if points.dtype != torch.int32 or points.dim() != 2 or points.shape[1] != 4 or not points.is_cuda or not points.is_contiguous():
                raise ValueError("points: expected a contiguous int32 device tensor of shape (n, 4)")
            where, r = "device", points
        else:
            a = np.asarray(points)
            if a.dtype == L.SURFACE_POINT and a.ndim == 1:
                r = np.ascontiguousarray(a)
            elif a.dtype == L.HIT and a.ndim == 1:
                r = np.ascontiguousarray(a).view(L.SURFACE_POINT)
            elif a.dtype in (np.dtype(np.uint32), np.dtype(np.int32)) and a.ndim == 2 and a.shape[1] == 4:
                r = np.ascontiguousarray(a).view(L.SURFACE_POINT).reshape(-1)
            else:
                raise ValueError("points: expected SURFACE_POINT or HIT records, an (n, 4) array of 32-bit words, an int32 device tensor "
                                 "of shape (n, 4) or the dict query_closest returns")
            where = "host"
        if seeds is not None:
            s = Scene._seeds(seeds, len(r))
            if where == "host":
                r = r.copy()
                r["seed"] = s
            else:
                import torch
                if r is points:
                    r = r.clone()
                r[:, 0] = torch.from_numpy(s.view(np.int32)).to(r.device)
        return where, r

    def bake_gather(self, points, seeds=None, samples: int = 1, max_ray_depth: int = 8, traversal: int = L.TRAVERSAL_REFERENCE,
                    cull_margin: float = L.CULL_MARGIN_SAFE, shading: int = 0, sum_only: bool = False, first_sample: int = 0, sample_stride=None,
                    accumulate_into=None, count: bool = False, handle=None, stream=None):
        """The light every surface point gathers over its hemisphere (mipt_bake_gather / _device): ``samples`` paths per point, each
        leaving along normalized(N + rand_in_unit_sphere) on a stream seeded from the point's seed and the sample's number
        ``first_sample + s``; their mean (``sum_only``: their sum).  ``points``: what ``bake_texels`` returns (host records or the
        device tensor), HIT records with seeds, an (n, 4) array of the record's words, or the dict ``query_closest`` returns -- the
        last two kinds of hits need ``seeds`` (n uint32).  ``sample_stride``: None = the number of points.  ``accumulate_into``: a
        float32 device tensor [n, 3] the call's samples are added to (device points only; implies ``sum_only``).  Returns
        (radiance [n, 3] float32 array or tensor, stats)."""
        where, r = self._bake_points(points, seeds)
        h = self._resident(handle)
        n = len(r)
        opt = L.MiptBakeOptions()
        opt.samples, opt.max_ray_depth, opt.traversal, opt.cull_margin, opt.shading = samples, max_ray_depth, traversal, cull_margin, shading
        opt.first_sample, opt.sample_stride = first_sample, (max(n, 1) if sample_stride is None else sample_stride)
        opt.flags = (L.FLAG_COUNT if count else 0) | (L.FLAG_SUM if sum_only or accumulate_into is not None else 0)
        st = L.MiptStats()
        lib = L.load()
        if where == "host":
            if accumulate_into is not None:
                raise ValueError("accumulate_into needs device points: the running sum lives in a device tensor")
            out = np.zeros((n, 3), dtype=np.float32)
            f = lib.mipt_bake_gather
            rc = f(h, L.ptr(r) if n else C.c_void_p(16), n, C.byref(opt), L.ptr(out) if n else C.c_void_p(16), C.byref(st))
        else:
            out, accum = self._radiance_out(accumulate_into, n, r.device, "points")
            opt.flags |= L.FLAG_ACCUM if accum else 0
            f = lib.mipt_bake_gather_device
            rc = f(h, r.data_ptr() if n else 16, n, C.byref(opt), out.data_ptr() if n else 16, self._stream_arg(stream, r.device), C.byref(st))
        return self._traced(rc, f, out, st)

    def bake_surface(self, points, unit_normals: bool = False, handle=None, stream=None, want=("position", "normal")):
        """World position and interpolated normal of every surface point (mipt_bake_surface / _device): the P and N ``bake_gather``
        leaves from, the guides of ``lightmap_filter``.  ``points`` as for ``bake_gather`` (no seeds needed).  ``unit_normals``:
        normalized(N) instead of N as formed.  ``want``: which of the two to compute.  Returns (position, normal), [n, 3] float32
        arrays (host points) or device tensors (device points); None for one not wanted.  A HIT_NONE point yields zeros."""
        where, r = self._bake_points(points, None if not isinstance(points, dict) else np.zeros(len(points["u"]), dtype=np.uint32))
        want = tuple(want)
        if not want or any(w not in ("position", "normal") for w in want):
            raise ValueError('want: expected "position", "normal" or both')
        h = self._resident(handle)
        n = len(r)
        opt = L.MiptBakeSurfaceOptions()
        opt.flags = L.BAKE_SURFACE_UNIT_NORMALS if unit_normals else 0
        lib = L.load()
        if where == "host":
            outs = [np.zeros((n, 3), dtype=np.float32) if w in want else None for w in ("position", "normal")]
            ptrs = [None if o is None else (L.ptr(o) if n else C.c_void_p(16)) for o in outs]
            L.check(lib.mipt_bake_surface(h, L.ptr(r) if n else C.c_void_p(16), n, C.byref(opt), ptrs[0], ptrs[1]), "mipt_bake_surface")
        else:
            import torch
            outs = [torch.empty((n, 3), dtype=torch.float32, device=r.device) if w in want else None for w in ("position", "normal")]
            ptrs = [None if o is None else (o.data_ptr() if n else 16) for o in outs]
            L.check(lib.mipt_bake_surface_device(h, r.data_ptr() if n else 16, n, C.byref(opt), ptrs[0], ptrs[1], self._stream_arg(stream, r.device)),
                    "mipt_bake_surface_device")
        return outs[0], outs[1]

    @staticmethod
    def _lightmap_planes(radiance, points, guides):
        """-> (torch?, (H, W), radiance, points, {name: guide}); ValueError naming the argument for anything else."""
        if not _is_torch(radiance):
            radiance = np.asarray(radiance)
        if radiance.ndim != 3 or radiance.shape[-1] != 3:
            raise ValueError(f"radiance: expected shape [H,W,3]; got {tuple(radiance.shape)}")
        h, w = int(radiance.shape[0]), int(radiance.shape[1])
        where, pts = Scene._bake_points(points, None)
        if (where == "device") != _is_torch(radiance):
            raise ValueError("points: radiance and points must both be numpy arrays or both device tensors")
        if len(pts) != h * w:
            raise ValueError(f"points: expected {h * w} records, one per texel; got {len(pts)}")
        torch_in, planes = _check_planes("radiance", radiance, "radiance and the guides",
                                         [(name, a, (h, w, 3), False) for name, a in [("radiance", radiance)] + list(guides.items())], flat=True)
        if torch_in and pts.device != radiance.device:
            raise ValueError(f"points: expected a tensor on radiance's device {radiance.device}")
        return torch_in, (h, w), planes.pop("radiance"), pts, planes

    @staticmethod
    def lightmap_filter(radiance, points, position=None, normal=None, iterations: int = 5, sigma_color: float = 4.0, sigma_normal: float = 0.5,
                        sigma_plane: float = 0.05, sigma_distance: float = 0.5, device_id: int = 0, stream=None):
        """The edge-avoiding a-trous filter of include/mipt.h "lightmap finishing" over the covered texels of one atlas: ``radiance``
        [H,W,3] float32, ``points`` the H*W records of ``bake_texels``, the optional guides ``position`` and ``normal`` [H,W,3] (or
        [H*W,3], as ``bake_surface`` returns them; None = their terms are left out).  Uncovered texels are never taps and come back
        unchanged.  numpy arrays go through mipt_lightmap_filter on ``device_id``; device tensors through mipt_lightmap_filter_device
        on ``stream`` without blocking.  Returns a new array / tensor [H,W,3]."""
        torch_in, (h, w), rad, pts, g = Scene._lightmap_planes(radiance, points, {"position": position, "normal": normal})
        opt = L.MiptLightmapFilterOptions()
        opt.width, opt.height, opt.iterations = w, h, iterations
        opt.sigma_color, opt.sigma_normal, opt.sigma_plane, opt.sigma_distance = sigma_color, sigma_normal, sigma_plane, sigma_distance
        bufs = L.MiptLightmapFilterBuffers()
        lib = L.load()
        if torch_in:
            import torch
            out = torch.empty_like(rad)
            touched = _fill(bufs, radiance=rad, points=pts, out=out, **g)
            raw, ws = _stream_ordered(rad.device, stream, touched, lib.mipt_lightmap_filter_workspace_bytes(w, h))
            L.check(lib.mipt_lightmap_filter_device(C.byref(opt), C.byref(bufs), ws.data_ptr(), ws.numel() * 4, raw), "mipt_lightmap_filter_device")
            return out
        out = np.empty_like(rad)
        _fill(bufs, radiance=rad, points=pts, out=out, **g)
        L.check(lib.mipt_lightmap_filter(C.byref(opt), C.byref(bufs), device_id), "mipt_lightmap_filter")
        return out

    @staticmethod
    def lightmap_dilate(radiance, points, radius: int = 2, want_level: bool = False, device_id: int = 0, stream=None):
        """Dilation of include/mipt.h "lightmap finishing": ``radius`` passes, each filling the uncovered texels that touch a covered
        or already filled one with the mean of those neighbours.  ``radiance`` [H,W,3] float32 and ``points`` as for
        ``lightmap_filter``.  Returns the dilated atlas [H,W,3], or (atlas, level [H,W] uint32 -- int32 for a tensor) with
        ``want_level``: 1 = covered, k + 1 = filled in pass k, 0 = still empty."""
        torch_in, (h, w), rad, pts, _ = Scene._lightmap_planes(radiance, points, {})
        opt = L.MiptLightmapDilateOptions()
        opt.width, opt.height, opt.radius = w, h, radius
        bufs = L.MiptLightmapDilateBuffers()
        lib = L.load()
        if torch_in:
            import torch
            out = torch.empty_like(rad)
            level = torch.empty((h, w), dtype=torch.int32, device=rad.device) if want_level else None
            touched = _fill(bufs, radiance=rad, points=pts, out=out, level=level)
            raw, ws = _stream_ordered(rad.device, stream, touched, lib.mipt_lightmap_dilate_workspace_bytes(w, h))
            L.check(lib.mipt_lightmap_dilate_device(C.byref(opt), C.byref(bufs), ws.data_ptr(), ws.numel() * 4, raw), "mipt_lightmap_dilate_device")
        else:
            out = np.empty_like(rad)
            level = np.zeros((h, w), dtype=np.uint32) if want_level else None
            _fill(bufs, radiance=rad, points=pts, out=out, level=level)
            L.check(lib.mipt_lightmap_dilate(C.byref(opt), C.byref(bufs), device_id), "mipt_lightmap_dilate")
        return (out, level) if want_level else out

    def bake_lightmap(self, width: int, height: int, samples: int, device=None, stream=None, filter=None, dilate: int = 0, **gather_args):
        """``bake_texels`` then ``bake_gather`` with the texel indices as seeds: the mean radiance every covered texel of the atlas
        gathers.  With torch and a visible device (``device`` None) or ``device=True`` both steps stay in HBM and tensors come back;
        otherwise numpy arrays.  ``filter``: None, or a dict of ``lightmap_filter``'s options -- the atlas is then filtered, guided
        by ``bake_surface``'s position and unit normal; ``dilate`` > 0: ``lightmap_dilate`` with that radius afterwards.  With
        neither, the result and the calls are those of the two steps alone.  Returns (atlas [height, width, 3] float32, covered
        [height, width] bool -- the texel pass's mask, whatever was dilated --, stats); stats carries the texel pass's info under
        "texels"."""
        if device is None:
            try:
                import torch
                device = torch.cuda.is_available()
            except ImportError:
                device = False
        points, info = self.bake_texels(width, height, stream=stream, device=device, handle=gather_args.get("handle"))
        rad, stats = self.bake_gather(points, samples=samples, stream=stream, **gather_args)
        stats["texels"] = info
        if device:
            covered = (points[:, 3] != -1).reshape(height, width)
        else:
            covered = (points["prim"] != L.HIT_NONE).reshape(height, width)
        rad = rad.reshape(height, width, 3)
        if width and height and (filter is not None or dilate):
            device_id = self._handle_device if gather_args.get("handle") is None else 0
            if filter is not None:
                pos, nrm = self.bake_surface(points, unit_normals=True, handle=gather_args.get("handle"), stream=stream)
                rad = Scene.lightmap_filter(rad, points, position=pos, normal=nrm, device_id=device_id, stream=stream, **dict(filter))
            if dilate:
                rad = Scene.lightmap_dilate(rad, points, radius=dilate, device_id=device_id, stream=stream)
        return rad, covered, stats

    # -- irradiance probes (include/mipt.h "irradiance probes") ----------------------------------------
    def bake_probes(self, positions, seeds=None, samples: int = 64, max_ray_depth: int = 8, traversal: int = L.TRAVERSAL_REFERENCE,
                    cull_margin: float = L.CULL_MARGIN_SAFE, shading: int = 0, first_sample: int = 0, sample_stride=None, sum: bool = False,
                    accumulate_into=None, count: bool = False, stream=None, handle=None):
        """The light that arrives at every probe from the whole sphere, projected onto real spherical harmonics up to band 2
        (mipt_probe_bake / _device): ``samples`` paths per probe, each leaving the probe's position along rand_in_unit_sphere on a
        stream seeded from the probe's seed and the sample's number ``first_sample + s``.  ``positions``: [n, 3] float32, a numpy
        array (host entry) or a device tensor (device entry on ``stream``).  ``seeds``: n uint32, None = ``radiance_default_seeds``;
        ``sample_stride``: None = n.  ``sum``: the ordered sums instead of the coefficients; ``accumulate_into``: a float32 device
        tensor [n, 9, 3] the call's samples are added to (device positions only; implies ``sum``).  Returns (sh [n, 9, 3] float32
        array or tensor -- coefficient k of channel c at [i, k, c] --, stats)."""
        torch_in = _is_torch(positions)
        if torch_in:
            import torch
            if positions.dtype != torch.float32 or positions.dim() != 2 or positions.shape[1] != 3 or not positions.is_cuda:
                raise ValueError("positions: expected a float32 device tensor of shape (n, 3)")
        else:
            positions = np.asarray(positions)
            if positions.dtype != np.float32 or positions.ndim != 2 or positions.shape[1] != 3:
                raise ValueError("positions: expected a float32 array of shape (n, 3)")
        h = self._resident(handle)
        n = int(positions.shape[0])
        s = self.radiance_default_seeds(n) if seeds is None else self._seeds(seeds, n)
        opt = L.MiptProbeBakeOptions()
        opt.samples, opt.max_ray_depth, opt.traversal, opt.cull_margin, opt.shading = samples, max_ray_depth, traversal, cull_margin, shading
        opt.first_sample, opt.sample_stride = first_sample, (max(n, 1) if sample_stride is None else sample_stride)
        opt.flags = (L.FLAG_COUNT if count else 0) | (L.FLAG_SUM if sum or accumulate_into is not None else 0)
        st = L.MiptStats()
        lib = L.load()
        if not torch_in:
            if accumulate_into is not None:
                raise ValueError("accumulate_into needs device positions: the running sum lives in a device tensor")
            r = np.zeros(n, dtype=L.PROBE)
            r["position"], r["seed"] = positions, s
            out = np.zeros((n, 9, 3), dtype=np.float32)
            f = lib.mipt_probe_bake
            rc = f(h, L.ptr(r) if n else C.c_void_p(16), n, C.byref(opt), L.ptr(out) if n else C.c_void_p(16), C.byref(st))
        else:
            r = torch.cat([positions, torch.from_numpy(s.view(np.int32)).to(positions.device).view(torch.float32).reshape(n, 1)], dim=1).contiguous()
            out, accum = self._radiance_out(accumulate_into, n, r.device, "positions", tail=(9, 3))
            opt.flags |= L.FLAG_ACCUM if accum else 0
            f = lib.mipt_probe_bake_device
            rc = f(h, r.data_ptr() if n else 16, n, C.byref(opt), out.data_ptr() if n else 16, self._stream_arg(stream, r.device), C.byref(st))
        return self._traced(rc, f, out, st)

    @staticmethod
    def probe_grid(origin, spacing, dims) -> np.ndarray:
        """The positions of a ``dims[0]`` x ``dims[1]`` x ``dims[2]`` probe grid in index order, (iz * dims[1] + iy) * dims[0] + ix:
        origin + spacing * (ix, iy, iz), one f32 multiplication and addition per coordinate.  -> [n, 3] float32"""
        o, sp = np.asarray(origin, dtype=np.float32), np.asarray(spacing, dtype=np.float32)
        d = [int(x) for x in dims]
        if o.shape != (3,) or sp.shape != (3,) or len(d) != 3 or min(d) < 1:
            raise ValueError("probe_grid: expected origin [3], spacing [3] and three dimensions greater than 0")
        iz, iy, ix = np.meshgrid(*(np.arange(k, dtype=np.float32) for k in (d[2], d[1], d[0])), indexing="ij")
        return np.ascontiguousarray(o + sp * np.stack([ix, iy, iz], axis=-1).reshape(-1, 3))

    @staticmethod
    def probe_irradiance(sh, grid, position, normal, valid=None, clamp: bool = False, device_id: int = 0, stream=None):
        """Irradiance at every point from a grid of baked probes (mipt_probe_irradiance / _device): the trilinear blend of the cell's
        eight probes, then the clamped-cosine convolution at ``normal`` (used as given).  ``sh``: [n_probes, 9, 3] float32, what
        ``bake_probes`` returns for ``probe_grid(*grid)``; ``grid``: (origin, spacing, dims); ``position``, ``normal``: [n, 3]
        float32; ``valid``: n_probes uint8 (a bool array or tensor is taken as such), 0 = leave the probe out; ``clamp``: no negative
        result.  numpy arrays go through the host entry on ``device_id``; device tensors through the device entry on ``stream``
        without blocking.  Returns [n, 3] float32."""
        origin, spacing, dims = grid
        g = L.MiptProbeGrid()
        g.origin[:], g.spacing[:], g.dims[:] = [float(x) for x in origin], [float(x) for x in spacing], [int(x) for x in dims]
        g.flags = L.PROBE_CLAMP if clamp else 0
        n_probes = int(g.dims[0]) * int(g.dims[1]) * int(g.dims[2])
        if not _is_torch(position):
            position = np.asarray(position)
        if position.ndim != 2 or position.shape[1] != 3:
            raise ValueError(f"position: expected shape [n,3]; got {tuple(position.shape)}")
        n = int(position.shape[0])
        torch_in, planes = _check_planes("position", position, "sh, position and normal",
                                         [("position", position, (n, 3), False), ("normal", normal, (n, 3), False), ("sh", sh, (n_probes, 9, 3), False)],
                                         flat=True, required=("normal", "sh"), missing="needed")
        if valid is not None:
            if _is_torch(valid) != torch_in:
                raise ValueError("valid: sh, position and normal must all be numpy arrays or all torch tensors")
            if torch_in:
                import torch
                if valid.dtype not in (torch.uint8, torch.bool) or valid.numel() != n_probes or valid.device != position.device or not valid.is_contiguous():
                    raise ValueError(f"valid: expected {n_probes} contiguous uint8 or bool values on position's device")
                valid = valid.view(torch.uint8)
            else:
                valid = np.asarray(valid)
                if valid.dtype not in (np.dtype(np.uint8), np.dtype(bool)) or valid.size != n_probes:
                    raise ValueError(f"valid: expected {n_probes} uint8 or bool values")
                valid = np.ascontiguousarray(valid).view(np.uint8)
        bufs = L.MiptProbeIrradianceBuffers()
        lib = L.load()
        if torch_in:
            import torch
            out = torch.empty((n, 3), dtype=torch.float32, device=position.device)
            touched = _fill(bufs, irradiance=out, valid=valid, **planes)
            raw, _ = _stream_ordered(position.device, stream, touched)
            if n == 0:
                bufs.position = bufs.normal = bufs.irradiance = 16
            L.check(lib.mipt_probe_irradiance_device(C.byref(g), n, C.byref(bufs), raw), "mipt_probe_irradiance_device")
            return out
        out = np.zeros((n, 3), dtype=np.float32)
        _fill(bufs, irradiance=out, valid=valid, **planes)
        if n == 0:
            bufs.position = bufs.normal = bufs.irradiance = 16
        L.check(lib.mipt_probe_irradiance(C.byref(g), n, C.byref(bufs), device_id), "mipt_probe_irradiance")
        return out

    def info(self, handle=None) -> dict:
        """MiptSceneInfo of the resident scene (sizes + what the setup took)."""
        h = self._resident(handle)
        inf = L.MiptSceneInfo()
        L.check(L.load().mipt_scene_info(h, C.byref(inf)), "mipt_scene_info")
        return inf.as_dict()

    def release(self) -> None:
        if self._handle is not None:
            L.load().mipt_scene_destroy(self._handle)
            self._handle = None
            self._tracks_motion = False
        if getattr(self, "_multi", None) is not None:
            L.load().mipt_multi_destroy(self._multi)
            self._multi = None

    def upload_multi(self, device_ids=None, from_triangles: bool = False, fetch_bvh: bool = False) -> C.c_void_p:
        """One replica + RCCL communicator per device (mipt_multi_create); device_ids None = every visible device.  The scene crosses
        PCIe once (to the first device), the other replicas are device-to-device copies.  ``from_triangles``: the BVH is built on
        that first device (mipt_multi_create_from_triangles); ``fetch_bvh`` then leaves nodes + reordered triangles in this Scene."""
        key = (None if device_ids is None else tuple(device_ids), from_triangles)
        if getattr(self, "_multi", None) is not None and self._multi_key == key:
            return self._multi
        if getattr(self, "_multi", None) is not None:
            L.load().mipt_multi_destroy(self._multi)
            self._multi = None
        h = C.c_void_p()
        d = self.desc()
        if self._handle is None:
            self._tri_order = None                                     # the replicas are built from tris as they are now
        ids = None if device_ids is None else (C.c_int * len(device_ids))(*device_ids)
        lib = L.load()
        if from_triangles:
            L.check(lib.mipt_multi_create_from_triangles(C.byref(d), ids, 0 if device_ids is None else len(device_ids), C.byref(h)), "mipt_multi_create_from_triangles")
            if fetch_bvh:
                self._fetch_bvh(lib.mipt_multi_scene(h, 0))
        else:
            L.check(lib.mipt_multi_create(C.byref(d), ids, 0 if device_ids is None else len(device_ids), C.byref(h)), "mipt_multi_create")
        self._multi, self._multi_key = h, key
        return h

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def refit_nodes(nodes: np.ndarray, tris: np.ndarray) -> np.ndarray:
    """The REFIT of mipt_scene_update_triangles on the host: `nodes` with every bound re-folded by Node::grow_by_tri (bvh.rs:185-193)
    over the node's triangles (`tris` in the tree's order) -- leaves over their range, inner nodes as the union of their children,
    deepest level first.  f32 min/max ignore a NaN coordinate, as f32::min / f32::max do."""
    out = nodes.copy()
    big = np.float32(3.4028235e38)
    pos = np.asarray(tris["vertices"]["position"], dtype=np.float32)
    lo = np.fmin(np.fmin.reduce(pos, axis=1), big)                 # per triangle, from Node::default's +-f32::MAX
    hi = np.fmax(np.fmax.reduce(pos, axis=1), -big)
    leaf = np.flatnonzero(out["num_tris"] > 0)
    if len(leaf):
        f, n = out["first_tri_or_child"][leaf].astype(np.int64), out["num_tris"][leaf].astype(np.int64)
        lo_s, hi_s = np.vstack([lo, np.full((1, 3), big, np.float32)]), np.vstack([hi, np.full((1, 3), -big, np.float32)])
        idx = np.stack([f, f + n], axis=1).ravel()
        out["bounds_min"][leaf] = np.fmin.reduceat(lo_s, idx, axis=0)[::2]
        out["bounds_max"][leaf] = np.fmax.reduceat(hi_s, idx, axis=0)[::2]
    levels, cur = [], np.array([0], dtype=np.int64)              # inner nodes by depth, from the root
    while len(cur):
        inner = cur[out["num_tris"][cur] == 0]
        if len(inner):
            levels.append(inner)
        c = out["first_tri_or_child"][inner].astype(np.int64)
        cur = np.concatenate([c, c + 1])
    for inner in reversed(levels):
        c = out["first_tri_or_child"][inner].astype(np.int64)
        out["bounds_min"][inner] = np.fmin(out["bounds_min"][c], out["bounds_min"][c + 1])
        out["bounds_max"][inner] = np.fmax(out["bounds_max"][c], out["bounds_max"][c + 1])
    return out


def make_options(width, height, samples, max_ray_depth, seed_mode=L.SEED_PIXEL_STREAM, traversal=L.TRAVERSAL_REFERENCE,
                 flags=0, tile_rank=0, tile_world=0, sample_begin=0, cull_margin=L.CULL_MARGIN_SAFE, shading=0) -> L.MiptOptions:
    o = L.MiptOptions()
    o.width, o.height, o.samples, o.max_ray_depth = width, height, samples, max_ray_depth
    o.seed_mode, o.traversal, o.flags = seed_mode, traversal, flags
    o.tile_rank, o.tile_world, o.sample_begin = tile_rank, tile_world, sample_begin
    o.cull_margin = cull_margin
    o.shading = shading
    return o


class Renderer:  # renderer.rs:8-85
    def __init__(self, options: RendererOptions):
        self.options = options
        self.last_stats: Optional[dict] = None

    @staticmethod
    def new(options: RendererOptions) -> Optional["Renderer"]:  # renderer.rs:14-48
        w, h = options.output_image_dimensions
        if w == 0 or h == 0:
            log_error("Width and height must be greater than 0")
            return None
        if options.max_ray_depth == 0:
            log_error("Max ray depth must be greater than 0")
            return None
        if options.samples == 0:
            log_error("Sample count must be greater than 0")
            return None
        if options.output_image_path is None and not options.is_realtime:
            log_error("Output image path must be Some if realtime mode is disabled")
            return None
        if options.backend != RendererBackend.GPU and options.is_realtime:
            log_error("Only the GPU backend is supported for realtime mode")
            return None
        return Renderer(options)

    def _mi355x(self) -> RendererOptions:
        """the options, for an arm that only this build's backend has"""
        o = self.options
        if o.backend != RendererBackend.MI355X:
            raise NotImplementedError(f"backend {o.backend.name} is not part of this build; use RendererBackend.MI355X")
        return o

    def _traced(self, rc, f, st) -> dict:
        """``Scene._traced`` for a render: its stats are ``last_stats`` as well"""
        _, self.last_stats = Scene._traced(rc, f, None, st)
        return self.last_stats

    def render_buffers(self, scene: Scene, want_hdr: bool = True, want_rgba8: bool = True, flags: int = 0):
        """The backend arm: (Renderer, &Scene) -> pixels.  Returns (hdr float32 [h,w,3] | None,
        rgba8 uint8 [h,w,4] | None, stats dict)."""
        o = self._mi355x()
        w, h = o.output_image_dimensions
        handle = scene.upload(o.device_id)
        opt = make_options(w, h, o.samples, o.max_ray_depth, o.seed_mode, o.traversal, flags, cull_margin=o.cull_margin, shading=o.shading)
        hdr = np.zeros((h, w, 3), dtype=np.float32) if want_hdr else None
        rgba = np.zeros((h, w, 4), dtype=np.uint8) if want_rgba8 else None
        st = L.MiptStats()
        rc = L.load().mipt_render(handle, L.ptr(scene.camera.uniform), C.byref(opt),
                                  L.ptr(hdr) if want_hdr else None, L.ptr(rgba) if want_rgba8 else None, C.byref(st))
        L.check(rc, "mipt_render")
        self.last_stats = st.as_dict()
        return hdr, rgba, self.last_stats

    def render_buffers_batch(self, scene: Scene, cameras, want_hdr: bool = True, want_rgba8: bool = True, flags: int = 0):
        """Many views of one scene in one launch (mipt_render_batch): `cameras` is a sequence of Camera (or CAMERA records), all
        rendered with this renderer's options.  View i equals render_buffers with cameras[i].  Returns (hdr float32 [n,h,w,3] |
        None, rgba8 uint8 [n,h,w,4] | None, stats dict of the one launch)."""
        o = self._mi355x()
        table = _camera_table(list(cameras), "render_buffers_batch")
        n = len(table)
        w, h = o.output_image_dimensions
        handle = scene.upload(o.device_id)
        opt = make_options(w, h, o.samples, o.max_ray_depth, o.seed_mode, o.traversal, flags, cull_margin=o.cull_margin, shading=o.shading)
        hdr = np.zeros((n, h, w, 3), dtype=np.float32) if want_hdr else None
        rgba = np.zeros((n, h, w, 4), dtype=np.uint8) if want_rgba8 else None
        st = L.MiptStats()
        rc = L.load().mipt_render_batch(handle, L.ptr(table), n, C.byref(opt),
                                        L.ptr(hdr) if want_hdr else None, L.ptr(rgba) if want_rgba8 else None, C.byref(st))
        L.check(rc, "mipt_render_batch")
        self.last_stats = st.as_dict()
        return hdr, rgba, self.last_stats

    def render_features(self, scene: Scene, cameras=None, features=("depth", "normal", "albedo"), device: bool = False, stream=None,
                        flags: int = 0, handle=None):
        """First-hit feature buffers (mipt_render_features / _device): per pixel what the camera ray hits and what the surface looks
        like there, with this renderer's width, height, samples, seed mode and traversal.  ``cameras``: a sequence of Camera (or CAMERA
        records), None = the scene's camera.  ``features``: names out of depth, prim, material, position, uv, normal, albedo, emission;
        only these are computed.  Returns ({name: array}, stats): numpy arrays [V,H,W] or [V,H,W,k] (depth / position / uv / normal /
        albedo / emission float32, prim / material uint32 -- prim as MiptHit.prim: bit 31 = front face, HIT_NONE = miss), or with
        ``device=True`` torch tensors of the same shapes on the scene's device (prim / material int32, the same bits), written on
        ``stream`` (a torch stream, a raw hipStream_t or None = torch's current stream).  ``handle``: another resident handle of the
        scene on ``options.device_id``, e.g. a replica of ``upload_multi``.  A stack overflow leaves the buffers written (stats["stack_overflows"] > 0)."""
        o = self._mi355x()
        known = {name: (k, dt) for name, k, dt in L.FEATURES}
        names = list(features)
        if not names or len(set(names)) != len(names) or any(n not in known for n in names):
            raise ValueError(f"features: expected distinct names out of {', '.join(known)}; got {features!r}")
        table = _camera_table([scene.camera] if cameras is None else list(cameras), "render_features")
        n = len(table)
        w, h = o.output_image_dimensions
        hnd = handle if handle is not None else scene.upload(o.device_id)
        opt = make_options(w, h, o.samples, o.max_ray_depth, o.seed_mode, o.traversal, flags, cull_margin=o.cull_margin, shading=o.shading)
        bufs, out = L.MiptFeatureBuffers(), {}
        st = L.MiptStats()
        lib = L.load()
        if device:
            import torch
            dev = torch.device("cuda", o.device_id)
            for name in names:
                k, dt = known[name]
                out[name] = torch.empty((n, h, w) + ((k,) if k > 1 else ()), dtype=torch.float32 if dt is np.float32 else torch.int32, device=dev)
            _fill(bufs, **out)
            f = lib.mipt_render_features_device
            rc = f(hnd, L.ptr(table), n, C.byref(opt), C.byref(bufs), _stream_arg(stream, dev), C.byref(st))
        else:
            for name in names:
                k, dt = known[name]
                out[name] = np.zeros((n, h, w) + ((k,) if k > 1 else ()), dtype=dt)
            _fill(bufs, **out)
            f = lib.mipt_render_features
            rc = f(hnd, L.ptr(table), n, C.byref(opt), C.byref(bufs), C.byref(st))
        return out, self._traced(rc, f, st)

    def render_motion(self, scene: Scene, cameras=None, prev_tris=None, device: bool = False, stream=None, handle=None):
        """Previous positions (mipt_render_motion / _device): per pixel the world position that the first hit's surface point had in
        the previous geometry, with this renderer's width, height, seed mode and traversal -- what ``temporal`` takes as ``position``
        when parts move.  ``prev_tris``: the previous frame's TRIANGLE array in the caller's order (a numpy array; with ``device=True``
        a numpy array, which is copied to the device, a contiguous uint8 / float32 tensor of it or a raw device pointer), None = the
        generation the scene tracks (``Scene.track_motion``).  ``cameras``, ``device``, ``stream`` and ``handle`` as in
        ``render_features``.  Returns ([V,H,W,3] float32 array or tensor, stats)."""
        o = self._mi355x()
        table = _camera_table([scene.camera] if cameras is None else list(cameras), "render_motion")
        n = len(table)
        w, h = o.output_image_dimensions
        keep = None
        if prev_tris is not None and not isinstance(prev_tris, int) and not Scene._is_torch(prev_tris):
            keep = np.ascontiguousarray(prev_tris)
            if keep.dtype != L.TRIANGLE or keep.ndim != 1:
                raise ValueError(f"prev_tris: expected a 1-d TRIANGLE array; got {keep.dtype} of shape {keep.shape}")
        elif Scene._is_torch(prev_tris) and not device:
            raise ValueError("prev_tris: a tensor needs device=True")
        elif isinstance(prev_tris, int) and not device:
            raise ValueError("prev_tris: a raw device pointer needs device=True")
        hnd = handle if handle is not None else scene.upload(o.device_id)
        opt = make_options(w, h, o.samples, o.max_ray_depth, o.seed_mode, o.traversal, 0, cull_margin=o.cull_margin, shading=o.shading)
        bufs, st, lib = L.MiptMotionBuffers(), L.MiptStats(), L.load()
        if device:
            import torch
            dev = torch.device("cuda", o.device_id)
            if keep is not None:
                keep = torch.from_numpy(keep.view(np.uint8).copy()).to(dev)
                bufs.prev_tris, bufs.n_prev_tris = keep.data_ptr(), keep.numel() // L.TRIANGLE.itemsize
            elif isinstance(prev_tris, int):
                bufs.prev_tris, bufs.n_prev_tris = prev_tris, scene.info(hnd)["n_tris"]       # a bare pointer: the scene's count
            elif prev_tris is not None:
                if not prev_tris.is_cuda or not prev_tris.is_contiguous() or (prev_tris.numel() * prev_tris.element_size()) % L.TRIANGLE.itemsize:
                    raise ValueError("prev_tris: expected a contiguous device tensor holding whole TRIANGLE records")
                keep = prev_tris
                bufs.prev_tris, bufs.n_prev_tris = keep.data_ptr(), keep.numel() * keep.element_size() // L.TRIANGLE.itemsize
            out = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
            bufs.prev_position = out.data_ptr()
            stream = _stream_arg(stream, dev)
            if keep is not None and stream != torch.cuda.current_stream(dev).cuda_stream:
                torch.cuda.current_stream(dev).synchronize()      # the copy above ran on torch's stream
            f = lib.mipt_render_motion_device
            rc = f(hnd, L.ptr(table), n, C.byref(opt), C.byref(bufs), stream, C.byref(st))
        else:
            if keep is not None:
                bufs.prev_tris, bufs.n_prev_tris = keep.ctypes.data, len(keep)
            out = np.zeros((n, h, w, 3), dtype=np.float32)
            bufs.prev_position = out.ctypes.data
            f = lib.mipt_render_motion
            rc = f(hnd, L.ptr(table), n, C.byref(opt), C.byref(bufs), C.byref(st))
        return out, self._traced(rc, f, st)

    # -- a-trous denoiser (include/mipt.h "a-trous denoiser") ------------------------------------
    @staticmethod
    def _denoise_planes(hdr, normal, depth, albedo):
        """-> (torch?, (V, H, W), {name: contiguous float32 array or tensor}); ValueError naming the argument for anything else."""
        if not _is_torch(hdr):
            hdr = np.asarray(hdr)
        if hdr.ndim not in (3, 4) or hdr.shape[-1] != 3:
            raise ValueError(f"hdr: expected shape [V,H,W,3] or [H,W,3]; got {tuple(hdr.shape)}")
        lead = tuple(hdr.shape[:-1])
        torch_in, planes = _check_planes("hdr", hdr, "hdr and the guides", [
            ("hdr", hdr, lead + (3,), False), ("normal", normal, lead + (3,), False), ("depth", depth, lead, False),
            ("albedo", albedo, lead + (3,), False)])
        return torch_in, _views(lead), planes

    def denoise(self, hdr, normal=None, depth=None, albedo=None, iterations: int = 5, sigma_color: float = 4.0, sigma_normal: float = 0.5,
                sigma_depth: float = 0.5, stream=None):
        """The edge-avoiding a-trous filter of include/mipt.h over a frame or a batch of views: ``hdr`` [V,H,W,3] or [H,W,3] float32,
        the optional guides ``normal`` [..,3], ``depth`` [..] and ``albedo`` [..,3] of the same leading shape (None = the term is left
        out; with ``albedo`` the frame is demodulated before and re-modulated after).  numpy arrays go through mipt_denoise on
        ``options.device_id``; contiguous torch tensors through mipt_denoise_device on ``stream`` (a torch stream, a raw hipStream_t or None =
        torch's current stream) without blocking, with a torch tensor as the workspace.  Returns a new array / tensor of ``hdr``'s
        kind and shape."""
        torch_in, (v, h, w), p = self._denoise_planes(hdr, normal, depth, albedo)
        opt = L.MiptDenoiseOptions()
        opt.width, opt.height, opt.n_views, opt.iterations = w, h, v, iterations
        opt.sigma_color, opt.sigma_normal, opt.sigma_depth = sigma_color, sigma_normal, sigma_depth
        bufs = L.MiptDenoiseBuffers()
        lib = L.load()
        if torch_in:
            import torch
            out = torch.empty_like(p["hdr"])
            touched = _fill(bufs, out=out, **p)
            raw, ws = _stream_ordered(out.device, stream, touched, lib.mipt_denoise_workspace_bytes(w, h, v))
            L.check(lib.mipt_denoise_device(C.byref(opt), C.byref(bufs), ws.data_ptr(), ws.numel() * 4, raw), "mipt_denoise_device")
            return out
        out = np.empty_like(p["hdr"])
        _fill(bufs, out=out, **p)
        L.check(lib.mipt_denoise(C.byref(opt), C.byref(bufs), self.options.device_id), "mipt_denoise")
        return out

    # -- variance-guided a-trous filter (include/mipt.h "variance-guided a-trous filter") -----------
    def denoise_variance(self, hdr, variance=None, length=None, normal=None, depth=None, albedo=None, iterations: int = 5,
                         sigma_luminance: float = 16.0, sigma_normal: float = 0.5, sigma_depth: float = 0.5, short_history: float = 4.0,
                         want_variance: bool = False, stream=None):
        """The variance-guided a-trous filter of include/mipt.h over a frame or a batch of views: ``hdr`` [V,H,W,3] or [H,W,3] float32
        (the accumulated frame of ``temporal``), ``variance`` and ``length`` [..] as ``temporal`` returns them (both or neither;
        neither = a single frame without history) and the optional guides of ``denoise``.  numpy arrays go through
        mipt_denoise_variance on ``options.device_id``; contiguous torch tensors through mipt_denoise_variance_device on ``stream``
        (a torch stream, a raw hipStream_t or None = torch's current stream) without blocking, with a torch tensor as the workspace.
        Returns a new array / tensor of ``hdr``'s kind and shape, or with ``want_variance`` the pair (out, variance_out [..])."""
        torch_in, (v, h, w), p = self._denoise_planes(hdr, normal, depth, albedo)
        lead = tuple(p["hdr"].shape[:-1])
        p.update(_check_planes("hdr", p["hdr"], "hdr, the guides, variance and length",
                               [("variance", variance, lead, False), ("length", length, lead, False)])[1])
        opt = L.MiptVarianceOptions()
        opt.width, opt.height, opt.n_views, opt.iterations = w, h, v, iterations
        opt.sigma_luminance, opt.sigma_normal, opt.sigma_depth, opt.short_history = sigma_luminance, sigma_normal, sigma_depth, short_history
        bufs = L.MiptVarianceBuffers()
        lib = L.load()
        if torch_in:
            import torch
            out = torch.empty_like(p["hdr"])
            var_out = torch.empty(lead, dtype=torch.float32, device=out.device) if want_variance else None
            touched = _fill(bufs, out=out, variance_out=var_out, **p)
            raw, ws = _stream_ordered(out.device, stream, touched, lib.mipt_denoise_variance_workspace_bytes(w, h, v))
            L.check(lib.mipt_denoise_variance_device(C.byref(opt), C.byref(bufs), ws.data_ptr(), ws.numel() * 4, raw),
                    "mipt_denoise_variance_device")
        else:
            out = np.empty_like(p["hdr"])
            var_out = np.zeros(lead, dtype=np.float32) if want_variance else None
            _fill(bufs, out=out, variance_out=var_out, **p)
            L.check(lib.mipt_denoise_variance(C.byref(opt), C.byref(bufs), self.options.device_id), "mipt_denoise_variance")
        return (out, var_out) if want_variance else out

    # -- guided upsampling (include/mipt.h "guided upsampling") ---------------------------------------
    _UPSAMPLE_GUIDES = (("normal", 3), ("depth", 1), ("albedo", 3), ("material", 1))

    @staticmethod
    def _upsample_planes(lo_hdr, lo_guides, guides, scale):
        """-> (torch?, (V, H, W), {buffer field: contiguous array or tensor}); ValueError naming the argument for anything else."""
        if not _is_torch(lo_hdr):
            lo_hdr = np.asarray(lo_hdr)
        if lo_hdr.ndim not in (3, 4) or lo_hdr.shape[-1] != 3:
            raise ValueError(f"lo_hdr: expected shape [V,h,w,3] or [h,w,3]; got {tuple(lo_hdr.shape)}")
        if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or not 2 <= scale <= 8:
            raise ValueError(f"scale: expected an integer 2 ... 8; got {scale!r}")
        for name, g in (("lo_guides", lo_guides), ("guides", guides)):
            if g is not None and not isinstance(g, dict):
                raise ValueError(f"{name}: expected a dict with any of normal, depth, albedo, material, or None")
        lo_guides, guides = lo_guides or {}, guides or {}
        lo_lead = tuple(lo_hdr.shape[:-1])
        lead = lo_lead[:-2] + (lo_lead[-2] * scale, lo_lead[-1] * scale)
        table = [("lo_hdr", lo_hdr, lo_lead + (3,), False)]
        for name, k in Renderer._UPSAMPLE_GUIDES:
            lo, hi = lo_guides.get(name), guides.get(name)
            if (lo is None) != (hi is None):
                where = "guides" if lo is None else "lo_guides"
                raise ValueError(f"{'lo_' + name if lo is None else name}: {name} is given at both resolutions or at neither; only {where} holds it")
            if lo is not None:
                last = (k,) if k > 1 else ()
                table += [("lo_" + name, lo, lo_lead + last, name == "material"), (name, hi, lead + last, name == "material")]
        torch_in, planes = _check_planes("lo_hdr", lo_hdr, "lo_hdr and the guides", table)
        return torch_in, _views(lead), lead, planes

    def upsample(self, lo_hdr, lo_guides, guides, scale, sigma_normal: float = 0.5, sigma_depth: float = 0.5, want_weight: bool = False,
                 stream=None):
        """The guided upsampling of include/mipt.h over a frame or a batch of views: ``lo_hdr`` [V,h,w,3] or [h,w,3] float32, the
        frame traced (and filtered) at 1/``scale`` of the resolution, comes back at [..,h*scale,w*scale,3].  ``lo_guides`` and
        ``guides``: dicts as ``render_features`` returns them at the low and at the full resolution; the keys used are ``normal``
        [..,3], ``depth`` [..], ``albedo`` [..,3] float32 and ``material`` [..] (uint32 arrays / int32 tensors, the same bits), each
        in both dicts or in neither (None = no guides); other keys are ignored.  numpy arrays go through mipt_upsample on
        ``options.device_id``; contiguous torch tensors through mipt_upsample_device on ``stream`` (a torch stream, a raw hipStream_t
        or None = torch's current stream) without blocking, with a torch tensor as the workspace.  Returns a new array / tensor of
        ``lo_hdr``'s kind, or with ``want_weight`` the pair (out, weight [..,h*scale,w*scale]): the sum of the accepted taps'
        weights, 0 where a pixel fell back to plain bilinear."""
        torch_in, (v, h, w), lead, p = self._upsample_planes(lo_hdr, lo_guides, guides, scale)
        opt = L.MiptUpsampleOptions()
        opt.width, opt.height, opt.n_views, opt.scale = w, h, v, int(scale)
        opt.sigma_normal, opt.sigma_depth = sigma_normal, sigma_depth
        bufs = L.MiptUpsampleBuffers()
        lib = L.load()
        if torch_in:
            import torch
            dev = p["lo_hdr"].device
            out = torch.empty(lead + (3,), dtype=torch.float32, device=dev)
            weight = torch.empty(lead, dtype=torch.float32, device=dev) if want_weight else None
            touched = _fill(bufs, out=out, weight=weight, **p)
            raw, ws = _stream_ordered(dev, stream, touched, lib.mipt_upsample_workspace_bytes(w, h, v, int(scale)))
            L.check(lib.mipt_upsample_device(C.byref(opt), C.byref(bufs), ws.data_ptr(), ws.numel() * 4, raw), "mipt_upsample_device")
        else:
            out = np.empty(lead + (3,), dtype=np.float32)
            weight = np.zeros(lead, dtype=np.float32) if want_weight else None
            _fill(bufs, out=out, weight=weight, **p)
            L.check(lib.mipt_upsample(C.byref(opt), C.byref(bufs), self.options.device_id), "mipt_upsample")
        return (out, weight) if want_weight else out

    _FULL_FEATURES = ("depth", "normal", "albedo", "material")

    def _low_resolution(self, upsample, who):
        """the renderer that traces at 1/upsample of this one's output_image_dimensions; ValueError unless they are multiples of it"""
        w, h = self.options.output_image_dimensions
        if isinstance(upsample, bool) or not isinstance(upsample, (int, np.integer)) or not 2 <= upsample <= 8:
            raise ValueError(f"{who}: upsample must be None or an integer 2 ... 8; got {upsample!r}")
        if w % upsample or h % upsample:
            raise ValueError(f"{who}: output_image_dimensions {w}x{h} are not multiples of upsample={upsample}")
        return Renderer(RendererOptions(**{**self.options.__dict__, "output_image_dimensions": (w // upsample, h // upsample)}))

    def render_denoised(self, scene: Scene, cameras=None, variance: bool = False, upsample=None, **denoise_args):
        """Render, guides and filter on one stream with nothing crossing PCIe in between: mipt_render_batch_device with this renderer's
        options, mipt_render_features_device for depth, normal and albedo (one sample, this renderer's seed mode) and
        mipt_denoise_device (``denoise_args``: iterations, the sigmas, stream).  ``variance=True`` filters with
        mipt_denoise_variance_device instead, as a single frame without history (``denoise_args``: iterations, sigma_luminance,
        sigma_normal, sigma_depth, short_history, stream).  ``cameras``: a sequence of Camera (or CAMERA records), None = the scene's
        camera.  Returns (denoised, noisy, features, stats): float32 tensors [V,H,W,3] on ``options.device_id``, the feature dict of
        ``render_features`` and the stats of the render launch.  ``upsample=k`` (2 ... 8; ``output_image_dimensions`` must be
        multiples of it) traces, takes the guides (material as well) and filters at (W/k, H/k) exactly as above, then runs one
        full-resolution feature pass (depth, normal, albedo, material; one sample; the same cameras) and mipt_upsample_device on the
        same stream (``denoise_args`` may hold upsample_sigma_normal and upsample_sigma_depth).  It returns (full, denoised, noisy,
        features, features_full, stats): ``full`` [V,H,W,3] and the dict ``features_full`` at ``output_image_dimensions``, the other
        four as above at (W/k, H/k)."""
        import torch
        o = self._mi355x()
        if upsample is not None:
            low = self._low_resolution(upsample, "render_denoised")
            u_args = {k[len("upsample_"):]: denoise_args.pop(k) for k in ("upsample_sigma_normal", "upsample_sigma_depth") if k in denoise_args}
            raw = denoise_args["stream"] = _stream_arg(denoise_args.get("stream"), torch.device("cuda", o.device_id))
            denoised, noisy, features, stats = low._render_denoised_low(scene, cameras, variance, ("depth", "normal", "albedo", "material"), denoise_args)
            cams = [scene.camera] if cameras is None else list(cameras)
            one = Renderer(RendererOptions(**{**o.__dict__, "samples": 1}))
            features_full, _ = one.render_features(scene, cams, self._FULL_FEATURES, device=True, stream=raw)
            full = self.upsample(denoised, features, features_full, upsample, stream=raw, **u_args)
            self.last_stats = stats
            return full, denoised, noisy, features, features_full, stats
        return self._render_denoised_low(scene, cameras, variance, ("depth", "normal", "albedo"), denoise_args)

    def _render_denoised_low(self, scene, cameras, variance, names, denoise_args):
        """render_denoised at this renderer's own size, with the feature planes `names`"""
        import torch
        o = self.options
        cams = [scene.camera] if cameras is None else list(cameras)
        table = _camera_table(cams, "render_denoised")
        n = len(cams)
        w, h = o.output_image_dimensions
        dev = torch.device("cuda", o.device_id)
        raw = _stream_arg(denoise_args.pop("stream", None), dev)
        handle = scene.upload(o.device_id)
        opt = make_options(w, h, o.samples, o.max_ray_depth, o.seed_mode, o.traversal, cull_margin=o.cull_margin, shading=o.shading)
        noisy = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
        st = L.MiptStats()
        L.check(L.load().mipt_render_batch_device(handle, L.ptr(table), n, C.byref(opt), noisy.data_ptr(), None, raw, C.byref(st)),
                "mipt_render_batch_device")
        stats = st.as_dict()
        one = Renderer(RendererOptions(**{**o.__dict__, "samples": 1}))
        features, _ = one.render_features(scene, cams, names, device=True, stream=raw, handle=handle)
        if variance:
            denoised = self.denoise_variance(noisy, None, None, features["normal"], features["depth"], features["albedo"], stream=raw, **denoise_args)
        else:
            denoised = self.denoise(noisy, features["normal"], features["depth"], features["albedo"], stream=raw, **denoise_args)
        self.last_stats = stats
        return denoised, noisy, features, stats

    # -- adaptive sampling (include/mipt.h "adaptive sampling") -------------------------------------
    def render_adaptive(self, scene: Scene, counts, cameras=None, flags: int = 0, sample_begin: int = 0, want_rgba8: bool = False,
                        stream=None, handle=None, out=None):
        """A batch render with a count plane (mipt_render_adaptive / _device): pixel p of view v is traced with
        min(counts[v, p], options.samples) samples -- ``options.samples`` is the cap -- and holds exactly what ``render_buffers``
        gives for that camera with that many samples; a pixel with 0 is not traced and holds 0.  ``counts``: [V,H,W] or [H,W], a
        uint32 numpy array (host entry) or a contiguous int32 tensor on ``options.device_id`` (the same bits; device entry, on
        ``stream``: a torch stream, a raw hipStream_t or None = torch's current stream).  ``cameras``: a sequence of Camera (or CAMERA
        records), None = the scene's camera.  ``flags``: FLAG_COUNT, FLAG_SUM and, with tensors and ``out``, FLAG_ACCUM.  ``out``: a
        float32 tensor [V,H,W,3] to write (to add to, under FLAG_ACCUM) instead of a new one.  ``handle`` as in ``render_features``.
        Returns (hdr [V,H,W,3] float32, rgba8 [V,H,W,4] uint8 | None, stats) as numpy arrays or tensors, after ``counts``' kind."""
        o = self._mi355x()
        table = _camera_table([scene.camera] if cameras is None else list(cameras), "render_adaptive")
        n = len(table)
        w, h = o.output_image_dimensions
        torch_in = _is_torch(counts)
        if not torch_in:
            counts = np.asarray(counts)
        if tuple(counts.shape) not in ((n, h, w), (h, w)) or (counts.ndim == 2 and n != 1):
            raise ValueError(f"counts: expected shape {(n, h, w)}; got {tuple(counts.shape)}")
        hnd = handle if handle is not None else scene.upload(o.device_id)
        opt = make_options(w, h, o.samples, o.max_ray_depth, o.seed_mode, o.traversal, flags, sample_begin=sample_begin,
                           cull_margin=o.cull_margin, shading=o.shading)
        st, lib = L.MiptStats(), L.load()
        if torch_in:
            import torch
            dev = torch.device("cuda", o.device_id)
            if counts.dtype != torch.int32 or not counts.is_cuda or counts.device != dev or not counts.is_contiguous():
                raise ValueError(f"counts: expected a contiguous int32 tensor on {dev}")
            if out is None:
                out = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
            elif not (Scene._is_torch(out) and out.dtype == torch.float32 and out.is_cuda and out.device == dev and out.is_contiguous()
                      and tuple(out.shape) == (n, h, w, 3)):
                raise ValueError(f"out: expected a contiguous float32 tensor of shape {(n, h, w, 3)} on {dev}")
            rgba = torch.empty((n, h, w, 4), dtype=torch.uint8, device=dev) if want_rgba8 else None
            f, hdr = lib.mipt_render_adaptive_device, out
            rc = f(hnd, L.ptr(table), n, C.byref(opt), counts.data_ptr(), out.data_ptr(), rgba.data_ptr() if want_rgba8 else None,
                   _stream_arg(stream, dev), C.byref(st))
        else:
            if out is not None:
                raise ValueError("out: a tensor to write needs counts as a tensor")
            if counts.dtype != np.uint32:
                raise ValueError(f"counts: expected uint32; got {counts.dtype}")
            counts = np.ascontiguousarray(counts)
            hdr = np.zeros((n, h, w, 3), dtype=np.float32)
            rgba = np.zeros((n, h, w, 4), dtype=np.uint8) if want_rgba8 else None
            f = lib.mipt_render_adaptive
            rc = f(hnd, L.ptr(table), n, C.byref(opt), L.ptr(counts), L.ptr(hdr), L.ptr(rgba) if want_rgba8 else None, C.byref(st))
        return hdr, rgba, self._traced(rc, f, st)

    def sample_map(self, variance, hdr=None, albedo=None, min_samples: int = 1, max_samples=None, budget=None, stream=None, rounds=None):
        """The sample map of include/mipt.h: a variance plane [V,H,W] or [H,W] float32 -- ``variance_out`` of ``denoise_variance``, or
        ``variance`` of ``temporal`` -- becomes a count plane of the same shape for ``render_adaptive``, every count in
        [min_samples, max_samples] and their mean at most ``budget``.  ``hdr`` [..,3] makes the weight the standard deviation
        relative to the frame's luminance, ``albedo`` [..,3] (only with ``hdr``) demodulates the frame first.  ``max_samples``
        defaults to ``options.samples``, ``budget`` to ``min_samples``.  numpy arrays go through mipt_sample_map on
        ``options.device_id`` and give a uint32 array; contiguous torch tensors through mipt_sample_map_device on ``stream`` (a torch
        stream, a raw hipStream_t or None = torch's current stream) without blocking and give an int32 tensor (the same bits).
        ``rounds`` (1 ... 8; None = the plain map) goes through mipt_sample_map_fill / _device instead: what the clamp at
        ``max_samples`` cuts off is handed on to the pixels below it, ``rounds`` - 1 times; ``rounds=1`` gives the plain map's counts."""
        if not _is_torch(variance):
            variance = np.asarray(variance)
        if variance.ndim not in (2, 3):
            raise ValueError(f"variance: expected shape [V,H,W] or [H,W]; got {tuple(variance.shape)}")
        if albedo is not None and hdr is None:
            raise ValueError("albedo: given only with hdr")
        lead = tuple(variance.shape)
        v, h, w = _views(lead)
        torch_in, p = _check_planes("variance", variance, "variance, hdr and albedo", [
            ("variance", variance, lead, False), ("hdr", hdr, lead + (3,), False), ("albedo", albedo, lead + (3,), False)])
        opt = L.MiptSampleMapOptions() if rounds is None else L.MiptSampleMapFillOptions()
        if rounds is not None:
            opt.rounds = rounds
        opt.width, opt.height, opt.n_views = w, h, v
        opt.min_samples = min_samples
        opt.max_samples = self.options.samples if max_samples is None else max_samples
        opt.budget = float(min_samples if budget is None else budget)
        bufs, lib = L.MiptSampleMapBuffers(), L.load()
        if torch_in:
            import torch
            counts = torch.empty(lead, dtype=torch.int32, device=variance.device)
            touched = _fill(bufs, counts=counts, **p)
            need = lib.mipt_sample_map_workspace_bytes(w, h, v) if rounds is None else lib.mipt_sample_map_fill_workspace_bytes(w, h, v, rounds)
            raw, ws = _stream_ordered(variance.device, stream, touched, need)
            if rounds is None:
                L.check(lib.mipt_sample_map_device(C.byref(opt), C.byref(bufs), ws.data_ptr(), raw), "mipt_sample_map_device")
            else:
                L.check(lib.mipt_sample_map_fill_device(C.byref(opt), C.byref(bufs), ws.data_ptr(), raw), "mipt_sample_map_fill_device")
            return counts
        counts = np.zeros(lead, dtype=np.uint32)
        _fill(bufs, counts=counts, **p)
        if rounds is None:
            L.check(lib.mipt_sample_map(C.byref(opt), C.byref(bufs), self.options.device_id), "mipt_sample_map")
        else:
            L.check(lib.mipt_sample_map_fill(C.byref(opt), C.byref(bufs), self.options.device_id), "mipt_sample_map_fill")
        return counts

    # -- temporal accumulation (include/mipt.h "temporal accumulation") ---------------------------
    _TEMPORAL_PLANES = (("position", 3, True), ("normal", 3, True), ("depth", 1, True), ("material", 1, True), ("albedo", 3, False))

    @staticmethod
    def _temporal_planes(hdr, features):
        """-> (torch?, (V, H, W), {name: contiguous array or tensor}); ValueError naming the argument for anything else."""
        if not _is_torch(hdr):
            hdr = np.asarray(hdr)
        if hdr.ndim not in (3, 4) or hdr.shape[-1] != 3:
            raise ValueError(f"hdr: expected shape [V,H,W,3] or [H,W,3]; got {tuple(hdr.shape)}")
        if not isinstance(features, dict):
            raise ValueError("features: expected a dict with position, normal, depth, material and optionally albedo")
        lead = tuple(hdr.shape[:-1])
        table = [("hdr", hdr, lead + (3,), False)]
        table += [(name, features.get(name), lead + ((k,) if k > 1 else ()), name == "material") for name, k, _ in Renderer._TEMPORAL_PLANES]
        torch_in, planes = _check_planes("hdr", hdr, "hdr and the features", table,
                                         required=[name for name, _, must in Renderer._TEMPORAL_PLANES if must],
                                         missing="features must hold it (render_features with position, normal, depth, material)")
        return torch_in, _views(lead), planes

    def temporal(self, hdr, features, cameras, history=None, alpha_min: float = 0.0, max_history: float = 32.0, normal_tol: float = 0.1,
                 depth_tol: float = 0.1, want_length: bool = False, want_variance: bool = False, stream=None, history_out=None,
                 counts=None, samples_cap=None):
        """The temporal accumulation of include/mipt.h over a frame or a batch of views: ``hdr`` [V,H,W,3] or [H,W,3] float32 is blended
        with the previous frame's ``history`` reprojected through the camera it carries.  ``features``: a dict with ``position``
        [..,3], ``normal`` [..,3], ``depth`` [..] float32 and ``material`` [..] (uint32 arrays / int32 tensors, the same bits) of the
        same leading shape -- what ``render_features`` returns -- and optionally ``albedo`` [..,3] (the frame is demodulated before
        and re-modulated after).  ``cameras``: the V Camera (or CAMERA records) that produced this frame.  ``history``: what the last
        call returned, None = the first frame.  numpy arrays go through mipt_temporal on ``options.device_id``; contiguous torch
        tensors through mipt_temporal_device on ``stream`` (a torch stream, a raw hipStream_t or None = torch's current stream)
        without blocking.  ``history_out``: an int32 tensor of mipt_temporal_history_bytes() to write instead of a new one (it must
        not be ``history``).  Returns (out, history, extras): ``out`` of ``hdr``'s kind and shape, the new history (a flat uint32
        array / int32 tensor in the header's layout) and a dict with ``length`` and ``variance`` [..] where asked for.
        ``counts`` [..] (a uint32 array with arrays, a contiguous int32 tensor with tensors: the plane ``render_adaptive`` was given
        for this frame) goes through mipt_temporal_counts / _device instead: the history length counts samples, a pixel with n
        samples is blended in with the weight n, one with 0 is reprojected only, and ``max_history`` is then a number of samples.
        ``samples_cap`` is that render's cap and defaults to ``options.samples``."""
        torch_in, (v, h, w), p = self._temporal_planes(hdr, features)
        cams = list(cameras.reshape(-1)) if isinstance(cameras, np.ndarray) else ([cameras] if isinstance(cameras, Camera) else list(cameras))
        if len(cams) != v:
            raise ValueError(f"cameras: expected {v} cameras, one per view; got {len(cams)}")
        table = _camera_table(cams)
        opt = L.MiptTemporalOptions()
        opt.width, opt.height, opt.n_views = w, h, v
        opt.alpha_min, opt.max_history, opt.normal_tol, opt.depth_tol = alpha_min, max_history, normal_tol, depth_tol
        bufs = L.MiptTemporalBuffers()
        lib = L.load()
        words = max(int(lib.mipt_temporal_history_bytes(w, h, v)), 16) // 4          # an impossible size is left to the library to refuse
        lead = tuple(p["hdr"].shape[:-1])
        want = (("length", want_length), ("variance", want_variance))
        if counts is None:
            if samples_cap is not None:
                raise ValueError("samples_cap: given only with counts")
        else:
            samples_cap = self.options.samples if samples_cap is None else samples_cap
            if _is_torch(counts) != torch_in:
                raise ValueError("counts: hdr and counts must both be numpy arrays or both torch tensors")
            if not torch_in:
                counts = np.asarray(counts)
                if counts.dtype != np.uint32:
                    raise ValueError(f"counts: expected uint32; got {counts.dtype}")
                counts = np.ascontiguousarray(counts)
            if tuple(counts.shape) != lead:
                raise ValueError(f"counts: expected shape {lead}; got {tuple(counts.shape)}")
        if torch_in:
            import torch
            dev = p["hdr"].device
            if counts is not None and (counts.dtype != torch.int32 or not counts.is_cuda or counts.device != dev or not counts.is_contiguous()):
                raise ValueError(f"counts: expected a contiguous int32 tensor on hdr's device {dev}")
            for name, t in (("history", history), ("history_out", history_out)):
                if t is not None and not (Scene._is_torch(t) and t.dtype == torch.int32 and t.is_cuda and t.device == dev and t.is_contiguous()
                                          and t.numel() == words):
                    raise ValueError(f"{name}: expected a contiguous int32 tensor of {words} words on hdr's device {dev}")
            out = torch.empty_like(p["hdr"])
            new = history_out if history_out is not None else torch.empty((words,), dtype=torch.int32, device=dev)
            extras = {name: torch.empty(lead, dtype=torch.float32, device=dev) for name, on in want if on}
            touched = _fill(bufs, out=out, history_in=history, history_out=new, **p, **extras)
            raw, _ = _stream_ordered(dev, stream, touched + [counts])
            if counts is None:
                L.check(lib.mipt_temporal_device(C.byref(opt), L.ptr(table), C.byref(bufs), raw), "mipt_temporal_device")
            else:
                L.check(lib.mipt_temporal_counts_device(C.byref(opt), L.ptr(table), C.byref(bufs), counts.data_ptr(), samples_cap, raw),
                        "mipt_temporal_counts_device")
            return out, new, extras
        if history is not None:
            history = np.ascontiguousarray(history)
            if history.dtype != np.uint32 or history.size != words:
                raise ValueError(f"history: expected a uint32 array of {words} words; got {history.dtype} of {history.size}")
        out = np.empty_like(p["hdr"])
        new = np.zeros(words, dtype=np.uint32)
        extras = {name: np.zeros(lead, dtype=np.float32) for name, on in want if on}
        _fill(bufs, out=out, history_in=history, history_out=new, **p, **extras)
        if counts is None:
            L.check(lib.mipt_temporal(C.byref(opt), L.ptr(table), C.byref(bufs), self.options.device_id), "mipt_temporal")
        else:
            L.check(lib.mipt_temporal_counts(C.byref(opt), L.ptr(table), C.byref(bufs), counts.ctypes.data, samples_cap, self.options.device_id),
                    "mipt_temporal_counts")
        return out, new, extras

    def render_sequence(self, scene: Scene, cameras_per_frame, denoise: bool = True, motion: bool = False, upsample=None, adaptive=None, **args):
        """A camera path without flicker, nothing crossing PCIe in between: a generator that per frame runs mipt_render_batch_device
        with this renderer's options, mipt_render_features_device (depth, normal, albedo, position, material; one sample),
        mipt_temporal_device and, with ``denoise``, mipt_denoise_device on one stream, the history in two tensors that swap roles.
        ``cameras_per_frame``: per frame a Camera (or CAMERA record) or a sequence of them, one per view; every frame has the same
        number of views.  ``args``: alpha_min, max_history, normal_tol, depth_tol (temporal), iterations, sigma_color, sigma_normal,
        sigma_depth (denoise), stream.  ``denoise="variance"`` runs mipt_denoise_variance_device in mipt_denoise_device's place, fed
        with the temporal step's ``length`` and ``variance`` on the same stream; its ``args`` are iterations, sigma_luminance,
        sigma_normal, sigma_depth and short_history.  The renderer must use SEED_PER_SAMPLE -- the pixel stream repeats the same noise every frame,
        and averaging it gains nothing: frame f renders the samples from 1 + f * samples on.  Yields per frame a dict with ``out``
        (the denoised frame, or the accumulated one), ``accumulated``, ``noisy`` [V,H,W,3], ``features``, ``history`` (valid until the
        frame after the next is produced: the two tensors are reused), ``length``, ``variance`` and ``stats``.  ``motion=True`` is for
        parts that move: the scene must be a resident mesh that tracks motion (``Scene.track_motion``), the caller moves its parts
        with ``scene.set_transforms`` / ``update_mesh_device`` between two ``next()`` calls (at most one update per frame), and each
        frame also runs mipt_render_motion_device with the options of its feature pass, hands that plane to the temporal step as
        ``position`` and yields it as ``prev_position``; ``features["position"]`` stays the current one.  ``upsample=k`` (2 ... 8;
        ``output_image_dimensions`` must be multiples of it): the trace, the feature and motion passes, the temporal step with its
        histories and the filter all run at (W/k, H/k) exactly as above, then one full-resolution feature pass (depth, normal, albedo,
        material; one sample; the same cameras) and mipt_upsample_device run on the same stream (``args`` may hold
        upsample_sigma_normal and upsample_sigma_depth).  Every key above keeps its meaning at (W/k, H/k); the dict gains ``out_full``
        [V,H,W,3], ``out`` upsampled to ``output_image_dimensions``, and ``features_full``, the dict of that feature pass.
        ``adaptive=dict(min_samples=..., max_samples=..., budget=...)`` (with ``denoise="variance"`` only) spends the samples where
        the last frame was noisy: the trace is mipt_render_adaptive_device with ``max_samples`` as its cap in
        mipt_render_batch_device's place.  Frame 0 gives every pixel max(1, floor(budget)) samples; frame f > 0 takes its counts from
        mipt_sample_map_device over frame f - 1's ``variance_out`` (the filter's, which is asked for it), with frame f - 1's ``out``
        as hdr and its albedo, on the same stream, and renders the samples from 1 + f * max_samples on, so that no pixel ever reuses a
        sample number.  The map is used at the same pixel, it is NOT reprojected: a fast camera smears it by its motion, and the
        pixels it misses still get ``min_samples``.  The dict gains ``counts`` (int32 [V,H,W]) and ``variance_out``; ``stats`` is the
        adaptive launch's.  With ``upsample=k`` all of this happens at (W/k, H/k).  Two optional keys of ``adaptive``:
        ``blend="counts"`` runs mipt_temporal_counts_device in the temporal step's place, with the plane the frame was rendered
        with (frame 0: the uniform one) and ``max_samples`` as the cap -- ``max_history`` is passed through unchanged and is then a
        number of SAMPLES, not of frames; ``rounds=R`` (1 ... 8) makes the map mipt_sample_map_fill_device, which hands on what the
        clamp at ``max_samples`` cuts off.  With neither key the call sequence is the one above, call for call."""
        import torch
        o = self._mi355x()
        if adaptive is not None:
            if denoise != "variance":
                raise ValueError("render_sequence: adaptive needs denoise=\"variance\": the sample map is made from the filter's variance_out")
            if not isinstance(adaptive, dict) or sorted(k for k in adaptive if k not in ("blend", "rounds")) != ["budget", "max_samples", "min_samples"]:
                raise ValueError(f"render_sequence: adaptive must be None or dict(min_samples=, max_samples=, budget=[, blend=\"counts\"][, rounds=]); got {adaptive!r}")
            if adaptive.get("blend", "counts") != "counts":
                raise ValueError(f"render_sequence: adaptive[\"blend\"] must be \"counts\" or absent; got {adaptive['blend']!r}")
        if o.seed_mode != L.SEED_PER_SAMPLE:
            raise ValueError("render_sequence: the renderer's seed_mode must be SEED_PER_SAMPLE; the pixel stream repeats the same noise every frame")
        if motion and (scene.mesh is None or scene._handle is None or not scene._tracks_motion):
            raise ValueError("render_sequence: motion=True needs a resident mesh scene that tracks motion (upload_from_mesh, track_motion)")
        guided = isinstance(denoise, str)
        if guided and denoise != "variance":
            raise ValueError(f"render_sequence: denoise must be True, False or \"variance\"; got {denoise!r}")
        t_names = ("alpha_min", "max_history", "normal_tol", "depth_tol")
        d_names = ("iterations", "sigma_luminance", "sigma_normal", "sigma_depth", "short_history") if guided else ("iterations", "sigma_color", "sigma_normal", "sigma_depth")
        stream = args.pop("stream", None)
        u_args = {}
        if upsample is not None:
            o = self._low_resolution(upsample, "render_sequence").options
            u_args = {k[len("upsample_"):]: args.pop(k) for k in ("upsample_sigma_normal", "upsample_sigma_depth") if k in args}
        unknown = [k for k in args if k not in t_names + d_names]
        if unknown:
            raise ValueError(f"render_sequence: unknown arguments {unknown}")
        t_args, d_args = {k: args[k] for k in t_names if k in args}, {k: args[k] for k in d_names if k in args}
        w, h = o.output_image_dimensions
        dev = torch.device("cuda", o.device_id)
        raw = _stream_arg(stream, dev)
        one = Renderer(RendererOptions(**{**o.__dict__, "samples": 1}))
        one_full = Renderer(RendererOptions(**{**self.options.__dict__, "samples": 1})) if upsample is not None else None
        lib = L.load()
        handle, pair, history, n = None, None, None, None
        capped, counts = None, None
        by_counts, map_args = False, None
        if adaptive is not None:
            by_counts = "blend" in adaptive
            map_args = {k: v for k, v in adaptive.items() if k != "blend"}
            capped = Renderer(RendererOptions(**{**o.__dict__, "samples": adaptive["max_samples"]}))
        for frame, cams in enumerate(cameras_per_frame):
            cams = [cams] if isinstance(cams, (Camera, np.void)) or (isinstance(cams, np.ndarray) and cams.ndim == 0) else list(cams)
            if not cams or (n is not None and len(cams) != n):
                raise ValueError(f"render_sequence: frame {frame} has {len(cams)} cameras; every frame needs the same number, at least 1")
            table = _camera_table(cams)
            if n is None:
                n = len(cams)
                handle = scene.upload(o.device_id)
                words = int(lib.mipt_temporal_history_bytes(w, h, n)) // 4
                pair = [torch.empty((max(words, 4),), dtype=torch.int32, device=dev) for _ in range(2)]
            if adaptive is not None:
                if counts is None:
                    counts = torch.full((n, h, w), max(1, int(adaptive["budget"])), dtype=torch.int32, device=dev)
                    if raw != torch.cuda.current_stream(dev).cuda_stream:
                        torch.cuda.current_stream(dev).synchronize()      # the fill above ran on torch's stream
                noisy, _, stats = capped.render_adaptive(scene, counts, cams, sample_begin=1 + frame * adaptive["max_samples"], stream=raw, handle=handle)
            else:
                opt = make_options(w, h, o.samples, o.max_ray_depth, o.seed_mode, o.traversal, sample_begin=1 + frame * o.samples,
                                   cull_margin=o.cull_margin, shading=o.shading)
                noisy = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
                st = L.MiptStats()
                L.check(lib.mipt_render_batch_device(handle, L.ptr(table), n, C.byref(opt), noisy.data_ptr(), None, raw, C.byref(st)),
                        "mipt_render_batch_device")
                stats = st.as_dict()
            features, _ = one.render_features(scene, cams, ("depth", "normal", "albedo", "position", "material"), device=True, stream=raw, handle=handle)
            t_features, prev_position = features, None
            if motion:
                prev_position, _ = one.render_motion(scene, cams, device=True, stream=raw, handle=handle)
                t_features = {**features, "position": prev_position}
            c_args = dict(counts=counts, samples_cap=adaptive["max_samples"]) if by_counts else {}
            acc, history, extras = self.temporal(noisy, t_features, table, history=history, want_length=True, want_variance=True, stream=raw,
                                                 history_out=pair[frame & 1], **t_args, **c_args)
            variance_out = None
            if adaptive is not None:
                out, variance_out = self.denoise_variance(acc, extras["variance"], extras["length"], features["normal"], features["depth"],
                                                          features["albedo"], want_variance=True, stream=raw, **d_args)
            elif guided:
                out = self.denoise_variance(acc, extras["variance"], extras["length"], features["normal"], features["depth"], features["albedo"],
                                            stream=raw, **d_args)
            else:
                out = self.denoise(acc, features["normal"], features["depth"], features["albedo"], stream=raw, **d_args) if denoise else acc
            self.last_stats = stats
            result = dict(frame=frame, out=out, accumulated=acc, noisy=noisy, features=features, history=history, length=extras["length"],
                          variance=extras["variance"], stats=stats)
            if motion:
                result["prev_position"] = prev_position
            if adaptive is not None:
                result["counts"], result["variance_out"] = counts, variance_out
                counts = self.sample_map(variance_out, out, features["albedo"], stream=raw, **map_args)      # the next frame's
            if upsample is not None:
                result["features_full"], _ = one_full.render_features(scene, cams, self._FULL_FEATURES, device=True, stream=raw, handle=handle)
                result["out_full"] = self.upsample(out, features, result["features_full"], upsample, stream=raw, **u_args)
            yield result

    def render_buffers_multi(self, scene: Scene, mode: int = L.MULTI_TILES, device_ids=None, want_hdr: bool = True,
                             want_rgba8: bool = True, flags: int = 0):
        """The same arm over all GPUs of the node in one call (mipt_render_multi): image tiles + one RCCL gather, or
        sample ranges + one RCCL sum-reduce.  Returns (hdr, rgba8, stats dict)."""
        o = self.options
        w, h = o.output_image_dimensions
        multi = scene.upload_multi(device_ids)
        opt = make_options(w, h, o.samples, o.max_ray_depth, o.seed_mode, o.traversal, flags, cull_margin=o.cull_margin, shading=o.shading)
        hdr = np.zeros((h, w, 3), dtype=np.float32) if want_hdr else None
        rgba = np.zeros((h, w, 4), dtype=np.uint8) if want_rgba8 else None
        st = L.MiptMultiStats()
        rc = L.load().mipt_render_multi(multi, L.ptr(scene.camera.uniform), C.byref(opt), mode,
                                        L.ptr(hdr) if want_hdr else None, L.ptr(rgba) if want_rgba8 else None, C.byref(st))
        L.check(rc, "mipt_render_multi")
        self.last_stats = st.as_dict()
        return hdr, rgba, self.last_stats

    def render(self, scene: Scene) -> bytes:  # renderer.rs:50-85 (offline arm)
        if self.options.is_realtime:
            raise NotImplementedError("the realtime window (gpu/window.rs) is out of scope")
        _, rgba, stats = self.render_buffers(scene, want_hdr=False, want_rgba8=True)
        log_info(f"Rendering took {stats['kernel_ms']:.1f} ms")
        path = self.options.output_image_path
        if path:
            w, h = self.options.output_image_dimensions
            write_ppm(path, rgba[:, :, :3]) if path.endswith(".ppm") else write_png_rgba8(path, rgba)
            log_info(f"Succesfully wrote image data to '{path}'")
        return rgba.tobytes()


def write_ppm(path: str, rgb: np.ndarray) -> None:
    h, w, _ = rgb.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(rgb, dtype=np.uint8).tobytes())


def write_png_rgba16(path: str, rgba16: np.ndarray) -> None:
    """RGBA16 PNG (big-endian samples) -- the format Renderer::render saves (renderer.rs:67-73, ColorType::Rgba16)."""
    import struct
    import zlib
    h, w, _ = rgba16.shape
    be = np.ascontiguousarray(rgba16, dtype=np.uint16).astype(">u2")
    raw = b"".join(b"\x00" + be[y].tobytes() for y in range(h))

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 6, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def write_png_rgba8(path: str, rgba: np.ndarray) -> None:
    """Minimal PNG writer (zlib + CRC from the stdlib).  The reference saves through image::save_buffer
    (renderer.rs:67-73) as Rgba16 -- which cannot hold the CPU path's RGBA8 bytes; this
    writes the RGBA8 pixels the CPU path actually produces."""
    import struct
    import zlib
    h, w, _ = rgba.shape
    raw = b"".join(b"\x00" + np.ascontiguousarray(rgba[y]).tobytes() for y in range(h))

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))
