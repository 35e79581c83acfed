"""CPU: the adaptive-sampling entry points (mipt_render_adaptive, mipt_render_adaptive_device, mipt_sample_map_workspace_bytes,
mipt_sample_map, mipt_sample_map_device) are declared, exported and bound, their structs have the sizes the header states, and every
argument check runs before anything touches a device and names its field."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mipt_render_adaptive", "mipt_render_adaptive_device", "mipt_sample_map_workspace_bytes", "mipt_sample_map", "mipt_sample_map_device")


def test_symbols_declared_exported_and_bound(rrt):
    from rust_ray_tracing_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mipt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mipt_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = rrt.load()
    for s in ENTRIES:
        assert s in declared and s in exported and s in L.EXPORTS, s
        assert getattr(lib, s).argtypes is not None, s
    assert len(lib.mipt_render_adaptive.argtypes) == 8 and len(lib.mipt_render_adaptive_device.argtypes) == 9
    assert len(lib.mipt_sample_map.argtypes) == 3 and len(lib.mipt_sample_map_device.argtypes) == 4
    assert lib.mipt_sample_map_workspace_bytes.restype is C.c_uint64
    assert lib.mipt_abi_version() == 4
    for name in ("MiptSampleMapOptions", "MiptSampleMapBuffers"):
        assert re.search(r"\}\s*" + name + r";\s*/\* 64 B \*/", open(os.path.join(ROOT, "include", "mipt.h")).read()), name


def test_struct_sizes_and_workspace_bytes(rrt):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    assert C.sizeof(L.MiptSampleMapOptions) == 64 and C.sizeof(L.MiptSampleMapBuffers) == 64
    assert L.MiptSampleMapOptions.budget.offset == 24 and L.MiptSampleMapBuffers.counts.offset == 24
    assert lib.mipt_sample_map_workspace_bytes(1, 1, 1) == 32
    assert lib.mipt_sample_map_workspace_bytes(1920, 1080, 4) == 32
    assert lib.mipt_sample_map_workspace_bytes(0, 8, 1) == 0 and lib.mipt_sample_map_workspace_bytes(8, 0, 1) == 0
    assert lib.mipt_sample_map_workspace_bytes(8, 8, 0) == 0
    assert lib.mipt_sample_map_workspace_bytes(65536, 65536, 1) == 0 and lib.mipt_sample_map_workspace_bytes(40000, 40000, 3) == 0


def _render(lib, which, scene, cams, n, opt, counts, hdr, rgba=None):
    if which == "mipt_render_adaptive":
        return lib.mipt_render_adaptive(scene, cams, n, C.byref(opt), counts, hdr, rgba, None)
    return lib.mipt_render_adaptive_device(scene, cams, n, C.byref(opt), counts, hdr, rgba, None, None)


@pytest.mark.parametrize("which", ENTRIES[:2])
def test_render_adaptive_argument_errors_without_a_device(rrt, which):
    """Refused with a message before the scene is touched: the scene argument below is an opaque non-null handle the checks never
    dereference."""
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    cams = np.zeros(3, dtype=L.CAMERA)
    opt = rrt.make_options(8, 8, 2, 1)
    handle = C.c_void_p(0x1000)
    counts = np.ones(2 * 64, dtype=np.uint32)
    hdr = np.zeros(2 * 64 * 3, dtype=np.float32)
    px = np.zeros(2 * 64 * 4, dtype=np.uint8)
    cp, hp = L.ptr(counts), L.ptr(hdr)
    cases = [
        ("null scene", None, L.ptr(cams), 2, opt, cp, hp, None, "null scene"),
        ("null cameras", handle, None, 2, opt, cp, hp, None, "null scene or cameras"),
        ("n_views = 0", handle, L.ptr(cams), 0, opt, cp, hp, None, "n_views == 0"),
        ("tile_world = 2", handle, L.ptr(cams), 2, rrt.make_options(8, 8, 1, 1, tile_world=2), cp, hp, None, "tile_world"),
        ("PACKED", handle, L.ptr(cams), 2, rrt.make_options(8, 8, 1, 1, flags=L.FLAG_PACKED), cp, hp, None, "PACKED"),
        ("TOUCHED", handle, L.ptr(cams), 2, rrt.make_options(8, 8, 1, 1, flags=L.FLAG_COUNT | L.FLAG_TOUCHED), cp, hp, None, "TOUCHED"),
        ("pixel limit", handle, L.ptr(cams), 3, rrt.make_options(40000, 40000, 1, 1), cp, hp, None, "2^32"),
        ("bad options", handle, L.ptr(cams), 2, rrt.make_options(0, 8, 1, 1), cp, hp, None, "Width and height"),
        ("samples = 0", handle, L.ptr(cams), 2, rrt.make_options(8, 8, 0, 1), cp, hp, None, "Sample count"),
        ("null counts", handle, L.ptr(cams), 2, opt, None, hp, None, "null counts"),
        ("ACCUM without SUM", handle, L.ptr(cams), 2, rrt.make_options(8, 8, 1, 1, flags=L.FLAG_ACCUM), cp, hp, None, "MIPT_FLAG_ACCUM needs MIPT_FLAG_SUM"),
        ("RGBA8 with SUM", handle, L.ptr(cams), 2, rrt.make_options(8, 8, 1, 1, flags=L.FLAG_SUM), cp, hp, L.ptr(px), "RGBA8"),
    ]
    if which == "mipt_render_adaptive":
        cases.append(("ACCUM on the host entry", handle, L.ptr(cams), 2, rrt.make_options(8, 8, 1, 1, flags=L.FLAG_SUM | L.FLAG_ACCUM), cp, hp, None,
                      "mipt_render_adaptive_device"))
    else:
        both = np.zeros(2 * 64 * 4, dtype=np.uint32)            # one allocation: counts inside hdr's range
        cases += [
            ("null hdr", handle, L.ptr(cams), 2, opt, cp, None, None, "d_hdr_rgb == NULL"),
            ("misaligned counts", handle, L.ptr(cams), 2, opt, C.c_void_p(counts.ctypes.data + 2), hp, None, "counts must be 4-byte aligned"),
            ("misaligned hdr", handle, L.ptr(cams), 2, opt, cp, C.c_void_p(hdr.ctypes.data + 1), None, "d_hdr_rgb must be 4-byte aligned"),
            ("counts overlaps hdr", handle, L.ptr(cams), 2, opt, C.c_void_p(both.ctypes.data + 64), L.ptr(both), None, "counts overlaps d_hdr_rgb"),
            ("counts overlaps rgba8", handle, L.ptr(cams), 2, opt, cp, hp, C.c_void_p(counts.ctypes.data + 16), "counts overlaps d_rgba8"),
            ("host memory", handle, L.ptr(cams), 2, opt, cp, hp, None, "is not device memory"),
        ]
    for name, sc, cm, n, o, c, h, r, msg in cases:
        assert _render(lib, which, sc, cm, n, o, c, h, r) == L.ERR_INVALID_ARG, name
        assert msg in lib.mipt_last_error().decode(), (name, lib.mipt_last_error())


def _map_args(L, n=64, **kw):
    opt = L.MiptSampleMapOptions()
    opt.width, opt.height, opt.n_views, opt.min_samples, opt.max_samples, opt.budget = 8, 8, 1, 1, 8, 2.0
    keep = dict(variance=np.zeros(n, dtype=np.float32), hdr=np.zeros(n * 3, dtype=np.float32), albedo=np.zeros(n * 3, dtype=np.float32),
                counts=np.zeros(n, dtype=np.uint32))
    bufs = L.MiptSampleMapBuffers()
    for k, a in keep.items():
        setattr(bufs, k, a.ctypes.data)
    return opt, bufs, keep


@pytest.mark.parametrize("which", ENTRIES[3:])
def test_sample_map_argument_errors_without_a_device(rrt, which):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    work = np.zeros(16, dtype=np.uint64)                        # 16-byte aligned below

    def call(opt, bufs, workspace="default"):
        o = C.byref(opt) if opt is not None else None
        b = C.byref(bufs) if bufs is not None else None
        if which == "mipt_sample_map":
            return lib.mipt_sample_map(o, b, 0)
        base = (work.ctypes.data + 15) & ~15
        return lib.mipt_sample_map_device(o, b, C.c_void_p(base) if workspace == "default" else workspace, None)

    def case(msg, edit=None, opt_none=False, bufs_none=False, **kw):
        opt, bufs, keep = _map_args(L)
        if edit:
            edit(opt, bufs, keep)
        assert call(None if opt_none else opt, None if bufs_none else bufs, **kw) == L.ERR_INVALID_ARG, msg
        assert msg in lib.mipt_last_error().decode(), (msg, lib.mipt_last_error())

    def set_(obj, **kw):
        for k, v in kw.items():
            setattr(obj, k, v)

    case("null opt", opt_none=True)
    case("null buffers", bufs_none=True)
    case("null variance", lambda o, b, k: set_(b, variance=None))
    case("null counts", lambda o, b, k: set_(b, counts=None))
    case("null hdr: albedo is given only with hdr", lambda o, b, k: set_(b, hdr=None))
    case("width and height", lambda o, b, k: set_(o, width=0))
    case("width and height", lambda o, b, k: set_(o, height=0))
    case("n_views == 0", lambda o, b, k: set_(o, n_views=0))
    case("below 2^32", lambda o, b, k: set_(o, width=65536, height=65536))
    case("flags 0x1", lambda o, b, k: set_(o, flags=1))
    case("reserved option fields", lambda o, b, k: o.reserved.__setitem__(8, 1))
    case("reserved buffer pointers", lambda o, b, k: b.reserved.__setitem__(3, 16))
    case("max_samples 0", lambda o, b, k: set_(o, min_samples=0, max_samples=0, budget=0.0))
    case("max_samples 65536", lambda o, b, k: set_(o, max_samples=65536))
    case("min_samples 9", lambda o, b, k: set_(o, min_samples=9))
    case("budget", lambda o, b, k: set_(o, budget=0.5))
    case("budget", lambda o, b, k: set_(o, budget=8.5))
    case("budget", lambda o, b, k: set_(o, budget=float("nan")))
    case("budget", lambda o, b, k: set_(o, budget=float("inf")))
    case("counts overlaps variance", lambda o, b, k: set_(b, counts=k["variance"].ctypes.data + 32))
    case("albedo overlaps hdr", lambda o, b, k: set_(b, albedo=k["hdr"].ctypes.data + 4))
    if which == "mipt_sample_map_device":
        case("null workspace", workspace=None)
        case("workspace must be 16-byte aligned", workspace=C.c_void_p(((work.ctypes.data + 15) & ~15) + 8))
        case("variance must be 4-byte aligned", lambda o, b, k: set_(b, variance=k["variance"].ctypes.data + 2, hdr=None, albedo=None))
        case("counts must be 4-byte aligned", lambda o, b, k: set_(b, counts=k["counts"].ctypes.data + 1))
        opt, bufs, keep = _map_args(L)
        assert call(opt, bufs, workspace=C.c_void_p((keep["counts"].ctypes.data + 15) & ~15)) == L.ERR_INVALID_ARG
        assert "counts overlaps the workspace" in lib.mipt_last_error().decode()
        case("is not device memory")                            # well-formed, but host pointers
