"""CPU: the entries of include/mipt.h "lightmap finishing" and mipt_bake_surface are declared, exported and bound, their structs have
the ABI's layout, the paths without work return MIPT_OK, and every refusal that needs no device is held to its status and its WHOLE
message; inputs with two faults fix the order in which the checks fire.  The planes are zero-filled host arrays of an 8 x 4 atlas,
which the device entries turn away as "not device memory" at the latest; the host entries are only ever given a fault or a device
ordinal that does not exist.  The Python wrappers refuse bad input before the library is called."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 8, 4
N = W * H
NO_DEVICE = 1 << 20
HIP_TEXTS = ("no ROCm-capable device is detected", "invalid device ordinal")
SURFACE = ("mipt_bake_surface", "mipt_bake_surface_device")
PLANE_ENTRIES = ("mipt_lightmap_filter", "mipt_lightmap_filter_device", "mipt_lightmap_dilate", "mipt_lightmap_dilate_device")
SIZERS = ("mipt_lightmap_filter_workspace_bytes", "mipt_lightmap_dilate_workspace_bytes")


def _block(n_bytes):
    raw = np.zeros(n_bytes + 96, dtype=np.uint8)
    off = -raw.ctypes.data % 16
    return raw[off: off + n_bytes + 64]


def test_symbols_declared_exported_and_bound(rrt):
    from rust_ray_tracing_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mipt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mipt_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = rrt.load()
    for s in SURFACE + PLANE_ENTRIES + SIZERS:
        assert s in declared and s in exported and s in L.EXPORTS, s
    for s in SURFACE + PLANE_ENTRIES:
        assert getattr(lib, s).restype is C.c_int, s
    assert [len(getattr(lib, s).argtypes) for s in SURFACE + PLANE_ENTRIES] == [6, 7, 3, 5, 3, 5]
    assert all(getattr(lib, s).restype is C.c_uint64 for s in SIZERS)
    assert exported == declared
    assert lib.mipt_abi_version() == 4


def test_struct_layouts(rrt):
    from rust_ray_tracing_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "mipt.h")).read()
    S = L.MiptBakeSurfaceOptions
    assert C.sizeof(S) == 32 and S.flags.offset == 0 and S.reserved.offset == 4 and L.BAKE_SURFACE_UNIT_NORMALS == 1
    assert "#define MIPT_BAKE_SURFACE_UNIT_NORMALS 1u" in text and "#define MIPT_LIGHTMAP_MAX_RADIUS 64u" in text
    O = L.MiptLightmapFilterOptions
    want = dict(width=0, height=4, iterations=8, sigma_color=12, sigma_normal=16, sigma_plane=20, sigma_distance=24, flags=28, reserved=32)
    assert C.sizeof(O) == 64 and {k: getattr(O, k).offset for k in want} == want and [k for k, _ in O._fields_] == list(want)
    body = re.search(r"typedef struct \{([^}]*)\} MiptLightmapFilterOptions;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    assert re.findall(r"(\w+)\s*(?:\[\d+\])?\s*[,;]", body) == list(want)
    B = L.MiptLightmapFilterBuffers
    want = dict(radiance=0, points=8, position=16, normal=24, out=32, reserved=40)
    assert C.sizeof(B) == 64 and {k: getattr(B, k).offset for k in want} == want
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} MiptLightmapFilterBuffers;", text).group(1))
    assert re.findall(r"\*\s*(\w+)", body) == list(want)
    O = L.MiptLightmapDilateOptions
    want = dict(width=0, height=4, radius=8, flags=12, reserved=16)
    assert C.sizeof(O) == 32 and {k: getattr(O, k).offset for k in want} == want
    B = L.MiptLightmapDilateBuffers
    want = dict(radiance=0, points=8, out=16, level=24, reserved=32)
    assert C.sizeof(B) == 64 and {k: getattr(B, k).offset for k in want} == want
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} MiptLightmapDilateBuffers;", text).group(1))
    assert re.findall(r"\*\s*(\w+)", body) == list(want)
    src = open(os.path.join(ROOT, "rust_ray_tracing_amd", "csrc", "mipt_lightmap.cpp")).read()
    assert "sizeof(MiptLightmapFilterOptions) == 64 && sizeof(MiptLightmapFilterBuffers) == 64" in src
    assert "sizeof(MiptLightmapDilateOptions) == 32 && sizeof(MiptLightmapDilateBuffers) == 64" in src


def test_workspace_sizes(rrt):
    lib = rrt.load()
    f, d = lib.mipt_lightmap_filter_workspace_bytes, lib.mipt_lightmap_dilate_workspace_bytes
    assert f(W, H) == 64 * N and d(W, H) == 32 * N and f(1, 1) == 64 and d(2048, 2048) == 32 << 22
    for w, h in ((0, 5), (5, 0), (1 << 16, 1 << 15), ((1 << 32) - 1, (1 << 32) - 1)):
        assert f(w, h) == 0 and d(w, h) == 0
    assert f((1 << 31) - 1, 1) == 64 * ((1 << 31) - 1)


# ---- mipt_bake_surface -------------------------------------------------------------------------------------------------------------
def _sopt(L, flags=0, reserved=None):
    o = L.MiptBakeSurfaceOptions()
    o.flags = flags
    if reserved is not None:
        o.reserved[reserved] = 1
    return o


@pytest.mark.parametrize("which", SURFACE)
def test_surface_refusals_whole_messages_and_order(rrt, which):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    device = which.endswith("_device")
    mem = _block(4 * 16 + 2 * 4 * 12)
    pp = mem.ctypes.data
    pos, nrm = pp + 64, pp + 64 + 48
    handle = C.c_void_p(0x1000)                                    # opaque: no check before the buffers' dereferences it
    null = "null scene or points, or position and normal both null"
    flags = "flags 0x2: only MIPT_BAKE_SURFACE_UNIT_NORMALS is accepted"
    cases = [
        ("null scene", None, pp, 4, None, pos, nrm, null),
        ("null points", handle, None, 4, None, pos, nrm, null),
        ("no output", handle, pp, 4, None, None, None, null),
        ("n = 2^31", handle, pp, 1 << 31, None, pos, nrm, "n 2147483648: must stay below 2^31"),
        ("a flag", handle, pp, 4, _sopt(L, flags=2), pos, nrm, flags),
        ("reserved[6]", handle, pp, 4, _sopt(L, reserved=6), pos, None, "reserved option fields must be 0"),
        # pairs: the earlier check speaks
        ("no output + n", handle, pp, 1 << 40, None, None, None, null),
        ("n + flag", handle, pp, 1 << 31, _sopt(L, flags=3), pos, nrm, "n 2147483648: must stay below 2^31"),
        ("flag + reserved", handle, pp, 4, _sopt(L, flags=2, reserved=0), pos, nrm, flags),
    ]
    if device:
        cases += [
            ("unaligned points", handle, pp + 8, 4, None, pos, nrm, "d_points must be 16-byte aligned"),
            ("unaligned position", handle, pp, 4, None, pos + 2, nrm, "d_position must be 4-byte aligned"),
            ("unaligned normal", handle, pp, 4, None, None, nrm + 1, "d_normal must be 4-byte aligned"),
            ("position in points", handle, pp, 4, None, pp + 60, nrm, "d_points overlaps d_position"),
            ("normal in points", handle, pp, 4, None, pos, pp + 16, "d_points overlaps d_normal"),
            ("normal in position", handle, pp, 4, None, pos, pos + 44, "d_position overlaps d_normal"),
            ("reserved + unaligned", handle, pp + 8, 4, _sopt(L, reserved=1), pos, nrm, "reserved option fields must be 0"),
            ("points + position unaligned", handle, pp + 4, 4, None, pos + 1, nrm, "d_points must be 16-byte aligned"),
            ("unaligned + overlap", handle, pp, 4, None, pp + 2, nrm, "d_position must be 4-byte aligned"),
            ("two overlaps", handle, pp, 4, None, pp + 32, pp + 36, "d_points overlaps d_position"),
        ]
    before = mem.copy()
    for name, sc, p, n, o, a, b, msg in cases:
        args = [sc, p, n, C.byref(o) if o is not None else None, a, b] + ([None] if device else [])
        assert getattr(lib, which)(*args) == L.ERR_INVALID_ARG, name
        assert lib.mipt_last_error().decode() == f"{which}: {msg}", (name, lib.mipt_last_error())
    # no points: MIPT_OK without a launch, whatever else is wrong behind the alignment checks
    assert getattr(lib, which)(*([handle, pp, 0, None, pos, nrm] + ([None] if device else []))) == L.OK
    assert getattr(lib, which)(*([handle, pp, 0, C.byref(_sopt(L, flags=1)), pp, None] + ([None] if device else []))) == L.OK
    assert np.array_equal(mem, before)


# ---- the plane entries -------------------------------------------------------------------------------------------------------------
class Entry:
    def __init__(self, L, which):
        self.which, self.device = which, which.endswith("_device")
        self.filter = "filter" in which
        self.opt_cls = L.MiptLightmapFilterOptions if self.filter else L.MiptLightmapDilateOptions
        self.buf_cls = L.MiptLightmapFilterBuffers if self.filter else L.MiptLightmapDilateBuffers
        self.defaults = (dict(width=W, height=H, iterations=2, sigma_color=1.0, sigma_normal=1.0, sigma_plane=1.0, sigma_distance=1.0)
                         if self.filter else dict(width=W, height=H, radius=2))
        sizes = dict(radiance=12, points=16, position=12, normal=12, out=12) if self.filter else dict(radiance=12, points=16, out=12, level=4)
        self.mem = {k: _block(N * b) for k, b in sizes.items()}
        self.ws_need = N * (64 if self.filter else 32)
        self.mem["ws"] = _block(self.ws_need + N * 16)
        self.sizer = "mipt_lightmap_filter_workspace_bytes" if self.filter else "mipt_lightmap_dilate_workspace_bytes"

    def at(self, name, off=0):
        return self.mem[name].ctypes.data + off

    def call(self, lib, opt=(), buf=(), ws=True, ws_bytes=None, device_id=NO_DEVICE):
        o = None
        if opt is not None:
            o = self.opt_cls()
            for k, v in dict(self.defaults, **dict(opt)).items():
                if k == "reserved":
                    o.reserved[v] = 1
                else:
                    setattr(o, k, v)
        b = None
        if buf is not None:
            b = self.buf_cls()
            for k, _ in self.buf_cls._fields_:
                if k != "reserved":
                    setattr(b, k, self.at(k))
            for k, v in dict(buf).items():
                if k == "reserved":
                    b.reserved[v] = self.at("ws")
                else:
                    setattr(b, k, v)
        args = [C.byref(o) if o is not None else None, C.byref(b) if b is not None else None]
        if self.device:
            p = self.at("ws") if ws is True else ws
            args += [p, self.ws_need if ws_bytes is None else ws_bytes, None]
        else:
            args += [device_id]
        return getattr(lib, self.which)(*args)


@pytest.mark.parametrize("which", PLANE_ENTRIES)
def test_plane_entry_refusals_whole_messages_and_order(rrt, which):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    e = Entry(L, which)
    nan, inf = float("nan"), float("inf")
    zero = "width and height must be greater than 0"
    cases = [
        ("null opt", dict(opt=None), "null opt"),
        ("null buffers", dict(buf=None), "null buffers"),
        ("null opt + buffers", dict(opt=None, buf=None), "null opt"),
        ("null radiance", dict(buf=dict(radiance=None)), "null radiance"),
        ("null points", dict(buf=dict(points=None)), "null points"),
        ("null out", dict(buf=dict(out=None)), "null out"),
        ("null radiance + out", dict(buf=dict(radiance=None, out=None)), "null radiance"),
        ("zero width", dict(opt=dict(width=0)), zero),
        ("zero height", dict(opt=dict(height=0)), zero),
        ("null out + zero width", dict(opt=dict(width=0), buf=dict(out=None)), "null out"),
        ("2^31 texels", dict(opt=dict(width=1 << 16, height=1 << 15)), "65536 x 32768 texels: width * height must stay below 2^31"),
        ("flags", dict(opt=dict(flags=1)), "flags 0x1: must be 0"),
        ("reserved option", dict(opt=dict(reserved=0)), "reserved option fields must be 0"),
        ("reserved pointer", dict(buf=dict(reserved=2)), "reserved buffer pointers must be NULL"),
        ("flags + reserved", dict(opt=dict(flags=4, reserved=1)), "flags 0x4: must be 0"),
        ("reserved option + pointer", dict(opt=dict(reserved=3), buf=dict(reserved=0)), "reserved option fields must be 0"),
        ("out inside points", dict(buf=dict(out=e.at("points", 16))), "out overlaps points (only out == radiance is allowed)"),
        ("out inside radiance", dict(buf=dict(out=e.at("radiance", 12))), "out overlaps radiance (only out == radiance is allowed)"),
        ("points inside radiance", dict(buf=dict(points=e.at("radiance", 16))), "points overlaps radiance (only out == radiance is allowed)"),
    ]
    if e.filter:
        it = "iterations 0: must be 1 ... 8"
        cases += [
            ("iterations 0", dict(opt=dict(iterations=0)), it),
            ("iterations 9", dict(opt=dict(iterations=9)), "iterations 9: must be 1 ... 8"),
            ("size + iterations", dict(opt=dict(width=1 << 20, height=1 << 20, iterations=0)), "1048576 x 1048576 texels: width * height must stay below 2^31"),
            ("iterations + flags", dict(opt=dict(iterations=0, flags=1)), it),
            ("sigma_color 0", dict(opt=dict(sigma_color=0.0)), "sigma_color must be finite and greater than 0"),
            ("sigma_color NaN", dict(opt=dict(sigma_color=nan)), "sigma_color must be finite and greater than 0"),
            ("sigma_color tiny", dict(opt=dict(sigma_color=1e-30)), "sigma_color 1e-30: 1 / (sigma_color * 2^-0)^2 is not finite and greater than 0"),
            ("sigma_color large", dict(opt=dict(sigma_color=2e19)), "sigma_color 2e+19: 1 / (sigma_color * 2^-0)^2 is not finite and greater than 0"),
            ("sigma_normal 0", dict(opt=dict(sigma_normal=0.0)), "sigma_normal 0: it and 1 / sigma_normal^2 must be finite and greater than 0"),
            ("sigma_plane inf", dict(opt=dict(sigma_plane=inf)), "sigma_plane inf: it and 1 / sigma_plane^2 must be finite and greater than 0"),
            ("sigma_distance -1", dict(opt=dict(sigma_distance=-1.0)), "sigma_distance must be finite and greater than 0"),
            ("sigma_distance large at i = 1", dict(opt=dict(sigma_distance=1e19)),
             "sigma_distance 1e+19: 1 / (sigma_distance * 2^1)^2 is not finite and greater than 0"),
            ("reserved + sigma", dict(opt=dict(sigma_color=0.0), buf=dict(reserved=0)), "reserved buffer pointers must be NULL"),
            ("colour + normal", dict(opt=dict(sigma_color=-1.0, sigma_normal=0.0)), "sigma_color must be finite and greater than 0"),
            ("normal + plane", dict(opt=dict(sigma_normal=nan, sigma_plane=0.0)), "sigma_normal nan: it and 1 / sigma_normal^2 must be finite and greater than 0"),
            ("plane + distance", dict(opt=dict(sigma_plane=0.0, sigma_distance=0.0)), "sigma_plane 0: it and 1 / sigma_plane^2 must be finite and greater than 0"),
            ("sigma + overlap", dict(opt=dict(sigma_distance=0.0), buf=dict(out=e.at("points"))), "sigma_distance must be finite and greater than 0"),
            ("normal inside position", dict(buf=dict(normal=e.at("position", 24))), "normal overlaps position (only out == radiance is allowed)"),
        ]
    else:
        cases += [
            ("radius 65", dict(opt=dict(radius=65)), "radius 65: must be 0 ... 64"),
            ("size + radius", dict(opt=dict(width=1 << 20, height=1 << 20, radius=99)), "1048576 x 1048576 texels: width * height must stay below 2^31"),
            ("radius + flags", dict(opt=dict(radius=1000, flags=1)), "radius 1000: must be 0 ... 64"),
            ("level inside out", dict(buf=dict(level=e.at("out", 4))), "level overlaps out (only out == radiance is allowed)"),
        ]
    if e.device:
        small = f"workspace of 16 bytes is too small: {e.sizer}() is {e.ws_need}"
        cases += [
            ("null workspace", dict(ws=None), "null workspace"),
            ("small workspace", dict(ws_bytes=16), small),
            ("unaligned workspace", dict(ws=e.at("ws", 8)), "workspace must be 16-byte aligned"),
            ("small + unaligned workspace", dict(ws=e.at("ws", 4), ws_bytes=16), small),
            ("overlap + null workspace", dict(ws=None, buf=dict(out=e.at("points"))), "out overlaps points (only out == radiance is allowed)"),
            ("unaligned radiance", dict(buf=dict(radiance=e.at("radiance", 2))), "radiance must be 4-byte aligned"),
            ("unaligned points", dict(buf=dict(points=e.at("points", 8))), "points must be 16-byte aligned"),
            ("unaligned out", dict(buf=dict(out=e.at("out", 1))), "out must be 4-byte aligned"),
            ("workspace + plane unaligned", dict(ws=e.at("ws", 8), buf=dict(points=e.at("points", 4))), "workspace must be 16-byte aligned"),
            ("out in the workspace", dict(buf=dict(out=e.at("ws", e.ws_need - 4))), "out overlaps the workspace"),
            ("host memory", dict(), "radiance is not device memory"),
            ("out == radiance in host memory", dict(buf=dict(out=e.at("radiance"))), "radiance is not device memory"),
        ]
    before = {k: v.copy() for k, v in e.mem.items()}
    for name, kw, msg in cases:
        assert e.call(lib, **kw) == L.ERR_INVALID_ARG, name
        assert lib.mipt_last_error().decode() == f"{which}: {msg}", (name, lib.mipt_last_error())
    if not e.device:
        # everything right: the first use of a device is the first thing that can fail (also with out == radiance and no guides)
        for kw in (dict(), dict(buf=dict(out=e.at("radiance"))), dict(buf=dict(position=None, normal=None) if e.filter else dict(level=None)),
                   dict(opt=dict(sigma_normal=0.0, sigma_plane=nan, sigma_distance=-1.0), buf=dict(position=None, normal=None)) if e.filter else dict()):
            assert e.call(lib, **kw) == L.ERR_HIP
            text = lib.mipt_last_error().decode()
            assert text.startswith(f"{which}: hipSetDevice(device_id = {NO_DEVICE}) failed: ") and text.endswith(HIP_TEXTS), text
    assert all(np.array_equal(v, before[k]) for k, v in e.mem.items())


def test_python_wrappers_refuse_bad_arguments_before_the_library(rrt):
    from rust_ray_tracing_amd import _lib as L
    sc = rrt.Scene()                                               # not resident: a call that got past the checks raises RuntimeError
    good = np.zeros(6, dtype=L.SURFACE_POINT)
    for bad in (np.zeros((6, 4), dtype=np.float32), np.zeros((6, 3), dtype=np.uint32), "points"):
        with pytest.raises(ValueError):
            sc.bake_surface(bad)
    for want in ((), ("uv",), ("position", "depth")):
        with pytest.raises(ValueError):
            sc.bake_surface(good, want=want)
    with pytest.raises(RuntimeError):
        sc.bake_surface(good)
    with pytest.raises(RuntimeError):
        sc.bake_surface(good, unit_normals=True, want=("normal",))
    rad = np.zeros((2, 3, 3), dtype=np.float32)
    for f in (rrt.lightmap_filter, rrt.lightmap_dilate, rrt.Scene.lightmap_filter, rrt.Scene.lightmap_dilate):
        for r, p in ((np.zeros((2, 3), np.float32), good), (np.zeros((2, 3, 4), np.float32), good), (rad, good[:5]),
                     (rad, np.zeros((6, 3), np.uint32)), (rad.astype(np.float64), good)):
            with pytest.raises(ValueError):
                f(r, p)
    for g in (np.zeros((2, 3, 3), np.float64), np.zeros((3, 3, 3), np.float32), np.zeros((6, 4), np.float32)):
        with pytest.raises(ValueError):
            rrt.lightmap_filter(rad, good, position=g)
        with pytest.raises(ValueError):
            rrt.lightmap_filter(rad, good, normal=g)
    # past the wrapper, the library's own refusal comes back as MiptError with its message
    with pytest.raises(L.MiptError, match="iterations 0: must be 1 ... 8"):
        rrt.lightmap_filter(rad, good, iterations=0, device_id=NO_DEVICE)
    with pytest.raises(L.MiptError, match="radius 65: must be 0 ... 64"):
        rrt.lightmap_dilate(rad, good, radius=65, device_id=NO_DEVICE)
    with pytest.raises(L.MiptError, match="hipSetDevice"):
        rrt.lightmap_filter(rad, good, position=np.zeros((6, 3), np.float32), normal=np.zeros((2, 3, 3), np.float32), device_id=NO_DEVICE)
    # bake_lightmap's new arguments do nothing until the two steps have run
    with pytest.raises(RuntimeError):
        sc.bake_lightmap(4, 4, 1, device=False, filter=dict(iterations=2), dilate=2)
