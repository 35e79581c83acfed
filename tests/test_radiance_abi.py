"""CPU: the radiance-query entry points (mipt_query_radiance and its _device form) are declared, exported and bound, their options
struct has the ABI's layout, every argument check that needs no device runs before anything touches the scene, and the Python
wrapper hands out the documented default seeds."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIANCE = ("mipt_query_radiance", "mipt_query_radiance_device")


def test_radiance_symbols_declared_exported_and_bound(rrt):
    from rust_ray_tracing_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mipt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mipt_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = rrt.load()
    for s in RADIANCE:
        assert s in declared and s in exported and s in L.EXPORTS, s
        assert getattr(lib, s).restype is C.c_int, s
        assert len(getattr(lib, s).argtypes) == (7 if s.endswith("_device") else 6), s
    assert exported == declared                      # libmipt.so still exports exactly the header's symbols
    assert lib.mipt_abi_version() == 4 and "#define MIPT_ABI_VERSION 4" in text


def test_radiance_options_layout(rrt):
    from rust_ray_tracing_amd import _lib as L
    O = L.MiptRadianceOptions
    assert C.sizeof(O) == 64
    want = dict(samples=0, max_ray_depth=4, traversal=8, cull_margin=12, shading=16, flags=20, reserved=24)
    assert {k: getattr(O, k).offset for k in want} == want and O.reserved.size == 40
    assert [k for k, _ in O._fields_] == list(want)
    assert L.RAY.itemsize == 32 and L.RAY.fields["reserved"][1] == 28 and L.RAY.fields["reserved"][0] == np.dtype("<u4")   # the seed word
    assert C.sizeof(L.MiptStats) == 8 + 22 * 8 and C.sizeof(L.MiptQueryOptions) == 32     # the existing structs keep their sizes
    text = open(os.path.join(ROOT, "include", "mipt.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} MiptRadianceOptions;", text).group(1)
    assert re.findall(r"(?:uint32_t|float)\s+(\w+)", body) == list(want)                # the header declares the same fields in the same order
    src = open(os.path.join(ROOT, "rust_ray_tracing_amd", "csrc", "mipt_radiance.cpp")).read()
    assert "sizeof(MiptRadianceOptions) == 64" in src                                     # the C side of the same claim


def _opt(L, **kw):
    o = L.MiptRadianceOptions()
    o.samples, o.max_ray_depth = 2, 8
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[v] = 1
        else:
            setattr(o, k, v)
    return o


@pytest.mark.parametrize("which", RADIANCE)
def test_radiance_argument_errors_without_a_device(rrt, which):
    """Refused with a message before the scene is touched: the scene argument is an opaque non-null handle the checks never
    dereference.  (Buffers that are not device memory of the scene's device need a scene: tests/test_gpu_radiance.py.)"""
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    device = which.endswith("_device")
    buf = np.zeros(4 * 32 + 4 * 12 + 32, dtype=np.uint8)         # 4 rays, then 4 results, from a 16-byte aligned address
    rp = buf.ctypes.data + (-buf.ctypes.data) % 16
    op = rp + 4 * 32
    handle = C.c_void_p(0x1000)
    nan, inf = float("nan"), float("inf")
    ok = _opt(L)
    cases = [
        ("null scene", None, rp, 4, ok, op, "null scene, rays, options or radiance"),
        ("null rays", handle, None, 4, ok, op, "null scene, rays, options or radiance"),
        ("null options", handle, rp, 4, None, op, "null scene, rays, options or radiance"),
        ("null radiance", handle, rp, 4, ok, None, "null scene, rays, options or radiance"),
        ("n_rays = 2^31", handle, rp, 1 << 31, ok, op, "below 2^31"),
        ("n_rays = 2^40", handle, rp, 1 << 40, ok, op, "below 2^31"),
        ("zero samples", handle, rp, 4, _opt(L, samples=0), op, "samples and max_ray_depth must be > 0"),
        ("zero depth", handle, rp, 4, _opt(L, max_ray_depth=0), op, "samples and max_ray_depth must be > 0"),
        ("bad traversal", handle, rp, 4, _opt(L, traversal=2), op, "unknown traversal"),
        ("bad shading", handle, rp, 4, _opt(L, shading=2), op, "unknown shading"),
        ("TOUCHED", handle, rp, 4, _opt(L, flags=L.FLAG_COUNT | L.FLAG_TOUCHED), op, "only MIPT_FLAG_COUNT, MIPT_FLAG_SUM and MIPT_FLAG_ACCUM"),
        ("PACKED", handle, rp, 4, _opt(L, flags=L.FLAG_PACKED), op, "only MIPT_FLAG_COUNT, MIPT_FLAG_SUM and MIPT_FLAG_ACCUM"),
        ("unknown flag", handle, rp, 4, _opt(L, flags=1 << 9), op, "only MIPT_FLAG_COUNT, MIPT_FLAG_SUM and MIPT_FLAG_ACCUM"),
        ("negative margin", handle, rp, 4, _opt(L, cull_margin=-0.5), op, "cull_margin"),
        ("NaN margin", handle, rp, 4, _opt(L, cull_margin=nan), op, "cull_margin"),
        ("infinite margin", handle, rp, 4, _opt(L, cull_margin=inf), op, "cull_margin"),
        ("reserved[0]", handle, rp, 4, _opt(L, reserved=0), op, "reserved"),
        ("reserved[9]", handle, rp, 4, _opt(L, reserved=9), op, "reserved"),
        ("ACCUM without SUM", handle, rp, 4, _opt(L, flags=L.FLAG_ACCUM), op, "MIPT_FLAG_ACCUM needs MIPT_FLAG_SUM"),
    ]
    if device:
        cases += [("unaligned rays", handle, rp + 4, 4, ok, op, "d_rays must be 16-byte aligned"),
                  ("unaligned radiance", handle, rp, 4, ok, op + 2, "d_radiance must be 4-byte aligned"),
                  ("radiance inside rays", handle, rp, 4, ok, rp + 64, "d_rays overlaps d_radiance"),
                  ("rays inside radiance", handle, rp + 16, 4, _opt(L, flags=L.FLAG_SUM | L.FLAG_ACCUM), rp, "d_rays overlaps d_radiance")]
    else:
        cases.append(("ACCUM on the host entry", handle, rp, 4, _opt(L, flags=L.FLAG_SUM | L.FLAG_ACCUM), op, "use mipt_query_radiance_device"))
    for name, sc, r, n, o, out, msg in cases:
        args = [sc, r, n, C.byref(o) if o is not None else None, out] + ([None] if device else []) + [None]
        assert getattr(lib, which)(*args) == L.ERR_INVALID_ARG, name
        assert msg in lib.mipt_last_error().decode() and which in lib.mipt_last_error().decode(), (name, lib.mipt_last_error())
    # no rays: MIPT_OK with nothing launched and the stats zeroed -- also against the opaque handle
    st = L.MiptStats()
    st.rays = 7
    args = [handle, rp, 0, C.byref(ok), op] + ([None] if device else []) + [C.byref(st)]
    assert getattr(lib, which)(*args) == L.OK
    assert st.rays == 0 and st.kernel_ms == 0.0


def test_default_seeds_are_the_pixel_formula_with_zero_replaced(rrt, orc):
    s = rrt.Scene.radiance_default_seeds(1000)
    assert s.dtype == np.uint32 and s.shape == (1000,)
    assert [int(x) for x in s[:3]] == [(987612486 * (i + 87636354)) % (1 << 32) for i in range(3)]
    lib = orc.load()
    assert all(int(s[i]) == lib.orc_pixel_seed(i) for i in (0, 1, 63, 64, 999))          # cpu.rs:28-29 as the oracle restates it
    # 987612486 = 2 * 493806243: the formula is 0 exactly where i + 87636354 is a multiple of 2^31
    z = (1 << 31) - 87636354
    t = rrt.Scene.radiance_default_seeds(3, first=z - 1)
    assert (987612486 * (z + 87636354)) % (1 << 32) == 0 and lib.orc_pixel_seed(z) == 0
    assert int(t[1]) == 1 and int(t[0]) == lib.orc_pixel_seed(z - 1) != 0 and int(t[2]) == lib.orc_pixel_seed(z + 1) != 0
    assert not np.any(rrt.Scene.radiance_default_seeds(4096) == 0)


def test_python_wrapper_rejects_bad_arguments_before_the_library(rrt):
    sc = rrt.Scene()                                             # not resident: a call that got past the ray checks raises RuntimeError
    good = np.zeros((5, 8), dtype=np.float32)
    for b in (np.zeros((5, 8), dtype=np.float64), np.zeros((5, 7), dtype=np.float32), "rays",
              (np.zeros((5, 3), np.float32), np.zeros((4, 3), np.float32))):
        with pytest.raises(ValueError):
            sc.query_radiance(b)
    with pytest.raises(RuntimeError):
        sc.query_radiance(good)
