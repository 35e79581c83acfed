"""-m gpu: texel_rgb (csrc/pt_texel.h) -- the one nearest-texel lookup the trace kernels and the first-hit pass inline -- evaluated
element-wise through libmipt_diag.so's mipt_debug_texel, against the numpy reading of tests/tools/texel_model.py (itself held to the
oracle by tests/test_texel_model.py): the colour bit for bit (NaN = NaN) and the clamp count exactly.

Every texture sits at a non-zero offset inside a pool, between guard texels whose colours differ from all of its own, so a wrong
offset or an index outside the texture shows as a wrong colour.  The probe is handed data only: every index the model forms is
checked to lie inside the texture before anything is launched, and the probe refuses a texture that does not fit its pool."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))

import texel_model as T  # noqa: E402


def _probe(rrt, pool, offset, width, height, u, v):
    lib = rrt.load_diag()
    uv = np.ascontiguousarray(np.stack([u, v], axis=1), dtype=np.float32)
    pool = np.ascontiguousarray(pool, dtype=np.uint32)
    rgb = np.full((len(uv), 3), -1.0, dtype=np.float32)
    clamped = C.c_uint64(1 << 60)
    rc = lib.mipt_debug_texel(uv.ctypes.data, len(uv), pool.ctypes.data, pool.size, offset, width, height, rgb.ctypes.data, C.byref(clamped))
    assert rc == 0, lib.mipt_diag_last_error()
    return rgb, clamped.value


def _compare(rrt, width, height, u, v, what):
    pool, offset, _ = T.guarded_pool(width, height)
    assert offset > 0 and offset + width * height < pool.size
    want, n_clamped, idx = T.texel_rgb(pool, offset, width, height, u, v)
    cov = T.coverage(u, v, width, height)
    # before the launch: the indices stay inside the texture, and the sweep reaches the classes it is for.  |fract| < 1, so on a
    # 1x1 texture both casts give 0 and no lookup can be clamped; every other shape must clamp some.
    assert cov["lo"] >= 0 and cov["hi"] < width * height
    assert (cov["clamped"] > 0) == (width * height > 1) and cov["clamped"] == n_clamped, cov
    assert cov["negative_unclamped"] > 0 and cov["first"] > 0 and cov["last"] > 0, cov
    got, got_clamped = _probe(rrt, pool, offset, width, height, u, v)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        k = int(np.argwhere(~same)[0][0])
        raise AssertionError(f"{what} {width}x{height}: {int((~same).any(axis=1).sum())} of {len(u)} colours differ, first at "
                             f"uv = ({u[k]!r}, {v[k]!r}): {got[k]!r} != {want[k]!r} (model index {idx[k]})")
    assert got_clamped == n_clamped, (what, width, height, got_clamped, n_clamped)


@pytest.mark.parametrize("width,height", T.SHAPES)
def test_device_texel_equals_model_on_the_edge_pairs(rrt, width, height):
    u, v = T.edge_pairs(width, height)
    _compare(rrt, width, height, u, v, "edges")


@pytest.mark.parametrize("width,height", T.SHAPES)
def test_device_texel_equals_model_on_the_random_pairs(rrt, width, height):
    u, v = T.random_pairs(width, height)
    _compare(rrt, width, height, u, v, "random")


def test_probe_refuses_what_does_not_fit_its_pool(rrt):
    lib = rrt.load_diag()
    pool = np.arange(20, dtype=np.uint32)
    uv, rgb, n = np.zeros((4, 2), np.float32), np.zeros((4, 3), np.float32), C.c_uint64(0)
    args = lambda off, w, h, words=pool.size: (uv.ctypes.data, 4, pool.ctypes.data, words, off, w, h, rgb.ctypes.data, C.byref(n))  # noqa: E731
    assert lib.mipt_debug_texel(*args(5, 5, 3)) == 0                         # 5 + 15 = 20: the last texel is the pool's last word
    assert lib.mipt_debug_texel(*args(6, 5, 3)) == -1
    assert lib.mipt_debug_texel(*args(0xFFFFFFFF, 1, 1)) == -1               # the sum is not taken in 32 bits
    assert lib.mipt_debug_texel(*args(0, 0x10000, 0x10000)) == -1            # nor the product
    assert lib.mipt_debug_texel(*args(0, 0, 3)) == -1 and lib.mipt_debug_texel(*args(0, 3, 0)) == -1
    assert lib.mipt_debug_texel(*args(0, 1, 1, words=0)) == -1
    assert lib.mipt_debug_texel(None, 4, pool.ctypes.data, pool.size, 0, 1, 1, rgb.ctypes.data, C.byref(n)) == -1
    assert lib.mipt_debug_texel(uv.ctypes.data, 0, pool.ctypes.data, pool.size, 0, 1, 1, rgb.ctypes.data, C.byref(n)) == -1
    assert b"mipt_debug_texel" in lib.mipt_diag_last_error()
