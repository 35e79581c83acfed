"""The numpy reading of the nearest-texel lookup (tests/tools/texel_model.py) held to the oracle's (oracle/pt_oracle.c tex_lookup,
through orc_texture_color_at and its batch form orc_texture_lookup_many, which also returns the flag trace adds to tex_clamped):
colour, texel index and clamp decision on every coordinate pair tests/test_gpu_texel.py hands the device function.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))

import texel_model as T  # noqa: E402


def _check(orc, width, height, u, v, what):
    pool, offset, tex = T.guarded_pool(width, height)
    rgba, flags, total = orc.texture_lookup_many(tex, u, v)
    rgb, n_clamped, idx = T.texel_rgb(pool, offset, width, height, u, v)
    _, clamped, _ = T.lookup_index(u, v, width, height)
    assert idx.min() >= 0 and idx.max() < width * height
    want = rgba[:, :3].astype(np.float32) / np.float32(255.0)
    bad = np.flatnonzero((rgb.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert bad.size == 0, f"{what} {width}x{height}: {bad.size} colours differ, first at uv = ({u[bad[0]]!r}, {v[bad[0]]!r})"
    # the texels are distinct, so equal colours are equal indices; said once more through the texture itself
    assert np.array_equal(tex.reshape(-1, 4)[idx], rgba)
    bad = np.flatnonzero(clamped != (flags != 0))
    assert bad.size == 0, f"{what} {width}x{height}: {bad.size} clamp decisions differ, first at uv = ({u[bad[0]]!r}, {v[bad[0]]!r})"
    assert n_clamped == total == int(flags.sum())
    return T.coverage(u, v, width, height)


@pytest.mark.parametrize("width,height", T.SHAPES)
def test_model_equals_oracle_on_the_edge_pairs(orc, width, height):
    u, v = T.edge_pairs(width, height)
    assert u.size == v.size and u.size <= T.MAX_SQUARE
    cov = _check(orc, width, height, u, v, "edges")
    # |fract| < 1, so on a 1x1 texture both casts give 0 and nothing can leave it; everywhere else the sweep must clamp some
    assert (cov["clamped"] > 0) == (width * height > 1), cov
    assert cov["negative_unclamped"] > 0 and cov["first"] > 0 and cov["last"] > 0, cov


@pytest.mark.parametrize("width,height", T.SHAPES)
def test_model_equals_oracle_on_the_random_pairs(orc, width, height):
    u, v = T.random_pairs(width, height)
    assert u.size == 1 << 21
    cov = _check(orc, width, height, u, v, "random")
    assert (cov["clamped"] > 0) == (width * height > 1) and cov["negative_unclamped"] > 0 and cov["first"] > 0 and cov["last"] > 0, cov


def test_batch_entry_is_the_single_lookup(orc):
    """orc_texture_lookup_many against orc_texture_color_at, pair by pair, on the specials and a period of boundaries"""
    lib = orc.load()
    for width, height in ((3, 5), (7, 1)):
        _, _, tex = T.guarded_pool(width, height)
        c = np.concatenate([T.special_coords(), T.boundary_coords(width)[::3], T.boundary_coords(height)[::3]])
        gu, gv = np.meshgrid(c, c)
        u, v = gu.reshape(-1), gv.reshape(-1)
        rgba, _, _ = orc.texture_lookup_many(tex, u, v)
        t = orc.OrcTexture(width, height, tex.ctypes.data)
        px = (C.c_uint8 * 4)()
        for k in range(u.size):
            lib.orc_texture_color_at(C.byref(t), C.c_float(float(u[k])), C.c_float(float(v[k])), C.byref(px))
            assert tuple(px) == tuple(rgba[k]), (u[k], v[k])


def test_worked_examples():
    """Cases worked by hand from texture.rs:33-38 on a 5x3 texture (width 5, height 3)."""
    w, h = 5, 3
    f = np.float32

    def one(u, v):
        idx, clamped, raw = T.lookup_index(np.array([u], f), np.array([v], f), w, h)
        return int(idx[0]), bool(clamped[0]), int(raw[0])

    assert one(0.0, 0.0) == (0, False, 0)
    assert one(0.5, 0.5) == (2 + 1 * 5, False, 7)                       # i = int(2.5) = 2, j = int(1.5) = 1
    assert one(-0.25, 0.75) == (-1 + 2 * 5, False, 9)                   # mixed signs: i = int(-1.25) = -1, j = int(2.25) = 2: inside, not counted
    assert one(0.25, -0.5) == (0, True, 1 - 5)                          # i = 1, j = int(-1.5) = -1: below the texture
    assert one(-1e-45, -1e-30) == (0, False, 0)                         # -tiny truncates to 0: negative, not counted
    assert one(7.0, -3.0) == (0, False, 0)                              # fract of an integer is +-0
    assert one(np.inf, np.nan) == (0, False, 0)                         # fract(inf) = NaN -> 0
    assert one(3e38, -2.0 ** 24) == (0, False, 0)                       # every f32 from 2^23 on is an integer
    assert one(np.nextafter(f(1), f(0)), np.nextafter(f(1), f(0))) == (14, False, 14)   # 5 (1 - 2^-24) rounds to 5 - 2^-21, 3 (1 - 2^-24) to 3 - 2^-22
    assert one(np.nextafter(f(-1), f(0)), 0.0) == (0, True, -4)
    rgb, n, idx = T.texel_rgb(np.array([9, 0x00FF8001, 9], np.uint32), 1, 1, 1, np.array([0.3], f), np.array([0.9], f))
    assert n == 0 and idx[0] == 0 and np.array_equal(rgb[0], np.array([1, 128, 255], f) / f(255))
    assert np.array_equal(T._sat_i32(np.array([2147483520.0, 2147483648.0, -2147483648.0, -3e9, np.nan, -0.9, 0.9], f)),
                          np.array([2147483520, T.I32_MAX, T.I32_MIN, T.I32_MIN, 0, 0, 0]))
