"""CPU: the array-shaped statements of the frame epilogues and of the shard assembly (tests/tools/epilogue_model.py) against the
oracle's scalar statements and sharding.unpack, and the placement of the boundary windows the GPU tests (tests/test_gpu_epilogue.py)
feed to the kernels.  Everything is compared exactly."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import epilogue_model as M  # noqa: E402


def _scalar_rgb8(orc, values):
    """orc_linear_to_srgb + orc_quantize, one value at a time."""
    lib = orc.load()
    out = np.zeros(len(values), dtype=np.uint8)
    s3, q3 = (C.c_float * 3)(), (C.c_uint8 * 3)()
    for i, v in enumerate(values):
        lib.orc_linear_to_srgb(C.byref((C.c_float * 3)(v, v, v)), 0, C.byref(s3))
        lib.orc_quantize(C.byref(s3), C.byref(q3))
        assert q3[0] == q3[1] == q3[2]
        out[i] = q3[0]
    return out


def test_rgba8_model_equals_the_scalar_oracle(orc):
    """Every value of the 8-bit boundary set (255 windows of 65 values) and the specials; the channels of the boundary pixels and the
    alpha byte too."""
    win, pixels = M.boundary8()
    values = np.concatenate([win.reshape(-1), np.float32([0.25, 0.5, 0.125]), M.specials()])   # + the filler channels of special_pixels
    want = _scalar_rgb8(orc, values)
    got = M.rgba8_model(np.repeat(values[:, None], 3, axis=1), 1.0)
    assert got.shape == (len(values), 4) and np.all(got[:, 3] == 255)
    for ch in range(3):
        assert np.array_equal(got[:, ch], want)
    by_value = dict(zip(values.view(np.uint32).tolist(), want.tolist()))
    for px in (pixels, M.special_pixels()):
        g = M.rgba8_model(px, 1.0)
        w = np.array([by_value[b] for b in px.view(np.uint32).reshape(-1).tolist()], dtype=np.uint8).reshape(-1, 3)
        assert np.array_equal(g[:, :3], w) and np.all(g[:, 3] == 255)
    sp = dict(zip(M.specials().view(np.uint32).tolist(), want[-len(M.specials()):].tolist()))
    assert sp[0x7F800000] == 0                       # +inf: inf * 0 in the mix is NaN, and NaN quantises to 0
    assert sp[0x7F7FFFFF] == 0                       # FLT_MAX too: the unused `lower` = c * 12.92 overflows to inf
    assert sp[0x3F800000] == 254 and sp[0x40F00000] == 255                               # 1.0 (254 in f32, test_oracle_kat), 7.5
    assert sp[0xFF800000] == 0 and sp[0x7FC12345] == 0 and sp[0xBF000000] == 0           # -inf, NaN, -0.5
    # a divisor: the same bytes as dividing first (numpy's correctly rounded f32 quotient), and 1.0 skips the division
    for d in (3.0, 7.0, 64.0):
        with np.errstate(all="ignore"):
            assert np.array_equal(M.rgba8_model(pixels, d), M.rgba8_model(pixels / np.float32(d), 1.0))
    with np.errstate(all="ignore"):
        assert not M.rgba8_model(M.special_pixels(), 0.0)[:, :3].any()                   # x / 0 is NaN or infinite: every byte 0
        assert not M.rgba8_model(M.special_pixels(), float("nan"))[:, :3].any()


def test_unpack_model_equals_sharding_unpack():
    from rust_ray_tracing_amd import sharding
    for (w, h, world) in M.UNPACK_SHAPES:
        slots = sharding.packed_pixels(w, h, world)
        src, n_slots = M.unpack_sources(w, h, world)
        assert n_slots == world * slots and len(np.unique(src)) == w * h and src.min() >= 0 and src.max() < n_slots
        packed = np.arange(world * slots * 3, dtype=np.uint32).reshape(world, slots, 3)
        got = M.unpack_model(packed, w, h, world)
        assert np.array_equal(got, sharding.unpack(packed, w, h, world)), (w, h, world)
        # the slots no pixel reads are exactly sharding's padding slots
        pad = np.ones(n_slots, dtype=bool)
        pad[src] = False
        want_pad = np.concatenate([sharding.slot_pixels(w, h, r, world) < 0 for r in range(world)])
        assert np.array_equal(pad, want_pad), (w, h, world)


def test_8bit_windows_straddle_every_code_boundary():
    """All 255 windows (+- 32 ulps around the float64 inverse of the transfer at k / 255) contain inputs of code k - 1 and of code k,
    and of no other code: achieved share 255 of 255 (the float32 boundary lies within [-2, +4] ulps of the window's centre)."""
    win, pixels = M.boundary8()
    assert win.shape == (255, 2 * M.WINDOW8 + 1) and pixels.shape == (255 * (2 * M.WINDOW8 + 1), 3)
    codes = M.rgba8_model(np.repeat(win.reshape(-1, 1), 3, axis=1), 1.0)[:, 0].reshape(win.shape).astype(np.int64)
    k = np.arange(1, 256)[:, None]
    assert np.all((codes == k) | (codes == k - 1))
    assert np.all((codes == k).any(axis=1) & (codes == k - 1).any(axis=1))
    assert np.all(np.diff(codes, axis=1) >= 0)
    # the three channels of a boundary pixel come from three different windows for all but a few k
    got = M.rgba8_model(pixels, 1.0)[:, :3].astype(np.int64)
    assert np.mean((got[:, 0] != got[:, 1]) & (got[:, 1] != got[:, 2]) & (got[:, 0] != got[:, 2])) > 0.95


def test_16bit_windows_straddle_the_code_boundaries(orc):
    """Windows of +- 8 ulps around the float64 bisection of pp(c) * 65535 + 0.5 = k, k = 1 .. 52677 (the code of 1.0, from the oracle):
    achieved share 52 522 of 52 677 windows = 99.71 % contain both code k - 1 and code k (required: 99 %).  +- 4 ulps reaches 93.35 %
    only, because the float32 chain's rounding moves a boundary by several ulps of its argument; +- 16 reaches 100 %."""
    top = M.top_code16()
    assert 52000 < top < 53500
    win, pixels = M.boundary16()
    assert win.shape == (top, 2 * M.WINDOW16 + 1)
    codes = orc.postprocess(np.repeat(win.reshape(-1, 1), 3, axis=1).reshape(1, -1, 3))[0, :, 0].reshape(win.shape).astype(np.int64)
    k = np.arange(1, top + 1)[:, None]
    both = (codes == k).any(axis=1) & (codes == k - 1).any(axis=1)
    print(f"16-bit windows holding both codes: {int(both.sum())} of {top} = {both.mean():.4%}")
    assert both.mean() >= 0.99
    assert np.all(np.abs(codes - k) <= 2)
    assert pixels.shape == (top * (2 * M.WINDOW16 + 1), 3) and pixels.min() > 0 and pixels.max() <= np.float32(1.0000011)


def test_postprocess_statements_agree_on_cpu(orc):
    """The C oracle and the Python reading of pp_compute.wgsl on the specials and a 1-in-64 subsample of the 16-bit boundary pixels."""
    from oracle import pt_oracle_py as py
    px = np.concatenate([M.special_pixels(), M.boundary16()[1][::64]])
    for d in (1.0, 3.0):
        assert np.array_equal(orc.postprocess(px[None], divisor=d)[0, :, :3], py.postprocess_wgsl(px, divisor=d)), d


def test_tiled_pixels_differ_between_neighbours():
    t = M.tiled_pixels()
    assert t.shape == (M.SIZES[-1], 3) and M.SIZES[-1] > 2 * M.GRID_THREADS
    b = t.view(np.uint32)
    assert np.mean(np.any(b[1:] != b[:-1], axis=1)) > 0.99
    assert np.mean((b[:, 0] != b[:, 1]) & (b[:, 1] != b[:, 2])) > 0.99
