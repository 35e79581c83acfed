"""-m gpu: the kernels of the timed frame other than the trace kernel -- tonemap_kernel, postprocess_kernel, unpack_tiles_kernel,
divide_kernel, popcount_kernel -- each against a plain CPU statement of the same operation, bit for bit (floats as u32 patterns,
NaN equal to NaN; integers exactly; nothing has a tolerance).

The inputs come from tests/tools/epilogue_model.py: float32 values on both sides of every output code's boundary, the specials
(zeros, denormals, the sRGB cut-off and 1.0 with their neighbours, huge, infinite, NaN, negative), three different windows in the
three channels of a pixel, and buffer sizes around and beyond one grid of 2048 x 256 threads.  Every output buffer carries 256
trailing canary bytes that must survive, and every call runs under two different prefills of the output, which must give the same
bytes: no output byte is left over from the prefill, none is written past the end."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import epilogue_model as M  # noqa: E402

CANARY, TAIL = 0x5C, 256
PREFILLS = (0x00, 0xA7)
DIVISORS = [1.0, 3.0, 7.0, 8.0, 64.0]                       # 1.0: the branch that skips the division
PREMULTIPLIED = [8.0, 2.0 ** -20, 2.0 ** -126]              # inputs x * d, so that the quotients land on the boundary set again


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _epilogue(entry, hdr, divisor, bytes_per_pixel, side_stream=False):
    """entry(d_hdr, n_pixels, divisor, d_out, stream) under both prefills -> the n_pixels * bytes_per_pixel output bytes."""
    import torch
    hdr = np.ascontiguousarray(hdr, dtype=np.float32).reshape(-1, 3)
    n, n_out = len(hdr), len(hdr) * bytes_per_pixel
    d_hdr = torch.from_numpy(hdr.reshape(-1).view(np.int32)).cuda()       # as integers: payloads of NaNs travel untouched
    stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
    outs = []
    for fill in PREFILLS:
        d_out = torch.full((n_out + TAIL,), fill, dtype=torch.uint8, device="cuda")
        d_out[n_out:] = CANARY
        torch.cuda.synchronize()                                             # the fills are done before another stream writes
        rc = entry(_vp(d_hdr), n, float(divisor), _vp(d_out), C.c_void_p(stream.cuda_stream))
        assert rc == 0, rc
        stream.synchronize()
        host = d_out.cpu().numpy()
        assert np.all(host[n_out:] == CANARY), "wrote past the end of the output"
        outs.append(host[:n_out].copy())
    assert np.array_equal(outs[0], outs[1]), "an output byte depends on the buffer's previous content"
    return outs[0]


def _first_diff(got, want, per_pixel):
    bad = np.flatnonzero(got != want)
    return f"{len(bad)} of {got.size} values differ, first at pixel {bad[0] // per_pixel} channel {bad[0] % per_pixel}: {got[bad[0]]} != {want[bad[0]]}" if len(bad) else ""


def _check8(rrt, hdr, divisor, side_stream=False, want=None):
    hdr = np.ascontiguousarray(hdr, dtype=np.float32).reshape(-1, 3)
    got = _epilogue(rrt.load().mipt_tonemap_device, hdr, divisor, 4, side_stream)
    want = (M.rgba8_model(hdr, divisor) if want is None else want).reshape(-1)
    assert np.array_equal(got, want), (divisor, _first_diff(got, want, 4))
    return want.reshape(-1, 4)


def _check16(rrt, orc, hdr, divisor, side_stream=False, want=None):
    hdr = np.ascontiguousarray(hdr, dtype=np.float32).reshape(-1, 3)
    got = _epilogue(rrt.load().mipt_postprocess_device, hdr, divisor, 8, side_stream).view(np.uint16)
    want = (orc.postprocess(hdr[None], divisor=divisor)[0] if want is None else want).reshape(-1)
    assert np.array_equal(got, want), (divisor, _first_diff(got, want, 4))
    assert np.all(got.reshape(-1, 4)[:, 3] == 65535)
    return want.reshape(-1, 4)


def _pixels8():
    return np.concatenate([M.boundary8()[1], M.special_pixels()])


def _pixels16():
    return np.concatenate([M.boundary16()[1], M.special_pixels()])


@functools.lru_cache(maxsize=None)
def _tiled_want8(divisor):
    return M.rgba8_model(M.tiled_pixels(), divisor)


@functools.lru_cache(maxsize=None)
def _tiled_want16(divisor):
    from oracle import orc
    return orc.postprocess(M.tiled_pixels()[None], divisor=divisor)[0]


# ---- a. mipt_tonemap_device against rgba8_model ----------------------------------------------------------------------------------
@pytest.mark.parametrize("divisor", DIVISORS)
def test_tonemap_code_boundaries_and_specials(rrt, divisor):
    want = _check8(rrt, _pixels8(), divisor)
    if divisor == 1.0:
        assert len(np.unique(want[:, :3])) == 256                          # both sides of all 255 boundaries are in the expected bytes
        assert np.mean((want[:, 0] != want[:, 1]) & (want[:, 1] != want[:, 2]) & (want[:, 0] != want[:, 2])) > 0.9   # a channel swap shows


def _premultiplied(pixels, divisor):
    """pixels * divisor, and the number of leading boundary pixels whose quotients are the boundary set itself (all of them where
    the product is exact, none under 2^-126)."""
    with np.errstate(all="ignore"):
        hdr = pixels * np.float32(divisor)
        back = hdr / np.float32(divisor)
    n = len(pixels) - len(M.special_pixels())                              # the boundary pixels; the specials go along as they come out
    exact = bool(np.array_equal(back[:n].view(np.uint32), pixels[:n].view(np.uint32)))
    assert exact == (divisor != 2.0 ** -126)
    if not exact:                                                          # 2^-126: the products are non-zero denormals (normal from 1.0 up)
        assert np.all(hdr[:n] > 0) and np.mean(hdr[:n] < np.float32(2.0 ** -126)) > 0.99
    return hdr, n if exact else 0


@pytest.mark.parametrize("divisor", PREMULTIPLIED)
def test_tonemap_quotients_on_the_code_boundaries(rrt, divisor):
    """x * d is exact for d = 8 and 2^-20: the quotients are the boundary set again.  Under d = 2^-126 the products are denormal and
    keep fewer bits the smaller x is, so the quotients only land near the boundaries -- what is tested there is that a denormal
    dividend is neither flushed nor scaled.  Either way the quotient must be the IEEE one, not a product with a reciprocal."""
    hdr, n_exact = _premultiplied(_pixels8(), divisor)
    want = _check8(rrt, hdr, divisor)
    assert np.array_equal(want[:n_exact], M.rgba8_model(_pixels8()[:n_exact], 1.0))


@pytest.mark.parametrize("divisor", [0.0, float("nan")])
def test_tonemap_zero_and_nan_divisor(rrt, divisor):
    hdr = np.concatenate([M.special_pixels(), M.boundary8()[1][::97]])
    want = _check8(rrt, hdr, divisor)
    assert not want[:, :3].any() and np.all(want[:, 3] == 255)             # x / 0 and x / NaN are infinite or NaN: byte 0 by the model


@pytest.mark.parametrize("n_pixels", M.SIZES)
def test_tonemap_sizes(rrt, n_pixels):
    for divisor in (1.0, 3.0):
        _check8(rrt, M.tiled_pixels()[:n_pixels], divisor, want=_tiled_want8(divisor)[:n_pixels])


def test_tonemap_on_a_side_stream(rrt):
    n = M.GRID_THREADS + 1
    _check8(rrt, M.tiled_pixels()[:n], 3.0, side_stream=True, want=_tiled_want8(3.0)[:n])
    _check8(rrt, _pixels8(), 1.0, side_stream=True)


# ---- b. mipt_postprocess_device against orc.postprocess ----------------------------------------------------------------------------
@pytest.mark.parametrize("divisor", DIVISORS)
def test_postprocess_code_boundaries_and_specials(rrt, orc, divisor):
    want = _check16(rrt, orc, _pixels16(), divisor)
    if divisor == 1.0:
        top = M.top_code16()
        assert len(np.unique(want[:, :3])) == top + 1                      # every reachable code, 0 .. top


@pytest.mark.parametrize("divisor", PREMULTIPLIED)
def test_postprocess_quotients_on_the_code_boundaries(rrt, orc, divisor):
    hdr, n_exact = _premultiplied(_pixels16(), divisor)
    want = _check16(rrt, orc, hdr, divisor)
    assert np.array_equal(want[:n_exact], orc.postprocess(_pixels16()[None, :n_exact])[0])


@pytest.mark.parametrize("divisor", [0.0, float("nan")])
def test_postprocess_zero_and_nan_divisor(rrt, orc, divisor):
    _check16(rrt, orc, np.concatenate([M.special_pixels(), M.boundary16()[1][::9973]]), divisor)


@pytest.mark.parametrize("n_pixels", M.SIZES)
def test_postprocess_sizes(rrt, orc, n_pixels):
    for divisor in (1.0, 3.0):
        _check16(rrt, orc, M.tiled_pixels()[:n_pixels], divisor, want=_tiled_want16(divisor)[:n_pixels])


def test_postprocess_on_a_side_stream(rrt, orc):
    n = M.GRID_THREADS + 1
    _check16(rrt, orc, M.tiled_pixels()[:n], 3.0, side_stream=True, want=_tiled_want16(3.0)[:n])


def test_postprocess_clamp_and_three_statements(rrt, orc):
    """The rt texture clamps radiance to [0, 1] before the pass: everything below 0 gives exactly the code of 0, everything above 1
    exactly the code of 1.  And the kernel, the C oracle and the Python reading of pp_compute.wgsl agree on the specials and on a
    1-in-64 subsample of the boundary pixels."""
    from oracle import pt_oracle_py as py
    code0, code1 = (int(orc.postprocess(np.full((1, 1, 3), v, dtype=np.float32))[0, 0, 0]) for v in (0.0, 1.0))
    assert code0 == 0 and code1 == M.top_code16()
    lo = np.float32([-0.0, -1e-45, -1e-30, -0.5, -1.0, -3e38, -np.inf])
    hi = np.float32([np.nextafter(np.float32(1), np.float32(2)), 1.5, 7.5, 65504.0, 3.4028235e38, np.inf])
    vals = np.concatenate([lo, hi])
    hdr = np.stack([vals, np.roll(vals, 1), np.roll(vals, 2)], axis=1)
    got = _epilogue(rrt.load().mipt_postprocess_device, hdr, 1.0, 8).view(np.uint16).reshape(-1, 4)
    assert np.array_equal(got[:, :3], np.where(hdr <= 0, code0, code1))
    px = np.concatenate([M.special_pixels(), M.boundary16()[1][::64]])
    for divisor in (1.0, 3.0):
        want = _check16(rrt, orc, px, divisor)
        assert np.array_equal(want[:, :3], py.postprocess_wgsl(px, divisor=divisor)), divisor


# ---- c. mipt_unpack_tiles against unpack_model -------------------------------------------------------------------------------------
PAD_WORD = 0xDEADBEEF                                                      # in the padding slots; must not reach the frame


@pytest.mark.parametrize("w,h,world", M.UNPACK_SHAPES)
def test_unpack_tiles_is_the_models_permutation(rrt, w, h, world):
    """Every input word is unique (a swap of two pixels of equal radiance cannot hide), some are NaNs with payloads and some are
    denormals (the copy must preserve the bits), the padding slots hold a word of their own."""
    import torch
    from rust_ray_tracing_amd import _lib as L
    from rust_ray_tracing_amd import sharding
    lib = rrt.load()
    slots = int(lib.mipt_packed_pixels(w, h, world))
    src, n_slots = M.unpack_sources(w, h, world)
    assert n_slots == world * slots
    n_out = w * h * 3
    j = np.arange(n_slots * 3, dtype=np.uint32)
    assert j[-1] < (1 << 22)
    for pattern in (j ^ np.uint32(0x7FC00000), j):                         # quiet NaNs with payload j / denormals (and +0 once)
        packed = pattern.reshape(n_slots, 3).copy()
        pad = np.ones(n_slots, dtype=bool)
        pad[src] = False
        packed[pad] = PAD_WORD
        want = M.unpack_model(packed.reshape(world, slots, 3), w, h, world).reshape(-1)
        assert not np.any(want == PAD_WORD) and len(np.unique(want)) == n_out
        assert np.array_equal(want, sharding.unpack(packed.reshape(world, slots, 3), w, h, world).reshape(-1))   # the third opinion
        d_in = torch.from_numpy(packed.reshape(-1).view(np.int32)).cuda()
        outs = []
        for fill in PREFILLS:
            d_out = torch.full((n_out * 4 + TAIL,), fill, dtype=torch.uint8, device="cuda")
            d_out[n_out * 4:] = CANARY
            L.check(lib.mipt_unpack_tiles(_vp(d_in), w, h, world, _vp(d_out), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "mipt_unpack_tiles")
            torch.cuda.synchronize()
            host = d_out.cpu().numpy()
            assert np.all(host[n_out * 4:] == CANARY)
            outs.append(host[:n_out * 4].view(np.uint32).copy())
        assert np.array_equal(outs[0], outs[1])
        bad = np.flatnonzero(outs[0] != want)
        assert len(bad) == 0, (w, h, world, len(bad), int(bad[0]) // 3)


def test_unpack_tiles_rejects_invalid_arguments(rrt):
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    w, h, world = 9, 8, 3
    d_in = torch.zeros(int(lib.mipt_packed_pixels(w, h, world)) * world * 3, dtype=torch.float32, device="cuda")
    d_out = torch.full((w * h * 3 * 4 + TAIL,), 0xA7, dtype=torch.uint8, device="cuda")
    for args in ((None, w, h, world, _vp(d_out)), (_vp(d_in), w, h, world, None), (_vp(d_in), 0, h, world, _vp(d_out)),
                 (_vp(d_in), w, 0, world, _vp(d_out)), (_vp(d_in), w, h, 0, _vp(d_out))):
        assert lib.mipt_unpack_tiles(*args, None) == L.ERR_INVALID_ARG, args[1:4]
    torch.cuda.synchronize()
    assert bool((d_out == 0xA7).all())


# ---- d. divide_kernel and popcount_kernel through the diagnostic library -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _divide_inputs():
    """The input set of test_device_arithmetic_matches_oracle: 400 000 values over 80 binades of both signs, and the specials."""
    rng = np.random.default_rng(1)
    n = 400_000
    a = (rng.standard_normal(n) * np.exp(rng.uniform(-40, 40, n))).astype(np.float32)
    a[:8] = [0, -0.0, np.inf, -np.inf, np.nan, 1, 1e-45, 3e38]
    return a


@pytest.mark.parametrize("n_floats", [1, 400_000, M.GRID_THREADS * 3 + 1])
def test_divide_kernel_is_the_ieee_quotient_in_place(rrt, n_floats):
    import torch
    diag = rrt.load_diag()
    base = _divide_inputs()
    a = np.resize(base, n_floats) if n_floats > 1 else np.float32([4e38 / 3])
    with np.errstate(all="ignore"):
        a = a * np.exp2(np.arange(n_floats) // len(base)).astype(np.float32) * np.float32(0.75)    # every pass over the set: other values
    tail = 64
    for divisor in (3.0, 7.0, 64.0, 1.0):
        buf = np.concatenate([a, np.full(tail, 123.0, dtype=np.float32)])
        d = torch.from_numpy(buf.view(np.int32)).cuda()
        assert diag.mipt_debug_divide(_vp(d), n_floats, divisor, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, diag.mipt_diag_last_error()
        torch.cuda.synchronize()
        got = d.cpu().numpy().view(np.float32)
        with np.errstate(all="ignore"):
            want = a / np.float32(divisor)
        assert np.all(got[n_floats:] == np.float32(123.0))
        same = (got[:n_floats].view(np.uint32) == want.view(np.uint32)) | (np.isnan(got[:n_floats]) & np.isnan(want))
        assert same.all(), (divisor, int((~same).sum()), int(np.flatnonzero(~same)[0]))
    assert diag.mipt_debug_divide(None, 4, 2.0, None) == -1 and diag.mipt_debug_divide(_vp(d), 0, 2.0, None) == -1


def _bit_count(words):
    return int.from_bytes(words.tobytes(), "little").bit_count()           # Python's exact integer arithmetic


@pytest.mark.parametrize("n_words", [1, 63, 64, 65, 262_143, 262_144, 262_145, 1_048_579])   # the grid is 1024 x 256 = 262 144 threads
def test_popcount_kernel_counts_exactly(rrt, n_words):
    import torch
    diag = rrt.load_diag()
    rng = np.random.default_rng(n_words)
    sparse = np.zeros(n_words, dtype=np.uint32)
    sparse[rng.integers(0, n_words, max(1, n_words // 1000))] = np.uint32(1) << rng.integers(0, 32, max(1, n_words // 1000)).astype(np.uint32)
    bitmaps = {"random": rng.integers(0, 2 ** 32, n_words, dtype=np.uint64).astype(np.uint32), "zero": np.zeros(n_words, dtype=np.uint32),
               "ones": np.full(n_words, 0xFFFFFFFF, dtype=np.uint32), "sparse": sparse}
    for name, words in bitmaps.items():
        d_words = torch.from_numpy(np.concatenate([words, np.full(64, 0xFFFFFFFF, dtype=np.uint32)]).view(np.int32)).cuda()   # set bits past the end
        for preset in (0, 5):                                              # the kernel adds to the counter
            out = np.full(33, 0x5C5C5C5C5C5C5C5C, dtype=np.uint64)
            out[0] = preset
            d_out = torch.from_numpy(out.view(np.int64)).cuda()
            assert diag.mipt_debug_popcount(_vp(d_words), n_words, _vp(d_out), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            torch.cuda.synchronize()
            got = d_out.cpu().numpy().view(np.uint64)
            assert np.all(got[1:] == np.uint64(0x5C5C5C5C5C5C5C5C))
            assert int(got[0]) == preset + _bit_count(words), (name, preset, int(got[0]))
        if name == "ones":
            assert _bit_count(words) == n_words * 32                       # at 1 048 579 words: 33 554 528, through the 64-bit accumulation
    assert diag.mipt_debug_popcount(None, 4, _vp(d_out), None) == -1 and diag.mipt_debug_popcount(_vp(d_words), 4, None, None) == -1
    assert diag.mipt_debug_popcount(_vp(d_words), 0, _vp(d_out), None) == -1
