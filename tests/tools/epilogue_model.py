"""A second, array-shaped statement of the two frame epilogues and of the shard assembly, and the input sets that pin them.

rgba8_model states cpu.rs:60-64 (divide, linear_to_srgb, floor(x * 255) clamped, [r, g, b, 255]) in numpy float32: one rounded
operation per source operator, no fused multiply-add, powf from the oracle's glibc 2.35 restatement (orc.eval_array op 2, pinned on
every binary32 argument by tests/test_libm_pin.py).  unpack_model states the tile de-interleave as a gather written from the pixel's
side -- for every pixel its (rank, local tile, slot) -- where rust_ray_tracing_amd.sharding.unpack scatters from the slot's side.

The input sets place float32 values on both sides of every output code's boundary: a kernel whose rounding, comparison or constant
differs by one ulp flips a byte there and nowhere else.  Shared by tests/test_epilogue_model.py (CPU) and tests/test_gpu_epilogue.py."""
import functools

import numpy as np

F = np.float32
GRID_THREADS = 2048 * 256                       # the epilogue launches: one grid-stride trip covers this many pixels
SIZES = (1, 2, 255, GRID_THREADS - 1, GRID_THREADS, GRID_THREADS + 1, 1_310_723)   # the last: three trips, ragged tail
WINDOW8 = 32                                    # +- ulps around each 8-bit code boundary
WINDOW16 = 8                                    # +- ulps around each 16-bit code boundary (+- 4 straddles only 93 % of them: the float32
                                                # chain's own rounding moves a boundary by up to ~8 ulps of its argument near the top)
UNPACK_SHAPES = [(1, 1, 1), (1, 1, 5), (7, 9, 2), (8, 8, 1), (9, 8, 3), (61, 37, 3), (64, 40, 2), (17, 129, 7),
                 (16, 16, 8),                   # world larger than the tile count of 4
                 (16, 16, 2),                   # two local tiles on each of two ranks: the smallest shape where rank and local tile can be confused
                 (8, 8, 64), (1000, 531, 5)]    # the last: more pixels than one grid


def _bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


# ---- the models --------------------------------------------------------------------------------------------------------------------
def srgb_model(c):
    """vec3.rs:80-90 with mix (:197-205) on a float32 array."""
    from oracle import orc
    c = np.ascontiguousarray(c, dtype=np.float32)
    with np.errstate(all="ignore"):
        cutoff = np.where(c < F(0.0031308), F(1.0), F(0.0)).astype(np.float32)          # a NaN compares false: cutoff 0
        p = orc.eval_array(2, c.reshape(-1), F(1.0) / F(2.4)).reshape(c.shape)
        higher = F(1.055) * p - F(0.055)
        lower = c * F(12.92)
        return (higher * (F(1.0) - cutoff)) + lower * cutoff


def rgba8_model(hdr, divisor):
    """hdr [..., 3] float32 -> [..., 4] uint8, cpu.rs:60-64."""
    c = np.ascontiguousarray(hdr, dtype=np.float32)
    with np.errstate(all="ignore"):
        if F(divisor) != F(1.0):                                                        # true for a NaN divisor
            c = c / F(divisor)
        q = np.floor(srgb_model(c) * F(255.0))
        q = np.where(q < F(0.0), F(0.0), q)                                             # f32::clamp keeps a NaN ...
        q = np.where(q > F(255.0), F(255.0), q)
        q = np.where(np.isnan(q), F(0.0), q)                                            # ... and `as u8` maps it to 0
    out = np.empty(c.shape[:-1] + (4,), dtype=np.uint8)
    out[..., :3] = q.astype(np.uint8)
    out[..., 3] = 255
    return out


def unpack_sources(width, height, world):
    """For every pixel (row-major) the index of its slot in the all-gathered [world, packed_pixels] array."""
    tiles_x, tiles_y = -(-width // 8), -(-height // 8)
    n_local = -(-(tiles_x * tiles_y) // world)                                          # local tiles per rank, the last rank(s) may hold fewer
    py, px = np.divmod(np.arange(width * height, dtype=np.int64), width)
    tile = (py // 8) * tiles_x + px // 8                                                # tiles are dealt round-robin to the ranks
    rank, local = tile % world, tile // world
    return (rank * n_local + local) * 64 + (py % 8) * 8 + px % 8, world * n_local * 64


def unpack_model(packed_all, width, height, world):
    """[world, packed_pixels, C] -> [height * width, C]."""
    src, n_slots = unpack_sources(width, height, world)
    packed_all = np.asarray(packed_all)
    flat = packed_all.reshape((-1,) + packed_all.shape[2:])
    assert len(flat) == n_slots
    return flat[src]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def specials():
    one, cut = F(1.0), F(0.0031308)
    down, up = F(-np.inf), F(np.inf)
    v = [F(0.0), F(-0.0), _bits([1])[0], _bits([0x00800000])[0],                        # +-0, the smallest denormal, FLT_MIN
         np.nextafter(cut, down), cut, np.nextafter(cut, up), np.nextafter(one, down), one, np.nextafter(one, up),
         F(7.5), _bits([0x7F7FFFFF])[0], up, down, _bits([0x7FC12345])[0], _bits([0xFFC00001])[0], F(-0.5), F(-1e-30)]
    return np.array(v, dtype=np.float32)


def special_pixels():
    """Every special in every channel position (the other two channels hold mid-range values), then three specials per pixel."""
    s = specials()
    rows = []
    for pos in range(3):
        px = np.empty((len(s), 3), dtype=np.float32)
        px[:] = (F(0.25), F(0.5), F(0.125))
        px[:, pos] = s
        rows.append(px)
    rows.append(np.stack([s, np.roll(s, 5), np.roll(s, 11)], axis=1))
    return np.concatenate(rows)


@functools.lru_cache(maxsize=None)
def centres8():
    """centres8()[k - 1]: the float32 nearest the linear value whose sRGB transfer times 255 is k, k = 1 .. 255 (float64 inverse)."""
    s = np.arange(1, 256, dtype=np.float64) / 255.0
    lin = s / 12.92
    c = np.where(lin < 0.0031308, lin, ((s + 0.055) / 1.055) ** 2.4)
    return c.astype(np.float32)


def _windows(centres, ulps):
    """[n, 2 * ulps + 1] float32: every value within +- ulps of each (positive, normal) centre."""
    b = centres.view(np.uint32).astype(np.int64)[:, None] + np.arange(-ulps, ulps + 1, dtype=np.int64)[None, :]
    return b.astype(np.uint32).view(np.float32)


def _decorrelate(win):
    """Windows [n, m] for codes 1 .. n -> pixels [n * m, 3] whose three channels sit in three different windows (k, n + 1 - k and
    (7 k) mod n + 1 -- three distinct codes for most k), so a swapped or misplaced channel changes the expected bytes."""
    n = len(win)
    k = np.arange(1, n + 1)
    return np.stack([win[k - 1], win[n - k], win[(k * 7) % n]], axis=2).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def boundary8():
    """(windows [255, 65], pixels [255 * 65, 3])."""
    win = _windows(centres8(), WINDOW8)
    return win, _decorrelate(win)


def pp_float64(c):
    """pp_compute.wgsl's channel in float64 (placing windows only, never an expected value)."""
    c = np.clip(np.asarray(c, dtype=np.float64), 0.0, 1.0)
    x = np.where(c < 0.0031308, c * 12.92, 1.055 * c ** (1.0 / 2.4) - 0.055)
    y = (x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)
    return np.clip(y, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def centres16(top):
    """centres16(top)[k - 1]: float32 nearest the c in [0, 1] with pp(c) * 65535 + 0.5 = k, k = 1 .. top, by bisection in float64."""
    k = np.arange(1, top + 1, dtype=np.float64)
    lo, hi = np.zeros_like(k), np.ones_like(k)
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        below = pp_float64(mid) * 65535.0 + 0.5 < k
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return (0.5 * (lo + hi)).astype(np.float32)


def top_code16():
    """The largest reachable 16-bit code: that of 1.0 (ACES of sRGB(1) is about 0.804), from the oracle."""
    from oracle import orc
    return int(orc.postprocess(np.ones((1, 1, 3), dtype=np.float32))[0, 0, 0])


@functools.lru_cache(maxsize=None)
def boundary16(ulps=WINDOW16):
    """(windows [top, 2 * ulps + 1], pixels [top * (2 * ulps + 1), 3])."""
    win = _windows(centres16(top_code16()), ulps)
    return win, _decorrelate(win)


@functools.lru_cache(maxsize=None)
def pool():
    """The values large buffers are tiled from: the 8-bit windows, every 16-bit centre and the specials."""
    return np.concatenate([boundary8()[0].reshape(-1), centres16(top_code16()), specials()])


@functools.lru_cache(maxsize=None)
def tiled_pixels(n_pixels=SIZES[-1]):
    """[n_pixels, 3]: the pool tiled with a per-pixel rotation -- the channels walk the pool at three different strides and every pass
    over it shifts by one, so neighbouring pixels and the three channels of a pixel differ.  A prefix serves a smaller size."""
    v = pool()
    i = np.arange(n_pixels, dtype=np.int64)[:, None]
    idx = (i * np.array([1, 3, 7]) + np.array([0, len(v) // 3, 2 * len(v) // 3]) + i // len(v)) % len(v)
    return v[idx]
