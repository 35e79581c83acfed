"""A second reading of the nearest-texel lookup of the default shading path (Texture::color_at, reference src/texture.rs:33-38, then
the division by 255 of vec3.rs:252-260), in numpy, written from the reference's text and not from the kernel's or the oracle's:

* f32::fract(u) is u - trunc(u), in f32 (so fract(+-inf) is NaN and the sign of u survives);
* the two products fract * width and fract * height are f32 products;
* `as i32` is Rust's saturating cast: NaN -> 0, values beyond the i32 range -> the nearest end, everything else truncated to zero;
* the index i + j * width and the decision whether it lies in [0, width * height) are made in int64 (the reference panics outside;
  the oracle and the kernels clamp to the nearest end and count the lookup in tex_clamped);
* a channel is np.float32(c) / np.float32(255).

tests/test_texel_model.py holds this model to the oracle (orc_texture_color_at); tests/test_gpu_texel.py compares the device
function (csrc/pt_texel.h, through mipt_debug_texel) with it bit for bit.  Also here: the coordinate lists those tests sweep."""
import numpy as np

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
MAX_SQUARE = 1 << 25                # pairs in a full square of the edge list (edge_pairs); the probe takes 2^26 per call
SHAPES = ((1, 1), (1, 7), (7, 1), (3, 5), (16, 16), (255, 3), (1024, 2))          # (width, height)


def _sat_i32(f):
    """Rust `f as i32` on an f32 array -> int64"""
    f = np.asarray(f, dtype=np.float32)
    out = np.zeros(f.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        ok = ~np.isnan(f)
        hi, lo = ok & (f >= np.float32(2147483648.0)), ok & (f <= np.float32(-2147483648.0))
        mid = ok & ~hi & ~lo
        out[mid] = np.trunc(f[mid]).astype(np.int64)
    out[hi], out[lo] = I32_MAX, I32_MIN
    return out


def lookup_index(u, v, width, height):
    """-> (texel index into the w*h texture after the clamp [n] int64, clamped flags [n] bool, the unclamped index [n] int64)"""
    u, v = np.asarray(u, dtype=np.float32), np.asarray(v, dtype=np.float32)
    with np.errstate(all="ignore"):
        fu, fv = u - np.trunc(u), v - np.trunc(v)
        fi, fj = fu * np.float32(width), fv * np.float32(height)
    assert fi.dtype == np.float32 and fj.dtype == np.float32
    i, j = _sat_i32(fi), _sat_i32(fj)
    raw = i + j * np.int64(width)
    n = np.int64(width) * np.int64(height)
    clamped = (raw < 0) | (raw >= n)
    return np.clip(raw, 0, n - 1), clamped, raw


def texel_rgb(pool, offset, width, height, u, v):
    """pool: the texel pool as uint32 words (packed RGBA8, R in the low byte); the texture is words [offset, offset + w*h), rows of w.
    -> (rgb [n,3] f32, number of clamped lookups, the index into the texture of every lookup [n] int64)"""
    pool = np.asarray(pool, dtype=np.uint32).reshape(-1)
    idx, clamped, _ = lookup_index(u, v, width, height)
    px = pool[np.int64(offset) + idx]
    rgb = np.stack([(px >> np.uint32(s)) & np.uint32(255) for s in (0, 8, 16)], axis=1).astype(np.float32) / np.float32(255)
    return rgb, int(clamped.sum()), idx


# ---- what the tests sweep ---------------------------------------------------------------------------------------------------------
def special_coords():
    """+-0, the smallest subnormal, a tiny normal, the neighbours of +-1, +-1, the integers' end of f32 (2^23, 2^24), values beyond
    the i32 range, the infinities and NaN"""
    one_below = np.nextafter(np.float32(1), np.float32(0))
    pos = [0.0, 1e-45, 1e-30, one_below, 1.0, 2.0 ** 23, 2.0 ** 24, 1e9, 3e38, np.inf]
    return np.array(pos + [-x for x in pos] + [np.nan], dtype=np.float32)


def _with_neighbours(x):
    x = np.asarray(x, dtype=np.float32)
    return np.concatenate([x, np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf))])


def boundary_coords(d, every=True):
    """k / d for k over three periods of both signs (k = -3d .. 3d), each with its two f32 neighbours.  every = False keeps, of a
    dimension above 16, only the k within 2 of a period's end (k = m d + {-2 .. 2}) and 8 evenly spaced ones inside each period."""
    k = np.arange(-3 * d, 3 * d + 1)
    if not every and d > 16:
        near = (np.abs(((k + d // 2) % d) - d // 2) <= 2) | ((k % d) % max(d // 8, 1) == 0)
        k = k[near]
    return _with_neighbours(k.astype(np.float32) / np.float32(d))


def edge_pairs(width, height):
    """The edge coordinates as (u, v) pairs.  The list is L = boundaries of both dimensions + the specials, and the pairs are
    L x L wherever that square has at most MAX_SQUARE pairs: every shape of SHAPES but 1024x2 (255x3: 2.2e7 pairs).  A dimension d
    puts 18 d + 3 entries into L, and at d = 1024 the square is 3.4e8 pairs -- above what the probe takes in one call (2^26) and
    far beyond a test of a few seconds.  There, and only there, the square is taken of the thinned list
    (boundary_coords(every=False)) and EVERY boundary coordinate is still paired, as u and as v, with every special: i depends on u
    alone and j on v alone, so no boundary value goes untested on either axis, and the products of the two (index, clamp) are
    covered by the thinned square."""
    spec = special_coords()
    full = np.unique(np.concatenate([boundary_coords(width), boundary_coords(height)]))
    if (len(full) + len(spec)) ** 2 <= MAX_SQUARE:
        both = np.concatenate([full, spec])
        gu, gv = np.meshgrid(both, both)
        return np.ascontiguousarray(gu.reshape(-1)), np.ascontiguousarray(gv.reshape(-1))
    thin = np.unique(np.concatenate([boundary_coords(width, False), boundary_coords(height, False)]))
    thin = np.concatenate([thin, spec])                                        # np.unique would fold NaN / +-0: keep the specials as they are
    gu, gv = np.meshgrid(thin, thin)
    us, vs = [gu.reshape(-1)], [gv.reshape(-1)]
    a, b = np.meshgrid(full, spec)
    us += [a.reshape(-1), b.reshape(-1)]
    vs += [b.reshape(-1), a.reshape(-1)]
    return np.concatenate(us).astype(np.float32), np.concatenate(vs).astype(np.float32)


def random_pairs(width, height, n=1 << 20):
    """(n pairs uniform in (-4, 4), n pairs of random binary32 bit patterns) as one (u, v)"""
    rng = np.random.default_rng(width * 4096 + height)
    a = rng.uniform(-4.0, 4.0, (n, 2)).astype(np.float32)
    b = rng.integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(np.uint32).view(np.float32)
    uv = np.concatenate([a, b])
    return np.ascontiguousarray(uv[:, 0]), np.ascontiguousarray(uv[:, 1])


def guarded_pool(width, height, seed=0):
    """A texture inside a pool, between guards: -> (pool words, offset, the texture as (h, w, 4) uint8).  The texture's texels are
    distinct from one another where 2^24 colours allow (they do, at these sizes) and every guard word's RGB differs from every
    texel's, so a lookup that leaves the texture, or starts from a wrong offset, returns a colour the model does not."""
    rng = np.random.default_rng(1000 + width * 4096 + height + seed)
    n = width * height
    rgb = rng.permutation(1 << 16)[:n].astype(np.uint32) * np.uint32(2)         # even 17-bit codes: distinct texels
    alpha = rng.integers(0, 256, n, dtype=np.uint32)
    tex_words = rgb | (alpha << np.uint32(24))
    n_pre, n_post = 5 + (width % 3), 7 + (height % 5)
    guard = (rng.permutation(1 << 16)[: n_pre + n_post].astype(np.uint32) * np.uint32(2) + np.uint32(1)) | np.uint32(0xFF000000)   # odd codes
    pool = np.concatenate([guard[:n_pre], tex_words, guard[n_pre:]]).astype(np.uint32)
    tex = tex_words.view(np.uint8).reshape(height, width, 4).copy()
    return pool, n_pre, tex


def coverage(u, v, width, height):
    """The classes a sweep must reach (computed from the model, before anything is launched)"""
    idx, clamped, _ = lookup_index(u, v, width, height)
    with np.errstate(all="ignore"):
        neg = (u < 0) | (v < 0)
    return dict(clamped=int(clamped.sum()), negative_unclamped=int((neg & ~clamped).sum()), first=int((idx == 0).sum()),
                last=int((idx == width * height - 1).sum()), lo=int(idx.min()), hi=int(idx.max()))
