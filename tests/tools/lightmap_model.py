"""The models of include/mipt.h "lightmap finishing" and of mipt_bake_surface, in numpy float32 over host arrays.  Written from the
header's text: one rounded f32 operation per operator, in the order written; expf is the oracle's restatement of glibc 2.35's
(orc.eval_array(17, .)); a tap outside the atlas or on an uncovered texel is not added at all.  filter() and dilate() are
vectorised over the atlas; filter_scalar() and dilate_scalar() state the same text a second time as a plain loop over every texel
and tap (tests/test_lightmap_model.py holds the two to each other).  Nothing comes from the library under test."""
import numpy as np

from bake_model import FRONT, NONE, POINT, _normalized, surface

F = np.float32
H5 = [F(1.0 / 16.0), F(1.0 / 4.0), F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0)]
EXPF = 17
MAX_RADIUS = 64


# ---- mipt_bake_surface -------------------------------------------------------------------------------------------------------------
def surface_all(tris, points, unit=False):
    """position, normal [n, 3] f32 of the points on the caller's triangles: bake_model.surface per point, normalized(N) with `unit`
    (a zero N gives NaNs), +0 for a point without a surface"""
    n = len(points)
    pos, nrm = np.zeros((n, 3), dtype=F), np.zeros((n, 3), dtype=F)
    with np.errstate(all="ignore"):
        for i in range(n):
            if int(points["prim"][i]) == NONE:
                continue
            P, N = surface(tris, points[i])
            pos[i], nrm[i] = P, (_normalized(N) if unit else N)
    return pos, nrm


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
def points_of(covered):
    """the records mipt_bake_texels would write for a coverage mask [H, W]: seed = the index, prim = triangle 0's front or NONE"""
    cov = np.asarray(covered, dtype=bool).reshape(-1)
    pts = np.zeros(len(cov), dtype=POINT)
    pts["seed"] = np.arange(len(cov), dtype=np.uint32)
    pts["prim"] = np.where(cov, np.uint32(FRONT), np.uint32(NONE))
    return pts


def covered_of(points, height, width):
    return (np.asarray(points)["prim"] != NONE).reshape(height, width)


def constants(iterations, sigma_color, sigma_normal, sigma_plane, sigma_distance):
    """(kc_i, kn, kl, kd_i) as the host forms them in f32"""
    with np.errstate(all="ignore"):
        kc, kd = [], []
        for i in range(iterations):
            sc = F(sigma_color) * F(2.0 ** -i)
            kc.append(F(1.0) / (sc * sc))
            sd = F(sigma_distance) * F(2.0 ** i)
            kd.append(F(1.0) / (sd * sd))
        return kc, F(1.0) / (F(sigma_normal) * F(sigma_normal)), F(1.0) / (F(sigma_plane) * F(sigma_plane)), kd


def _sq3(d):
    return ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])


def _dot3(a, b):
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


# ---- the filter --------------------------------------------------------------------------------------------------------------------
def _iteration(orc, c, cov, position, normal, step, kc, kn, kl, kd):
    h, w, _ = c.shape
    s = np.zeros_like(c)                                           # sum_ch, from +0
    wsum = np.zeros((h, w), dtype=F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = dy * step, dx * step
            y0, y1 = max(0, -oy), min(h, h - oy)                   # the texels p whose tap q = p + (ox, oy) lies inside the atlas
            x0, x1 = max(0, -ox), min(w, w - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
            hk = H5[dy + 2] * H5[dx + 2]
            cq = c[Q]
            take = cov[P] & cov[Q]                                  # an uncovered tap is skipped; an uncovered centre keeps its words
            if dy == 0 and dx == 0:
                wt = np.full(cq.shape[:-1], hk, dtype=F)            # the centre: 9/64 without evaluation
            else:
                e = _sq3(c[P] - cq) * kc
                if normal is not None:
                    e = e + (_sq3(normal[P] - normal[Q]) * kn)
                if position is not None:
                    D = position[Q] - position[P]
                    if normal is not None:
                        l = _dot3(normal[P], D)
                        e = e + ((l * l) * kl)
                    e = e + (_sq3(D) * kd)
                e = np.where(e < F(128.0), e, F(128.0)).astype(F)   # a NaN gives 128
                wt = hk * orc.eval_array(EXPF, -e).reshape(e.shape)
            s[P] = np.where(take[..., None], s[P] + (wt[..., None] * cq), s[P])
            wsum[P] = np.where(take, wsum[P] + wt, wsum[P])
    ok = cov & (wsum > F(0.0))
    safe = np.where(ok, wsum, F(1.0))
    out = c.copy()
    new = (s / safe[..., None]).astype(F)
    out[ok] = new[ok]
    return out


def filter(orc, radiance, covered, position=None, normal=None, iterations=5, sigma_color=4.0, sigma_normal=0.5, sigma_plane=0.05,
           sigma_distance=0.5):
    """radiance [H,W,3] f32, covered [H,W] bool and the optional guides [H,W,3] -> the filtered atlas [H,W,3]"""
    c = np.array(radiance, dtype=F, copy=True)
    h, w, _ = c.shape
    cov = np.asarray(covered, dtype=bool).reshape(h, w)
    position = None if position is None else np.asarray(position, dtype=F).reshape(h, w, 3)
    normal = None if normal is None else np.asarray(normal, dtype=F).reshape(h, w, 3)
    assert 1 <= iterations <= 8
    kc, kn, kl, kd = constants(iterations, sigma_color, sigma_normal, sigma_plane, sigma_distance)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            c = _iteration(orc, c, cov, position, normal, 1 << i, kc[i], kn, kl, kd[i])
    return c


def _expf1(orc, x):
    return F(orc.eval_array(EXPF, np.array([x], dtype=F))[0])


def filter_scalar(orc, radiance, covered, position=None, normal=None, iterations=5, sigma_color=4.0, sigma_normal=0.5, sigma_plane=0.05,
                  sigma_distance=0.5):
    """filter() as a plain loop over every texel and tap"""
    c = np.array(radiance, dtype=F, copy=True)
    h, w, _ = c.shape
    cov = np.asarray(covered, dtype=bool).reshape(h, w)
    kc, kn, kl, kd = constants(iterations, sigma_color, sigma_normal, sigma_plane, sigma_distance)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            step, new = 1 << i, c.copy()
            for y in range(h):
                for x in range(w):
                    if not cov[y, x]:
                        continue
                    s, wsum = [F(0.0), F(0.0), F(0.0)], F(0.0)
                    for dy in range(-2, 3):
                        for dx in range(-2, 3):
                            qy, qx = y + dy * step, x + dx * step
                            if not (0 <= qy < h and 0 <= qx < w) or not cov[qy, qx]:
                                continue
                            hk = H5[dy + 2] * H5[dx + 2]
                            if dy == 0 and dx == 0:
                                wt = hk
                            else:
                                d = c[y, x] - c[qy, qx]
                                e = (((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])) * kc[i]
                                if normal is not None:
                                    m = normal[y, x] - normal[qy, qx]
                                    e = e + ((((m[0] * m[0]) + (m[1] * m[1])) + (m[2] * m[2])) * kn)
                                if position is not None:
                                    D = position[qy, qx] - position[y, x]
                                    if normal is not None:
                                        n = normal[y, x]
                                        l = ((n[0] * D[0]) + (n[1] * D[1])) + (n[2] * D[2])
                                        e = e + ((l * l) * kl)
                                    e = e + ((((D[0] * D[0]) + (D[1] * D[1])) + (D[2] * D[2])) * kd[i])
                                e = e if e < F(128.0) else F(128.0)
                                wt = hk * _expf1(orc, -e)
                            for ch in range(3):
                                s[ch] = s[ch] + (wt * c[qy, qx, ch])
                            wsum = wsum + wt
                    if wsum > F(0.0):
                        for ch in range(3):
                            new[y, x, ch] = s[ch] / wsum
            c = new
    return c


# ---- dilation ----------------------------------------------------------------------------------------------------------------------
def dilate(radiance, covered, radius):
    """-> (out [H,W,3] f32, level [H,W] u32)"""
    val = np.array(radiance, dtype=F, copy=True)
    h, w, _ = val.shape
    level = np.asarray(covered, dtype=bool).reshape(h, w).astype(np.uint32)
    assert 0 <= radius <= MAX_RADIUS
    with np.errstate(all="ignore"):
        for k in range(1, radius + 1):
            s = np.zeros_like(val)
            count = np.zeros((h, w), dtype=np.uint32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    if dy == 0 and dx == 0:
                        continue
                    y0, y1 = max(0, -dy), min(h, h - dy)
                    x0, x1 = max(0, -dx), min(w, w - dx)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                    nb = level[Q] != 0
                    s[P] = np.where(nb[..., None], s[P] + val[Q], s[P])
                    count[P] += nb
            fill = (level == 0) & (count != 0)
            mean = (s / np.where(count != 0, count, 1).astype(F)[..., None]).astype(F)
            val, level = val.copy(), level.copy()
            val[fill] = mean[fill]
            level[fill] = k + 1
    return val, level


def dilate_scalar(radiance, covered, radius):
    val = np.array(radiance, dtype=F, copy=True)
    h, w, _ = val.shape
    level = np.asarray(covered, dtype=bool).reshape(h, w).astype(np.uint32)
    with np.errstate(all="ignore"):
        for k in range(1, radius + 1):
            nval, nlevel = val.copy(), level.copy()
            for y in range(h):
                for x in range(w):
                    if level[y, x] != 0:
                        continue
                    s, count = [F(0.0), F(0.0), F(0.0)], 0
                    for dy in range(-1, 2):
                        for dx in range(-1, 2):
                            qy, qx = y + dy, x + dx
                            if (dy == 0 and dx == 0) or not (0 <= qy < h and 0 <= qx < w) or level[qy, qx] == 0:
                                continue
                            for ch in range(3):
                                s[ch] = s[ch] + val[qy, qx, ch]
                            count += 1
                    if count:
                        for ch in range(3):
                            nval[y, x, ch] = s[ch] / F(count)
                        nlevel[y, x] = k + 1
            val, level = nval, nlevel
    return val, level


def chebyshev_level(covered, radius):
    """1 + the Chebyshev distance to the nearest covered texel where that is <= radius, else 0: a brute force over all pairs"""
    cov = np.asarray(covered, dtype=bool)
    h, w = cov.shape
    ys, xs = np.nonzero(cov)
    out = np.zeros((h, w), dtype=np.uint32)
    if len(ys) == 0:
        return out
    for y in range(h):
        for x in range(w):
            d = int(np.min(np.maximum(np.abs(ys - y), np.abs(xs - x))))
            out[y, x] = d + 1 if d <= radius else 0
    return out


def same_bits(a, b):
    """bit for bit on uint32 views, a NaN equal to any NaN (its sign and payload are the implementation's)"""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def rmse(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float(np.sqrt(np.mean(d * d)))
