"""The model of the variance-guided a-trous filter (include/mipt.h "variance-guided a-trous filter"), in numpy float32 over host
arrays.  Written from the contract's text: one rounded f32 operation per operator, in the order written; expf is the oracle's
restatement of glibc 2.35's (orc.eval_array(17, .)); numpy's float32 sqrt is correctly rounded; a tap outside the frame is not added
at all.  Nothing comes from the library under test."""
import numpy as np

F = np.float32
H5 = [F(1.0 / 16.0), F(1.0 / 4.0), F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0)]
G3 = [F(1.0 / 4.0), F(1.0 / 2.0), F(1.0 / 4.0)]
FLOOR = F(1.0 / 256.0)
LUMA = (F(0.2126), F(0.7152), F(0.0722))
EPS = F(1e-8)
EXPF = 17
DEFAULTS = dict(iterations=5, sigma_luminance=16.0, sigma_normal=0.5, sigma_depth=0.5, short_history=4.0)


def luminance(c):
    """((0.2126f*c.r) + (0.7152f*c.g)) + (0.0722f*c.b) of the last axis"""
    return ((LUMA[0] * c[..., 0]) + (LUMA[1] * c[..., 1])) + (LUMA[2] * c[..., 2])


def _sq3(a, b):
    d = a - b
    return ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])


def _window(h, w, oy, ox):
    """the pixels p whose tap q = p + (ox, oy) lies inside the frame, and those taps: (P, Q) index tuples, or None when there are none"""
    y0, y1 = max(0, -oy), min(h, h - oy)
    x0, x1 = max(0, -ox), min(w, w - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(None), slice(y0, y1), slice(x0, x1)), (slice(None), slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def _guide_terms(normal, depth, P, Q, kn, kz):
    """(dn*kn) + (dz*kz) with an absent guide's term left out; None without any guide"""
    e = None
    if normal is not None:
        e = _sq3(normal[P], normal[Q]) * kn
    if depth is not None:
        dz = (depth[P] - depth[Q]) * (depth[P] - depth[Q])
        e = (dz * kz) if e is None else e + (dz * kz)
    return e


def _expf_clamped(orc, e):
    e = np.where(e < F(128.0), e, F(128.0)).astype(F)                   # a NaN gives 128
    return orc.eval_array(EXPF, -e).reshape(e.shape)


def spatial_estimate(orc, c, var0, length, normal, depth, kn, kz, short_history):
    """the variance plane after the spatial-estimate pass"""
    sh = F(short_history)
    if not sh > F(0.0):
        return var0
    v, h, w, _ = c.shape
    lum = luminance(c)
    s1, s2, ws = (np.zeros((v, h, w), dtype=F) for _ in range(3))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            win = _window(h, w, dy, dx)
            if win is None:
                continue
            P, Q = win
            lq = lum[Q]
            eg = None if (dy == 0 and dx == 0) else _guide_terms(normal, depth, P, Q, kn, kz)
            wt = np.ones(lq.shape, dtype=F) if eg is None else _expf_clamped(orc, eg)   # the centre, or no guide at all: 1 without evaluation
            s1[P] = s1[P] + (wt * lq)
            s2[P] = s2[P] + (wt * (lq * lq))
            ws[P] = ws[P] + wt
    mu = s1 / ws
    est = (s2 / ws) - (mu * mu)
    est = np.where(est > F(0.0), est, F(0.0)).astype(F)
    lc = np.where(length > F(1.0), length, F(1.0)).astype(F)
    est = est * (sh / lc)
    return np.where(~(length >= sh), est, var0).astype(F)               # a NaN length takes the estimate


def _iteration(orc, c, var, normal, depth, step, sigma_l, kn, kz):
    v, h, w, _ = c.shape
    # the 3x3 prefilter of the variance, at distance 1 whatever the step
    gs, gw = np.zeros((v, h, w), dtype=F), np.zeros((v, h, w), dtype=F)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            win = _window(h, w, dy, dx)
            if win is None:
                continue
            P, Q = win
            gk = G3[dy + 1] * G3[dx + 1]
            gs[P] = gs[P] + (gk * var[Q])
            gw[P] = gw[P] + gk
    gv = gs / gw
    kl = F(1.0) / ((sigma_l * np.sqrt(gv)) + EPS)
    lum = luminance(c)
    s = np.zeros_like(c)
    sv, wsum = np.zeros((v, h, w), dtype=F), np.zeros((v, h, w), dtype=F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            win = _window(h, w, dy * step, dx * step)
            if win is None:
                continue
            P, Q = win
            hk = H5[dy + 2] * H5[dx + 2]
            cq, vq = c[Q], var[Q]
            if dy == 0 and dx == 0:
                wt = np.full(vq.shape, hk, dtype=F)                     # the centre: 9/64 without evaluation
            else:
                e = np.abs(lum[P] - lum[Q]) * kl[P]                     # then (dn*kn) and (dz*kz), added one after the other
                if normal is not None:
                    e = e + (_sq3(normal[P], normal[Q]) * kn)
                if depth is not None:
                    dz = (depth[P] - depth[Q]) * (depth[P] - depth[Q])
                    e = e + (dz * kz)
                wt = hk * _expf_clamped(orc, e)
            s[P] = s[P] + (wt[..., None] * cq)
            sv[P] = sv[P] + ((wt * wt) * vq)
            wsum[P] = wsum[P] + wt
    ok = wsum > F(0.0)
    safe = np.where(ok, wsum, F(1.0))
    c2 = np.where(ok[..., None], s / safe[..., None], c).astype(F)
    var2 = np.where(ok, sv / (safe * safe), var).astype(F)
    return c2, var2


def denoise_variance(orc, hdr, variance=None, length=None, normal=None, depth=None, albedo=None, iterations=5, sigma_luminance=16.0,
                     sigma_normal=0.5, sigma_depth=0.5, short_history=4.0):
    """hdr [V,H,W,3] (or [H,W,3]) float32, the temporal step's variance and length [V,H,W] (both or neither) and the optional guides
    -> (the filtered frame, the filtered variance), of hdr's leading shape"""
    hdr = np.asarray(hdr, dtype=F)
    single = hdr.ndim == 3
    lift = (lambda a: None if a is None else np.asarray(a, dtype=F)[None]) if single else (lambda a: None if a is None else np.asarray(a, dtype=F))
    c, variance, length, normal, depth, albedo = (lift(x) for x in (hdr, variance, length, normal, depth, albedo))
    assert 1 <= iterations <= 8 and (variance is None) == (length is None)
    with np.errstate(all="ignore"):
        kn = F(1.0) / (F(sigma_normal) * F(sigma_normal))
        kz = F(1.0) / (F(sigma_depth) * F(sigma_depth))
        if albedo is not None:
            a = np.where(albedo > FLOOR, albedo, FLOOR).astype(F)       # a NaN albedo gives the floor
            c = c / a
        if variance is None:
            var = np.zeros(c.shape[:-1], dtype=F)
            length = np.ones(c.shape[:-1], dtype=F)
        else:
            var = np.where(variance > F(0.0), variance, F(0.0)).astype(F)   # a NaN gives 0
        var = spatial_estimate(orc, c, var, length, normal, depth, kn, kz, short_history)
        for i in range(iterations):
            c, var = _iteration(orc, c, var, normal, depth, 1 << i, F(sigma_luminance), kn, kz)
        if albedo is not None:
            c = c * a
    c, var = c.astype(F), var.astype(F)
    return (c[0], var[0]) if single else (c, var)


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
