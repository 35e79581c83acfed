"""The model of the a-trous denoiser (include/mipt.h "a-trous denoiser"), in numpy float32 over host arrays.  Written from the
contract's text: one rounded f32 operation per operator, in the order written; expf is the oracle's restatement of glibc 2.35's
(orc.eval_array(17, .)); a tap outside the frame is not added at all.  Nothing comes from the library under test."""
import numpy as np

F = np.float32
H5 = [F(1.0 / 16.0), F(1.0 / 4.0), F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0)]
FLOOR = F(1.0 / 256.0)
EXPF = 17


def constants(iterations, sigma_color, sigma_normal, sigma_depth):
    """(kc_i for every iteration, kn, kz) as the host forms them in f32"""
    with np.errstate(all="ignore"):
        kc = []
        for i in range(iterations):
            sc = F(sigma_color) * F(2.0 ** -i)
            kc.append(F(1.0) / (sc * sc))
        return kc, F(1.0) / (F(sigma_normal) * F(sigma_normal)), F(1.0) / (F(sigma_depth) * F(sigma_depth))


def _sq3(a, b):
    """((dx*dx) + (dy*dy)) + (dz*dz) of the last axis"""
    d = a - b
    return ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])


def _iteration(orc, c, normal, depth, step, kc, kn, kz):
    v, h, w, _ = c.shape
    s = np.zeros_like(c)                                           # sum_ch, from +0
    wsum = np.zeros((v, h, w), dtype=F)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = dy * step, dx * step
            # the pixels p whose tap q = p + (ox, oy) lies inside the frame
            y0, y1 = max(0, -oy), min(h, h - oy)
            x0, x1 = max(0, -ox), min(w, w - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(None), slice(y0, y1), slice(x0, x1))
            Q = (slice(None), slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
            hk = H5[dy + 2] * H5[dx + 2]
            cq = c[Q]
            if dy == 0 and dx == 0:
                wt = np.full(cq.shape[:-1], hk, dtype=F)                # the centre: 9/64 without evaluation
            else:
                e = _sq3(c[P], cq) * kc
                if normal is not None:
                    e = e + (_sq3(normal[P], normal[Q]) * kn)
                if depth is not None:
                    dz = (depth[P] - depth[Q]) * (depth[P] - depth[Q])
                    e = e + (dz * kz)
                e = np.where(e < F(128.0), e, F(128.0)).astype(F)       # a NaN gives 128
                wt = hk * orc.eval_array(EXPF, -e).reshape(e.shape)
            s[P] = s[P] + (wt[..., None] * cq)
            wsum[P] = wsum[P] + wt
    ok = wsum > F(0.0)
    safe = np.where(ok, wsum, F(1.0))
    return np.where(ok[..., None], s / safe[..., None], c).astype(F)


def denoise(orc, hdr, normal=None, depth=None, albedo=None, iterations=5, sigma_color=4.0, sigma_normal=0.5, sigma_depth=0.5):
    """hdr [V,H,W,3] (or [H,W,3]) float32 and the optional guides -> the filtered frame, same shape"""
    hdr = np.asarray(hdr, dtype=F)
    single = hdr.ndim == 3
    lift = (lambda a: None if a is None else np.asarray(a, dtype=F)[None]) if single else (lambda a: None if a is None else np.asarray(a, dtype=F))
    c, normal, depth, albedo = lift(hdr), lift(normal), lift(depth), lift(albedo)
    assert 1 <= iterations <= 8
    kc, kn, kz = constants(iterations, sigma_color, sigma_normal, sigma_depth)
    with np.errstate(all="ignore"):
        if albedo is not None:
            a = np.where(albedo > FLOOR, albedo, FLOOR).astype(F)       # a NaN albedo gives the floor
            c = c / a
        for i in range(iterations):
            c = _iteration(orc, c, normal, depth, 1 << i, kc[i], kn, kz)
        if albedo is not None:
            c = c * a
    c = c.astype(F)
    return c[0] if single else c


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
