"""The model of the guided upsampling (include/mipt.h "guided upsampling"), in numpy float32 over host arrays.  Written from the
contract's text: one rounded f32 operation per operator, in the order written; expf is the oracle's restatement of glibc 2.35's
(orc.eval_array(17, .)); a skipped tap is not added at all.  Nothing comes from the library under test."""
import numpy as np

F = np.float32
FLOOR = F(1.0 / 256.0)
EXPF = 17
DEFAULTS = dict(sigma_normal=0.5, sigma_depth=0.5)


def _floored(albedo):
    return np.where(albedo > FLOOR, albedo, FLOOR).astype(F)            # a NaN albedo gives the floor


def upsample(orc, lo_hdr, scale, lo_guides=None, guides=None, sigma_normal=0.5, sigma_depth=0.5):
    """lo_hdr [V,h,w,3] (or [h,w,3]) float32; lo_guides / guides: dicts with any of normal [..,3], depth [..], albedo [..,3] float32
    and material [..] (any 32-bit integer kind; the bits count), the same keys at both resolutions -> (out [V,h*k,w*k,3],
    weight [V,h*k,w*k], bilinear [V,h*k,w*k,3]): the frame, wsum, and what plain bilinear alone gives (sb / bsum, re-modulated) --
    the value of a pixel whose weight is 0"""
    lo_hdr = np.asarray(lo_hdr, dtype=F)
    single = lo_hdr.ndim == 3
    lo_guides, guides = dict(lo_guides or {}), dict(guides or {})
    names = ("normal", "depth", "albedo", "material")
    lo_guides = {n: a for n, a in lo_guides.items() if n in names and a is not None}
    guides = {n: a for n, a in guides.items() if n in names and a is not None}
    assert set(lo_guides) == set(guides), "a guide is given at both resolutions or at neither"

    def lift(name, a):
        a = np.ascontiguousarray(a)
        a = a.view(np.uint32) if name == "material" else a.astype(F)
        return a[None] if single else a

    lo = {n: lift(n, a) for n, a in lo_guides.items()}
    hi = {n: lift(n, a) for n, a in guides.items()}
    c = lo_hdr[None] if single else lo_hdr
    k = int(scale)
    assert 2 <= k <= 8
    v, h, w, _ = c.shape
    H, W = h * k, w * k
    with np.errstate(all="ignore"):
        kn = F(1.0) / (F(sigma_normal) * F(sigma_normal))
        kz = F(1.0) / (F(sigma_depth) * F(sigma_depth))
        if "albedo" in lo:
            c = c / _floored(lo["albedo"])
        X, Y = np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64)
        x0, y0 = X // k, Y // k
        rx, ry = X - x0 * k, Y - y0 * k
        wx, wy = rx.astype(F) / F(k), ry.astype(F) / F(k)
        ux, uy = F(1.0) - wx, F(1.0) - wy
        sb, s = np.zeros((v, H, W, 3), dtype=F), np.zeros((v, H, W, 3), dtype=F)
        bsum, wsum = np.zeros((v, H, W), dtype=F), np.zeros((v, H, W), dtype=F)
        for ty in (0, 1):
            for tx in (0, 1):
                # the pixels whose tap takes part: rows and columns are independent
                ys = np.nonzero((ry != 0) & (y0 + 1 < h))[0] if ty else Y
                xs = np.nonzero((rx != 0) & (x0 + 1 < w))[0] if tx else X
                if len(ys) == 0 or len(xs) == 0:
                    continue
                P = (slice(None), ys[:, None], xs[None, :])
                Q = (slice(None), (y0[ys] + ty)[:, None], (x0[xs] + tx)[None, :])
                b = ((wx if tx else ux)[xs][None, :] * (wy if ty else uy)[ys][:, None]).astype(F)      # [len(ys), len(xs)]
                b = np.broadcast_to(b[None], (v,) + b.shape)
                cq = c[Q]
                sb[P] = sb[P] + (b[..., None] * cq)
                bsum[P] = bsum[P] + b
                e = None
                if "normal" in hi:
                    d = hi["normal"][P] - lo["normal"][Q]
                    e = (((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])) * kn
                if "depth" in hi:
                    dz = (hi["depth"][P] - lo["depth"][Q]) * (hi["depth"][P] - lo["depth"][Q])
                    e = (dz * kz) if e is None else e + (dz * kz)
                if e is None:
                    wt = b                                              # neither normal nor depth: b without evaluation
                else:
                    e = np.where(e < F(128.0), e, F(128.0)).astype(F)   # a NaN gives 128
                    wt = (b * orc.eval_array(EXPF, -e).reshape(e.shape)).astype(F)
                ok = np.ones(b.shape, dtype=bool)
                if "material" in hi:
                    ok = hi["material"][P] == lo["material"][Q]         # a tap of another material takes no further part
                s[P] = np.where(ok[..., None], s[P] + (wt[..., None] * cq), s[P])
                wsum[P] = np.where(ok, wsum[P] + wt, wsum[P])
        guided = wsum > F(0.0)
        safe = np.where(guided, wsum, F(1.0))
        bil = sb / bsum[..., None]
        col = np.where(guided[..., None], s / safe[..., None], bil).astype(F)
        if "albedo" in hi:
            a = _floored(hi["albedo"])
            col, bil = col * a, bil * a
    col, wsum, bil = col.astype(F), wsum.astype(F), bil.astype(F)
    return (col[0], wsum[0], bil[0]) if single else (col, wsum, bil)


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
