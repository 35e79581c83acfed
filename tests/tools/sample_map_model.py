"""The model of the sample map (include/mipt.h "adaptive sampling"), in numpy over host arrays.  Written from the contract's text: one
rounded f32 operation per operator in the order written, every comparison with a NaN on the "zero" side, the sum of the weights in
exact integers, the ratio and the shares in binary64.  Nothing comes from the library under test."""
import numpy as np

F = np.float32
FLOOR = F(1.0 / 256.0)
QMAX = 16777215


def weights(variance, hdr=None, albedo=None):
    """qi per pixel as uint64 (exact integers), of variance's shape"""
    assert albedo is None or hdr is not None, "albedo is given only with hdr"
    with np.errstate(all="ignore"):
        var = np.asarray(variance, dtype=F)
        v = np.where(var > 0, var, F(0)).astype(F)                    # NaN, negatives, -inf -> 0
        s = np.sqrt(v, dtype=F)
        w = s
        if hdr is not None:
            c = np.asarray(hdr, dtype=F)
            if albedo is not None:
                alb = np.asarray(albedo, dtype=F)
                c = (c / np.where(alb > FLOOR, alb, FLOOR).astype(F)).astype(F)   # a NaN albedo gives the floor
            lum = ((F(0.2126) * c[..., 0]).astype(F) + (F(0.7152) * c[..., 1]).astype(F)).astype(F)
            lum = (lum + (F(0.0722) * c[..., 2]).astype(F)).astype(F)
            lum = np.where(lum > 0, lum, F(0)).astype(F)
            w = (s / (lum + F(0.00390625)).astype(F)).astype(F)
        q = (w * F(4096.0)).astype(F)
        small = q < F(QMAX)
        qi = np.where(q > 0, np.where(small, np.where(small & (q > 0), q, F(0)).astype(np.uint64), np.uint64(QMAX)), np.uint64(0))
    return qi.astype(np.uint64)


def total(budget, n_pixels):
    """T: the host's floor((double)budget * (double)N) for the f32 budget the options carry"""
    return int(np.floor(np.float64(F(budget)) * np.float64(n_pixels)))


def sample_map(variance, hdr=None, albedo=None, min_samples=1, max_samples=8, budget=None):
    """variance [..] float32, hdr / albedo [..,3] float32 or None -> counts [..] uint32"""
    budget = min_samples if budget is None else budget
    assert 0 <= min_samples <= max_samples and 1 <= max_samples <= 65535
    assert np.isfinite(F(budget)) and F(min_samples) <= F(budget) <= F(max_samples)
    qi = weights(variance, hdr, albedo)
    n = qi.size
    span = max_samples - min_samples
    extra = total(budget, n) - min_samples * n
    assert extra >= 0
    s = int(qi.sum(dtype=np.uint64)) if n < (1 << 39) else sum(int(x) for x in qi.ravel())   # 2^24 * 2^39 < 2^64: exact
    if s == 0:
        e = np.full(qi.shape, min(extra // n, span), dtype=np.uint64)
    else:
        r = np.float64(extra) / np.float64(s)
        x = qi.astype(np.float64) * r
        e = np.where(x < np.float64(span), np.where(x < np.float64(span), x, 0.0).astype(np.uint64), np.uint64(span))
    return (np.uint64(min_samples) + e).astype(np.uint32)
