"""The model of the filling sample map (include/mipt.h "mipt_sample_map_fill"), in numpy over host arrays.  Written from the contract's
text on top of sample_map_model: the weights, T and round 1 are the plain map's; every later round sums in exact integers, forms one
binary64 ratio and hands each pixel below the span its floored share of what is left.  Nothing comes from the library under test."""
import numpy as np

import sample_map_model as SM


def fill(variance, hdr=None, albedo=None, min_samples=1, max_samples=8, budget=None, rounds=1, trace=None):
    """variance [..] float32, hdr / albedo [..,3] float32 or None -> counts [..] uint32.  `trace`, a list, receives per round
    k >= 2 a dict(A, S, E, r, active) of the frame's numbers."""
    assert 1 <= rounds <= 8
    budget = min_samples if budget is None else budget
    qi = SM.weights(variance, hdr, albedo)
    n = qi.size
    span = max_samples - min_samples
    extra = SM.total(budget, n) - min_samples * n
    e = SM.sample_map(variance, hdr, albedo, min_samples, max_samples, budget).astype(np.int64) - min_samples      # e_1
    for _ in range(2, rounds + 1):
        open_ = e < span
        a = int(e.sum(dtype=np.uint64))
        s = int(qi[open_].sum(dtype=np.uint64))
        left = extra - a if a < extra else 0
        active = s != 0 and left != 0
        r = np.float64(left) / np.float64(s) if active else np.float64(0.0)
        if trace is not None:
            trace.append(dict(A=a, S=s, E=left, r=float(r), active=active))
        if not active:
            continue                                            # the sums stay as they are: no later round changes anything either
        x = qi.astype(np.float64) * r
        room = (span - e).astype(np.int64)
        fits = x < room.astype(np.float64)
        add = np.where(fits, np.where(fits, x, 0.0).astype(np.int64), room)
        e = np.where(open_, e + add, e)
    return (e + min_samples).astype(np.uint32)
