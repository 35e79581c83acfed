"""CPU: the numpy model of the sample map (tests/tools/sample_map_model.py) obeys the properties include/mipt.h states -- the bounds,
the budget, monotonicity, the uniform case and finite counts for every non-finite input.  The kernels are held to the model bit for
bit in tests/test_gpu_sample_map.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import sample_map_model as SM  # noqa: E402

F = np.float32


def _planes(seed, shape=(2, 9, 13)):
    rng = np.random.default_rng(seed)
    variance = (rng.random(shape) ** 4).astype(F)
    hdr = (rng.random(shape + (3,)) ** 2 * 3.0).astype(F)
    albedo = rng.random(shape + (3,)).astype(F)
    return variance, hdr, albedo


@pytest.mark.parametrize("with_hdr,with_albedo", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("lo,hi,budget", [(1, 8, 2.0), (0, 16, 1.5), (2, 2, 2.0), (1, 65535, 300.25), (3, 9, 9.0)])
def test_bounds_and_budget(with_hdr, with_albedo, lo, hi, budget):
    variance, hdr, albedo = _planes(lo * 100 + hi)
    counts = SM.sample_map(variance, hdr if with_hdr else None, albedo if with_albedo else None, lo, hi, budget)
    assert counts.dtype == np.uint32 and counts.shape == variance.shape
    assert counts.min() >= lo and counts.max() <= hi
    assert int(counts.sum(dtype=np.uint64)) <= SM.total(budget, variance.size)


def test_monotone_in_variance_at_fixed_hdr():
    """one pixel's variance rises, everything else fixed: its weight never falls; and within one frame a pixel with more variance
    and the same hdr never gets fewer samples"""
    variance, hdr, albedo = _planes(3)
    steps = np.array([0.0, 1e-12, 1e-6, 1e-3, 0.1, 0.5, 1.0, 50.0, 1e12], dtype=F)
    last = -1
    for s in steps:
        v = variance.copy()
        v[0, 4, 4] = s
        q = int(SM.weights(v, hdr, albedo)[0, 4, 4])
        assert q >= last
        last = q
    hdr[...] = hdr[0, 0, 0]
    albedo[...] = albedo[0, 0, 0]
    counts = SM.sample_map(variance, hdr, albedo, 1, 32, 4.0)
    order = np.argsort(variance.ravel(), kind="stable")
    assert np.all(np.diff(counts.ravel()[order].astype(np.int64)) >= 0)
    assert counts.max() > counts.min()


def test_zero_sum_gives_the_uniform_value():
    z = np.zeros((3, 5, 7), dtype=F)
    assert np.all(SM.sample_map(z, None, None, 1, 8, 3.75) == 3)
    assert np.all(SM.sample_map(z, None, None, 0, 8, 0.5) == 0)
    assert np.all(SM.sample_map(z, None, None, 2, 4, 4.0) == 4)
    assert np.all(SM.sample_map(np.full((2, 2), np.nan, dtype=F), None, None, 1, 8, 2.0) == 2)
    assert np.all(SM.sample_map(np.full((2, 2), -np.inf, dtype=F), None, None, 1, 8, 2.0) == 2)


def test_non_finite_inputs_give_finite_counts():
    variance, hdr, albedo = _planes(9, (1, 4, 8))
    variance[0, 0, :6] = [np.nan, -1.0, np.inf, -np.inf, 1e-42, 0.0]
    hdr[0, 1, 0] = 0.0
    hdr[0, 1, 1] = -3.0
    hdr[0, 1, 2] = np.nan
    hdr[0, 1, 3] = np.inf
    albedo[0, 2, 0] = 0.0
    albedo[0, 2, 1] = np.nan
    albedo[0, 2, 2] = -1.0
    albedo[0, 2, 3] = np.inf
    for args in ((None, None), (hdr, None), (hdr, albedo)):
        q = SM.weights(variance, *args)
        assert q.dtype == np.uint64 and q.max() <= SM.QMAX
        assert q[0, 0, 0] == 0 and q[0, 0, 1] == 0 and q[0, 0, 3] == 0 and q[0, 0, 5] == 0
        assert q[0, 0, 2] == SM.QMAX                                        # +inf variance saturates
        counts = SM.sample_map(variance, *args, 1, 8, 2.0)
        assert counts.min() >= 1 and counts.max() <= 8
        assert int(counts.sum()) <= SM.total(2.0, variance.size)


def test_budget_at_the_ends():
    variance, hdr, albedo = _planes(5)
    assert np.all(SM.sample_map(variance, hdr, albedo, 2, 8, 2.0) == 2)      # budget == min: all min
    one = np.zeros((1, 6, 6), dtype=F)
    one[0, 3, 3] = 4.0                                                       # one noisy pixel takes what it can, and no more than max
    counts = SM.sample_map(one, None, None, 1, 8, 8.0)
    assert counts[0, 3, 3] == 8 and counts.max() == 8
    assert np.all(np.delete(counts.ravel(), 3 * 6 + 3) == 1)                 # the cut-off share is not redistributed
    assert int(counts.sum()) <= SM.total(8.0, one.size)


def test_total_is_the_hosts_double_product():
    assert SM.total(2.0, 10) == 20 and SM.total(1.5, 3) == 4 and SM.total(0.0, 7) == 0
    assert SM.total(np.float32(1.1), 1000) == int(np.floor(float(np.float32(1.1)) * 1000.0))
