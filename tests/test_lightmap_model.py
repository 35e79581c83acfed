"""CPU: the models of include/mipt.h "lightmap finishing" (tests/tools/lightmap_model.py).  The vectorised filter and dilation are
held to a plain loop over every texel and tap, bit for bit, and to the properties that follow from the definition: what an uncovered
texel holds reaches no covered one, two charts far enough apart in the world do not see each other, and a dilation's level is one
more than the Chebyshev distance to the nearest covered texel."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import lightmap_model as M  # noqa: E402

SHAPES = ((1, 1), (5, 3), (9, 7))                                  # (width, height)
GUIDES = ((False, False), (True, False), (False, True), (True, True))   # (position, normal)


def _atlas(seed, w, h, fill=0.6):
    """radiance, coverage, position, unit normal of a random atlas; at least one covered texel"""
    rng = np.random.default_rng(seed)
    rad = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
    cov = rng.random((h, w)) < fill
    cov[rng.integers(h), rng.integers(w)] = True
    pos = rng.uniform(-0.3, 0.3, (h, w, 3)).astype(np.float32)
    nrm = rng.normal(size=(h, w, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    return rad, cov, pos, nrm


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("iterations", (1, 3, 8))
def test_filter_equals_the_scalar_loop(orc, w, h, iterations):
    """all four guide subsets; at 8 iterations the last step is 128 and only the centre tap is left"""
    rad, cov, pos, nrm = _atlas(100 * w + iterations, w, h)
    for use_pos, use_nrm in GUIDES:
        kw = dict(position=pos if use_pos else None, normal=nrm if use_nrm else None, iterations=iterations, sigma_color=1.5, sigma_normal=1.0,
                  sigma_plane=0.4, sigma_distance=0.25)
        a, b = M.filter(orc, rad, cov, **kw), M.filter_scalar(orc, rad, cov, **kw)
        assert M.same_bits(a, b), (use_pos, use_nrm)
        assert np.array_equal(a.view(np.uint32)[~cov], rad.view(np.uint32)[~cov])            # uncovered: word for word
        if w * h > 1 and cov.sum() > 1 and iterations < 8:
            assert not M.same_bits(a, rad)


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("radius", (0, 1, 3, 8))
def test_dilate_equals_the_scalar_loop(w, h, radius):
    rad, cov, _, _ = _atlas(7 * w + radius, w, h, fill=0.25)
    a, la = M.dilate(rad, cov, radius)
    b, lb = M.dilate_scalar(rad, cov, radius)
    assert M.same_bits(a, b) and np.array_equal(la, lb)
    assert np.array_equal(a.view(np.uint32)[cov], rad.view(np.uint32)[cov]) and np.all(la[cov] == 1)
    still = la == 0
    assert np.array_equal(a.view(np.uint32)[still], rad.view(np.uint32)[still])
    if radius == 0:
        assert np.array_equal(a.view(np.uint32), rad.view(np.uint32))


def test_uncovered_radiance_reaches_no_covered_texel(orc):
    rad, cov, pos, nrm = _atlas(5, 9, 7)
    assert (~cov).sum() >= 10
    poisoned = rad.copy()
    poisoned[~cov] = np.nan
    for use_pos, use_nrm in GUIDES:
        kw = dict(position=pos if use_pos else None, normal=nrm if use_nrm else None, iterations=3, sigma_distance=0.5, sigma_plane=0.5)
        a, b = M.filter(orc, rad, cov, **kw), M.filter(orc, poisoned, cov, **kw)
        assert np.array_equal(a.view(np.uint32)[cov], b.view(np.uint32)[cov])
        assert np.all(np.isnan(b[~cov])) and not np.any(np.isnan(b[cov]))


def separated_charts(seed=11, w=12, h=6, iterations=3, sigma_distance=0.01):
    """Two charts side by side in the atlas, a 2-texel gutter between them, whose world positions lie apart: chart A around the
    origin, chart B around x = gap.  kd_i is smallest at the last iteration, sd = sigma_distance * 2^(iterations-1); the squared
    distance between any texel of A and any of B is at least (gap - 2 * 0.05)^2, and gap is chosen so that this is 2 * 128 * sd^2:
    dd * kd_i >= 256 >= 128 for every i, with the margin of 2 on the squared distance."""
    rng = np.random.default_rng(seed)
    rad = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
    cov = np.ones((h, w), dtype=bool)
    cov[:, 5:7] = False
    a, b = np.zeros((h, w), dtype=bool), np.zeros((h, w), dtype=bool)
    a[:, :5], b[:, 7:] = True, True
    pos = rng.uniform(-0.05, 0.05, (h, w, 3)).astype(np.float32)
    sd = sigma_distance * 2.0 ** (iterations - 1)
    gap = 0.1 + float(np.sqrt(2.0 * 128.0)) * sd
    pos[b, 0] += np.float32(gap)
    d2 = ((pos[a][:, None, :].astype(np.float64) - pos[b][None, :, :].astype(np.float64)) ** 2).sum(-1).min()
    assert d2 / (sd * sd) >= 2 * 128.0
    return rad, cov, pos, a, b, dict(iterations=iterations, sigma_distance=sigma_distance, sigma_color=4.0)


def test_charts_far_apart_in_the_world_do_not_see_each_other(orc):
    rad, cov, pos, a, b, kw = separated_charts()
    base = M.filter(orc, rad, cov, position=pos, **kw)
    other = rad.copy()
    other[b] = other[b] * np.float32(3.0) + np.float32(1.0)
    out = M.filter(orc, other, cov, position=pos, **kw)
    assert np.array_equal(out.view(np.uint32)[a], base.view(np.uint32)[a])                   # A does not depend on B's values
    assert not np.array_equal(out.view(np.uint32)[b], base.view(np.uint32)[b])
    other = rad.copy()
    other[a] = np.float32(0.25)
    out = M.filter(orc, other, cov, position=pos, **kw)
    assert np.array_equal(out.view(np.uint32)[b], base.view(np.uint32)[b])                   # nor B on A's
    # without the position the charts do mix across the 2-texel gutter
    assert not np.array_equal(M.filter(orc, other, cov, **kw).view(np.uint32)[b], M.filter(orc, rad, cov, **kw).view(np.uint32)[b])


@pytest.mark.parametrize("radius", (0, 1, 2, 5, 64))
def test_dilation_levels_are_chebyshev_distances(radius):
    rng = np.random.default_rng(radius)
    for w, h, fill in ((9, 7, 0.1), (20, 13, 0.02), (4, 1, 0.3)):
        cov = rng.random((h, w)) < fill
        cov[rng.integers(h), rng.integers(w)] = True
        rad = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
        _, level = M.dilate(rad, cov, radius)
        assert np.array_equal(level, M.chebyshev_level(cov, radius))
    _, level = M.dilate(rad, np.zeros_like(cov), radius)                                     # nothing covered: nothing filled
    assert not level.any()


def test_constants_and_the_clamp(orc):
    kc, kn, kl, kd = M.constants(3, 4.0, 0.5, 0.25, 2.0)
    assert [float(k) for k in kc] == [1 / 16.0, 1 / 4.0, 1.0] and [float(k) for k in kd] == [1 / 4.0, 1 / 16.0, 1 / 64.0]
    assert float(kn) == 4.0 and float(kl) == 16.0
    assert orc.eval_array(M.EXPF, np.float32([-128.0, -0.0])).tolist() == [0.0, 1.0]
