"""CPU: the models of tests/tools/probe_model.py, held to what include/mipt.h "irradiance probes" says independently of the library:
the literals against their closed forms, the basis against orthonormality, the vectorised lookup against its scalar restatement and
against closed forms of the cosine convolution in float64, the f32 bake model against a float64 projection written from the textbook
formulas, the conditions every scene of tests/test_gpu_probe.py must meet on the model alone, and those of the hard lookup cases of
tests/test_gpu_probe_hard.py (PM.lookup_hard_case)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import probe_model as PM  # noqa: E402

F = np.float32


def test_literals_are_the_nearest_floats_to_their_closed_forms():
    for name, (lit, closed) in PM.CLOSED.items():
        assert lit.dtype == np.float32 and lit == np.float32(closed), (name, float(lit), closed)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mipt.h")).read()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rust_ray_tracing_amd", "csrc", "probe.hip")).read()
    for lit in ("0.2820948f", "0.48860252f", "1.0925485f", "0.31539157f", "0.54627424f", "3.1415927f", "2.0943952f", "0.7853982f", "12.566371f"):
        assert lit in text and lit in src, lit                      # the header, the kernels and the model state the same digits
        assert any(np.float32(float(lit[:-1])) == v for v, _ in PM.CLOSED.values()), lit


def _quadrature(n_theta=8, n_phi=16):
    """Gauss-Legendre in cos(theta) x uniform in phi: exact for products of two band-2 functions (degree 4) -> (dirs [m, 3], weights [m])"""
    mu, w = np.polynomial.legendre.leggauss(n_theta)
    phi = (np.arange(n_phi) + 0.5) * (2 * np.pi / n_phi)
    s = np.sqrt(1 - mu * mu)
    d = np.stack([np.outer(s, np.cos(phi)), np.outer(s, np.sin(phi)), np.outer(mu, np.ones(n_phi))], axis=-1).reshape(-1, 3)
    return d, np.repeat(w, n_phi) * (2 * np.pi / n_phi)


def test_basis_is_orthonormal():
    d, w = _quadrature()
    for Y in (PM.basis64(d), PM.basis(d.astype(np.float32)).astype(np.float64)):
        gram = np.einsum("m,mj,mk->jk", w, Y, Y)
        assert np.abs(gram - np.eye(9)).max() < 1e-6, gram
    # the f32 directions of the second pass are rounded: that costs 6e-8 relative, far inside the bound
    assert np.abs(PM.basis(d.astype(np.float32)) - PM.basis64(d)).max() < 1e-6


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 1, 3), (4, 3, 2)])
@pytest.mark.parametrize("clamp", [False, True])
def test_vectorised_lookup_equals_the_scalar_loop(dims, clamp):
    grid, sh, P, N = PM.lookup_case(dims, 300, 3)
    for valid in (None, (np.arange(len(sh)) % 3 != 1).astype(np.uint8), np.zeros(len(sh), dtype=np.uint8)):
        a, b = PM.lookup(sh, grid, P, N, valid, clamp), PM.lookup_scalar(sh, grid, P, N, valid, clamp)
        assert PM.same_bits(a, b), np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))[:8]
        if clamp:
            assert not np.any(a < 0) and not np.any(np.isnan(a))
    assert not np.any(PM.lookup(sh, grid, P, N, np.zeros(len(sh), dtype=np.uint8)))            # every corner left out: +0


def test_zero_weight_hides_a_nan_probe_and_a_multiply_would_not():
    grid, sh, P, N = PM.lookup_case((4, 3, 2), 64, 4)
    bad = sh.copy()
    bad[5] = np.nan                                                                            # probe (1, 1, 0)
    pts = PM.grid_positions(*grid)
    on = np.stack([pts[4], pts[6], pts[1], pts[17]])                                          # its neighbours along x, y, z: weight exactly 0 for probe 5
    out = PM.lookup(bad, grid, on, N[:4])
    assert not np.any(np.isnan(out)) and PM.same_bits(out, PM.lookup(sh, grid, on, N[:4]))
    assert np.all(np.isnan(PM.lookup(bad, grid, pts[5:6], N[:1])))                             # on the probe itself it shows


def _const_grid(coeffs, dims=(2, 2, 2)):
    sh = np.zeros((int(np.prod(dims)), 9, 3), dtype=np.float32)
    for k, v in coeffs.items():
        sh[:, k, :] = v
    return ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dims), sh


def test_lookup_closed_forms():
    rng = np.random.default_rng(9)
    n = 200
    N = rng.normal(0, 1, (n, 3))
    N = N / np.linalg.norm(N, axis=1, keepdims=True)
    P = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    a, b = 0.7, 0.4
    s4 = np.sqrt(4 * np.pi)
    # L = a: E = pi a for every normal
    grid, sh = _const_grid({0: a * s4})
    E = PM.lookup(sh, grid, P, N.astype(np.float32)).astype(np.float64)
    assert np.abs(E / (np.pi * a) - 1).max() < 1e-5
    # L = a + b d_z: slot 2 is z
    grid, sh = _const_grid({0: a * s4, 2: b * np.sqrt(4 * np.pi / 3)})
    E = PM.lookup(sh, grid, P, N.astype(np.float32)).astype(np.float64)
    want = np.pi * a + (2 * np.pi / 3) * b * N[:, 2]
    assert np.abs(E[:, 0] / want - 1).max() < 1e-5
    # L = d_z^2
    grid, sh = _const_grid({0: s4 / 3, 6: (2 / 3) * np.sqrt(4 * np.pi / 5)})
    E = PM.lookup(sh, grid, P, N.astype(np.float32)).astype(np.float64)
    want = np.pi / 3 + np.pi * (3 * N[:, 2] ** 2 - 1) / 12
    assert np.abs(E[:, 1] / want - 1).max() < 1e-5


# ---- the hard lookup cases of tests/test_gpu_probe_hard.py ------------------------------------------------------------------------------
LOOKUP_HARD_SEED = 7
_hard_lookup = []


def _hard_cases():
    if not _hard_lookup:
        _hard_lookup.extend(PM.lookup_hard_case(LOOKUP_HARD_SEED))
    return list(zip(PM.LOOKUP_HARD_NAMES, _hard_lookup))


def _nan_rows(x):
    return int(np.isnan(x).any(axis=1).sum())


def _same_or_both_nan(a, b):
    wa, wb = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    return not np.any((wa != wb) & ~(np.isnan(a) & np.isnan(b)))


def test_hard_lookup_cases_vectorised_equals_scalar_and_the_models_conditions():
    seen = set()
    for name, (grid, sh, valid, P, N) in _hard_cases():
        assert len(P) % 64 != 0 and P.dtype == N.dtype == sh.dtype == np.float32 and valid.dtype == np.uint8, name
        seen |= set(valid.tolist())
        planes = (valid,) if name.startswith("non-finite") else (None, valid)         # without its plane that grid is all NaN, by design
        for v in planes:
            for clamp in (False, True):
                a = PM.lookup(sh, grid, P, N, v, clamp)
                if clamp:
                    assert not np.any(np.isnan(a)) and not np.any(a < 0), (name, v is not None)
                else:
                    assert 10 * _nan_rows(a) <= len(a) and np.any(a < 0), (name, v is not None, _nan_rows(a), len(a))
                assert np.any(a > 0) and np.any(np.isfinite(a) & (a != 0))
                if (v is None) == (not clamp):                                       # (no plane, no clamp) and (plane, clamp): the scalar loop is slow
                    b = PM.lookup_scalar(sh, grid, P, N, v, clamp)
                    assert _same_or_both_nan(a, b), (name, np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))[:8])
        normal_kinds = [np.any(np.all(N == 0, axis=1)), np.any(np.signbit(N) & (N == 0)), np.any(np.isnan(N)), np.any(np.isinf(N)),
                        np.any(N == F(1e30)), np.any(N == F(1e-30)), np.any(N == F(1e-42))]
        odd = ~np.isclose(np.linalg.norm(N.astype(np.float64), axis=1), 1.0, atol=1e-5)
        assert (all(normal_kinds) or len(P) < 100) and 10 * int(odd.sum()) <= len(P), (name, normal_kinds, int(odd.sum()))
    assert seen == set(range(256))                                                    # every byte value of `valid`, 0 among them


def test_hard_lookup_grids_do_not_divide_back_and_cover_their_points():
    for name, (grid, sh, valid, P, N) in _hard_cases()[:3]:
        origin, spacing, dims = grid
        pts = PM.grid_positions(*grid)
        assert PM.same_bits(P[: len(pts)], pts)
        inexact = 0
        for a in range(3):
            g = (pts[:, a] - F(origin[a])) / F(spacing[a])
            inexact += int((g != np.round(g)).sum())
            i0, f = PM._axis(P[:, a], origin[a], spacing[a], dims[a])
            if dims[a] > 1:
                assert set(i0.tolist()) == set(range(dims[a] - 1)), (name, a)        # every cell of the axis is visited
                assert np.any(f == 0) and np.any(f == 1) and np.any((f > 0) & (f < 2.0 ** -10)) and np.any((f < 1) & (f > 1 - 2.0 ** -10))
        assert inexact > 0, name                                                      # a probe's own position does not give an integer quotient
        assert np.isnan(P).any() and np.isinf(P).any() and np.any(np.abs(P) == F(3e38)) and np.any(P == F(1e-42))
        assert np.any((P == 0) & np.signbit(P)) and np.any((P == 0) & ~np.signbit(P))
    # a multiplication by the reciprocal of the spacing is another function on these grids
    grid, sh, valid, P, N = _hard_cases()[0][1]
    with np.errstate(all="ignore"):
        g = (P[:, 0] - F(grid[0][0])) / F(grid[1][0])
        r = (P[:, 0] - F(grid[0][0])) * (F(1.0) / F(grid[1][0]))
    assert np.any((g != r) & np.isfinite(g))


def test_hard_lookup_extreme_spacings_overflow_go_denormal_and_underflow():
    for name, (grid, sh, valid, P, N) in _hard_cases()[3:5]:
        origin, spacing, dims = grid
        with np.errstate(all="ignore"):
            g = [(P[:, a] - F(origin[a])) / F(spacing[a]) for a in range(3)]
        assert np.any(np.isinf(g[0])) and np.any((g[2] != 0) & (np.abs(g[2]) < 2.0 ** -126)), name    # a quotient overflows, one is denormal
        w = [(F(1.0) - f, f) for _, f in (PM._axis(P[:, a], origin[a], spacing[a], dims[a]) for a in range(3))]
        under = np.zeros(len(P), dtype=bool)
        with np.errstate(all="ignore"):
            for c in range(8):
                parts = (w[0][c & 1], w[1][(c >> 1) & 1], w[2][c >> 2])
                under |= ((parts[0] * parts[1]) * parts[2] == 0) & (parts[0] != 0) & (parts[1] != 0) & (parts[2] != 0)
        assert int(under.sum()) >= 4, (name, int(under.sum()))                       # three non-zero weights whose product is exactly 0: skipped


def test_hard_lookup_never_reads_an_invalid_probe_and_divides_by_a_tiny_sum():
    cases = dict(_hard_cases())
    grid, sh, valid, P, N = cases["non-finite words behind invalid probes"]
    bad = sh[valid == 0]
    assert len(bad) and not np.isfinite(bad).any() and np.any(bad.view(np.uint32) == PM.SENTINEL_BITS) and np.isfinite(sh[valid != 0]).all()
    noise = sh.copy()
    noise[valid == 0] = np.random.default_rng(3).normal(0, 1, bad.shape).astype(np.float32)
    for clamp in (False, True):
        a, b = PM.lookup(sh, grid, P, N, valid, clamp), PM.lookup(noise, grid, P, N, valid, clamp)
        assert PM.same_bits(a[~np.isnan(a).any(axis=1)], b[~np.isnan(a).any(axis=1)]) and _same_or_both_nan(a, b)
    with np.errstate(all="ignore"):                                                   # a multiply by 0 in place of the skip shows on most points
        leaky = PM.lookup(np.where(np.isfinite(sh), sh, np.nan), grid, P, N, None)
    assert 2 * _nan_rows(leaky) >= len(P)
    grid, sh, valid, P, N = cases["inf on a valid probe"]
    assert int(np.isinf(sh).sum()) == 1 and valid[np.flatnonzero(np.isinf(sh).reshape(len(sh), -1).any(axis=1))[0]] != 0
    assert np.isinf(PM.lookup(sh, grid, P, N, valid)).any()
    grid, sh, valid, P, N = cases["one valid corner of tiny weight"]
    E, wsum = PM.lookup(sh, grid, P, N, valid, with_wsum=True)
    tiny = (wsum > 0) & (wsum < 2.0 ** -60)
    assert int(tiny.sum()) >= 4 and np.all(np.isfinite(E[tiny])) and np.all(E[tiny] != 0), (int(tiny.sum()), E[tiny])


def test_grid_positions_are_in_index_order(rrt):
    dims = (4, 3, 2)
    pts = PM.grid_positions((1.0, 2.0, 3.0), (0.5, 0.25, 2.0), dims)
    assert pts.shape == (24, 3) and pts.dtype == np.float32
    for iz in range(2):
        for iy in range(3):
            for ix in range(4):
                assert tuple(pts[(iz * 3 + iy) * 4 + ix]) == (1.0 + 0.5 * ix, 2.0 + 0.25 * iy, 3.0 + 2.0 * iz)
    assert PM.same_bits(pts, rrt.Scene.probe_grid((1.0, 2.0, 3.0), (0.5, 0.25, 2.0), dims)) and rrt.probe_grid is not None


# ---- the bake model -----------------------------------------------------------------------------------------------------------------
_cases = {}


def _case(rrt, orc, kind):
    if kind not in _cases:
        tris, mats, texs = PM.case_scene(rrt, kind)
        sc = rrt.Scene.from_arrays(tris, mats, texs)                                          # the tree built on the host
        _cases[kind] = (sc, PM.Bake(orc, sc), PM.case_probes(sc.tris))
    return _cases[kind]


# Which coefficients the bound of the next test can speak for at which N -- from the expressions alone.  The bound charges every
# rounding against sum |L * Y_k|.  That is what a product, an addition, the division and the factor 4 pi cost, and what evaluating
# Y_k costs where Y_k is a product of its inputs (k = 0 ... 5, 7).  Y_6 = K6 * (3 z^2 - 1) and Y_8 = K8 * (x^2 - y^2) end in a
# subtraction, whose error is relative to its OPERANDS: up to about (3 * 3 z^2 + 1) u K6 <= 3.2 u per sample however small |Y_6| is
# (u = 2^-24).  Over N samples that is at most 3.2 u N |L| against a bound of (2 N + 6) u * N E|Y_6| |L| with E|Y_6| about 0.25 over the
# sphere: the bound covers it with a factor (2 N + 6) / 12.8 to spare -- 10 at N = 64, 40 at N = 256, but less than 1 at N = 1 and
# about 1 at N = 3, where a direction near a node of Y_6 or Y_8 breaks it for ANY f32 evaluation of the header's expression.  So k = 6
# and 8 are held to the bound at N = 64 and 256, the other seven at every N.  Measured on these probes (error / bound, worst probe and
# channel): N = 1: 0.44 over k != 6, 8; k = 6: 2.42, k = 8: 0.71.  N = 3: 0.41.  N = 64: 0.075.  N = 256: 0.070.
PRODUCT_FORM = [0, 1, 2, 3, 4, 5, 7]


@pytest.mark.parametrize("n", [1, 3, 64, 256])
def test_bake_model_against_a_float64_projection(rrt, orc, n):
    """The f32 ordered sums against the textbook Monte-Carlo estimate in float64 over the same directions and radiances, within
    (N + 3) 2^-23 * sum |L * Y| * 4 pi / N per coefficient and channel (which coefficients at which N: the comment above)."""
    _, model, probes = _case(rrt, orc, "cornell")
    ok = np.ones(len(probes), dtype=bool)
    ok[list(PM.PLANTED_NAN)] = False
    pr = probes[ok][:12] if n == 256 else probes[ok]
    ks = list(range(9)) if n >= 64 else PRODUCT_FORM
    out = model.run(pr, n, 4)
    worst = np.zeros(9)
    for i in range(len(pr)):
        want = PM.project64(out["dirs"][i], out["radiance"][i])
        mag = 4 * np.pi / n * np.einsum("sk,sc->kc", np.abs(PM.basis64(out["dirs"][i])), np.abs(out["radiance"][i].astype(np.float64)))
        bound = (n + 3) * 2.0 ** -23 * mag
        err = np.abs(out["mean"][i].astype(np.float64) - want)
        with np.errstate(all="ignore"):
            worst = np.maximum(worst, np.where(bound > 0, err / bound, err > 0).max(axis=1))
        assert np.all(err[ks] <= bound[ks]), (n, i, (err / bound)[ks])
    print(f"[probe] N = {n}: error / bound per coefficient, worst probe and channel: {np.round(worst, 3).tolist()}")
    assert np.any(out["mean"][:, 1:] != 0)


@pytest.mark.parametrize("kind", PM.KINDS)
def test_every_gpu_scene_meets_the_conditions_on_the_model_alone(rrt, orc, kind):
    sc, model, probes = _case(rrt, orc, kind)
    assert len(sc.tris) >= 64 and len(probes) == PM.N_PROBES
    for shading in (0, 1):
        out = model.run(probes, 3, 4, shading=shading)
        PM.conditions(out, PM.PLANTED_NAN)
        assert not np.any(np.isnan(out["sum"]))                                               # a non-finite origin sees the sky: no NaN is planted
        assert out["hit"][PM.I_INSIDE].all()                                                   # nothing leaves the closed cube on the first segment
    d = model.run(probes, 1, 1)["dirs"][:, 0]
    assert PM.same_bits(d[PM.I_ZERO0], d[PM.I_ZERO1])                                          # both zero seeds run on stream 1
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6               # unit vectors as drawn


def test_split_sums_continue_the_single_sum(rrt, orc):
    _, model, probes = _case(rrt, orc, "helmet")
    whole = model.run(probes[:16], 8, 4, stride=65)["sum"]
    for split in ((4, 4), (1, 5, 2)):
        acc, first = None, 0
        for k in split:
            acc = model.run(probes[:16], k, 4, stride=65, first_sample=first, start=acc)["sum"]
            first += k
        assert PM.same_bits(acc, whole), split
