"""CPU: the numpy model of the filling sample map (tests/tools/sample_map_fill_model.py) obeys what include/mipt.h states for
mipt_sample_map_fill -- one round is the plain map, no count falls from one round count to the next, the sum never passes T, the
bounds hold on every hostile input -- and gives the counts worked out by hand on a plane whose first round saturates a known set.  The
kernels are held to the model bit for bit in tests/test_gpu_sample_map_fill.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import sample_map_fill_model as FM  # noqa: E402
import sample_map_model as SM  # noqa: E402

F = np.float32
ROUNDS = (1, 2, 3, 4, 8)
TRIPLES = [(1, 8, 2.0), (0, 16, 1.5), (2, 2, 2.0), (1, 65535, 300.25), (3, 9, 9.0), (2, 8, 2.0), (0, 5, 4.75)]


def _planes(seed, shape=(2, 9, 13)):
    rng = np.random.default_rng(seed)
    variance = (rng.random(shape) ** 4).astype(F)
    hdr = (rng.random(shape + (3,)) ** 2 * 3.0).astype(F)
    albedo = rng.random(shape + (3,)).astype(F)
    return variance, hdr, albedo


def _hostile():
    """the kinds of tests/test_sample_map_model.py: NaN, +-inf, negatives, denormals, S == 0, one noisy pixel, a few very noisy ones"""
    variance, hdr, albedo = _planes(9, (1, 4, 8))
    variance[0, 0, :6] = [np.nan, -1.0, np.inf, -np.inf, 1e-42, 0.0]
    hdr[0, 1, :4, 0] = [0.0, -3.0, np.nan, np.inf]
    albedo[0, 2, :4, 1] = [0.0, np.nan, -1.0, np.inf]
    one = np.zeros((1, 6, 6), dtype=F)
    one[0, 3, 3] = 4.0
    few = (np.random.default_rng(4).random((2, 9, 13)) ** 8 * 1e-3).astype(F)
    few[:, ::4, ::5] = 2.0
    yield "odd values", variance, hdr, albedo
    yield "odd values, variance alone", variance, None, None
    yield "zero sum", np.zeros((3, 5, 7), dtype=F), None, None
    yield "all NaN", np.full((2, 2), np.nan, dtype=F), None, None
    yield "one noisy pixel", one, None, None
    yield "a few saturate", few, None, None
    yield "ordinary", *_planes(3)


@pytest.mark.parametrize("with_hdr,with_albedo", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("lo,hi,budget", TRIPLES)
def test_one_round_is_the_plain_map(with_hdr, with_albedo, lo, hi, budget):
    variance, hdr, albedo = _planes(lo * 100 + hi)
    args = (variance, hdr if with_hdr else None, albedo if with_albedo else None, lo, hi, budget)
    assert np.array_equal(FM.fill(*args, rounds=1), SM.sample_map(*args))


@pytest.mark.parametrize("lo,hi,budget", TRIPLES)
def test_bounds_budget_and_monotone_in_rounds(lo, hi, budget):
    """every count in [min, max]; the sum at most T after every round count; no single count falls as rounds grow, so neither does
    the sum; and once a round changes nothing, none after it does"""
    for name, variance, hdr, albedo in _hostile():
        last, t = None, SM.total(budget, variance.size)
        for rounds in ROUNDS:
            trace = []
            counts = FM.fill(variance, hdr, albedo, lo, hi, budget, rounds, trace)
            assert counts.dtype == np.uint32 and counts.shape == variance.shape, name
            assert counts.min() >= lo and counts.max() <= hi, (name, rounds)
            assert int(counts.sum(dtype=np.uint64)) <= t, (name, rounds, int(counts.sum(dtype=np.uint64)), t)
            if last is not None:
                assert np.all(counts >= last), (name, rounds)
            idle = [k for k, tr in enumerate(trace) if not tr["active"]]
            assert not idle or idle == list(range(idle[0], len(trace))), (name, trace)
            last = counts


def test_the_budget_ends():
    variance, hdr, albedo = _planes(5)
    for rounds in ROUNDS:
        assert np.all(FM.fill(variance, hdr, albedo, 2, 8, 2.0, rounds) == 2)          # budget == min: E = 0
        assert np.all(FM.fill(variance, hdr, albedo, 2, 8, 8.0, 8) >= 2)
    # budget == max: E = span * N; all but the noiseless pixels end at max once the cut-off share is handed on
    v = variance.copy()
    v[0, 0, 0] = 0.0
    full = FM.fill(v, None, None, 1, 8, 8.0, 8)
    assert full[0, 0, 0] == 1 and int(np.count_nonzero(full == 8)) > int(np.count_nonzero(FM.fill(v, None, None, 1, 8, 8.0, 1) == 8))
    # S == 0: the uniform value, and no later round has anything to tell the pixels apart by
    z = np.zeros((3, 5, 7), dtype=F)
    for rounds in ROUNDS:
        assert np.all(FM.fill(z, None, None, 1, 8, 3.75, rounds) == 3)


def test_more_rounds_spend_more_of_the_budget():
    """the plane of DESIGN's measurement in small: a few pixels far noisier than the rest saturate in round 1, and what they cannot
    take reaches the others from round 2 on"""
    rng = np.random.default_rng(21)
    variance = (rng.random((1, 24, 32)) ** 6 * 1e-2).astype(F)
    variance[0, ::5, ::7] = 4.0
    t = SM.total(2.0, variance.size)
    spent = [int(FM.fill(variance, None, None, 1, 8, 2.0, r).sum(dtype=np.uint64)) for r in (1, 2, 4)]
    assert spent[0] < spent[1] <= spent[2] <= t and spent[0] < 0.9 * t


def test_round_two_by_hand():
    """Six pixels, min 0, max 4, budget 2: T = E = 12, span 4.  The standard deviations 2, 1, 1/4, 1/4, 1/4, 1/4 give
    qi = 8192, 4096, 1024 x 4 and S = 16384, r = 12 / 16384 (a power of two times 3: every product below is exact).
    Round 1: x = 6, 3, 0.75 x 4 -> e_1 = 4 (clamped), 3, 0, 0, 0, 0; 5 of the budget's samples are cut off.
    Round 2: A = 7, E_2 = 5, S_2 = 4096 + 4096 = 8192 over the five pixels below the span, r_2 = 5 / 8192;
             x = 2.5 (room 1 -> add 1), 0.625 x 4 (add 0) -> e_2 = 4, 4, 0, 0, 0, 0.
    Round 3: A = 8, E_3 = 4, S_3 = 4096, r_3 = 4 / 4096; x = 1 for each of the four -> e_3 = 4, 4, 1, 1, 1, 1: the budget is met."""
    variance = np.array([[4.0, 1.0, 0.0625, 0.0625, 0.0625, 0.0625]], dtype=F)
    assert SM.weights(variance).tolist() == [[8192, 4096, 1024, 1024, 1024, 1024]]
    assert FM.fill(variance, None, None, 0, 4, 2.0, 1).tolist() == [[4, 3, 0, 0, 0, 0]]
    trace = []
    assert FM.fill(variance, None, None, 0, 4, 2.0, 2, trace).tolist() == [[4, 4, 0, 0, 0, 0]]
    assert trace == [dict(A=7, S=8192, E=5, r=5.0 / 8192.0, active=True)]
    trace = []
    assert FM.fill(variance, None, None, 0, 4, 2.0, 3, trace).tolist() == [[4, 4, 1, 1, 1, 1]]
    assert trace[1] == dict(A=8, S=4096, E=4, r=4.0 / 4096.0, active=True)
    trace = []
    assert FM.fill(variance, None, None, 0, 4, 2.0, 5, trace).tolist() == [[4, 4, 1, 1, 1, 1]]
    assert [tr["active"] for tr in trace] == [True, True, False, False] and trace[2]["E"] == 0
    # with min_samples = 1 the same shares sit on top of the floor: T = 18, E = 12, span 4, max 5
    assert FM.fill(variance, None, None, 1, 5, 3.0, 3).tolist() == [[5, 5, 2, 2, 2, 2]]
