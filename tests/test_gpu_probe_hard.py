"""GPU: mipt_probe_bake / mipt_probe_irradiance and their _device forms (csrc/probe.hip, mipt::chunked_trace) where
tests/test_gpu_probe.py does not go.  A: a probe that straddles a chunk edge under MIPT_FLAG_ACCUM, a chunk edge that falls exactly
between two probes after a call that left a carry slot non-zero, the batch loop, the tail loop and a carry slot in one span, the
counters of a call of more than one chunk, and the chunk staging after it grew.  B: the hard probes of tests/tools/hard_inputs.py --
an origin shared by all of a probe's samples on both sides of every origin clause of ray_safe, on vertices, edges, triangles, node
planes and corners -- alone, among ordinary probes and as whole waves, and on a scene whose tiny planes switch the zero-origin clause
off.  C: the lookup on grids that do not divide back, with spacings whose quotients overflow and go denormal, non-finite words behind
invalid probes, every `valid` byte and a weight sum below 2^-60.  Everything is compared with tests/tools/probe_model.py bit for bit,
two produced NaNs counting as equal (H.differing), with a sentinel behind every output; tests/test_probe_model.py and
tests/test_hard_inputs_model.py (CPU) hold the model alone to its conditions on the same inputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import hard_inputs as H  # noqa: E402
import probe_model as PM  # noqa: E402
import test_gpu_bake as TB  # noqa: E402
from test_gpu_probe import CULL, KEYS, PERIOD, REF, SAFE, SENTINEL, _bake, _case, _dev, _from_triangles, _lookup, _periodic  # noqa: E402
from test_gpu_radiance_hard import _tiny_plane_scene  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
ARMS = ((REF, 0.0), (CULL, 0.0), (CULL, SAFE))
CHUNK = 1 << 22                                # mipt::kChunkPaths
K_BATCH = 16                                   # probe.hip: kBatch
LOOKUP_HARD_SEED = 7                           # tests/test_probe_model.py holds the model to its conditions at this seed
_models, _hard = {}, {}


def _run(rrt, orc, kind, tag, probes, samples, depth, **kw):
    """PM.Bake.run on the scene of `kind`, once per (kind, tag)"""
    key = (kind, tag)
    if key not in _models:
        with np.errstate(all="ignore"):
            _models[key] = _case(rrt, orc, kind)[1].run(probes, samples, depth, **kw)
    return _models[key]


def _expand(period_probes, index):
    import torch
    return _dev(period_probes)[torch.from_numpy(index).cuda()].contiguous()


def _preset_period():
    """what an ACCUM call finds in the buffer, per member of the period: f32(i mod 251) + 0.5 in all 27 words"""
    return np.ascontiguousarray(np.broadcast_to((F(0.5) + (np.arange(PERIOD) % 251).astype(np.float32))[:, None, None], (PERIOD, 9, 3)))


def _preset_buffer(index, extra=5):
    import torch
    n = len(index)
    buf = torch.empty((n * 27 + extra,), dtype=torch.float32, device="cuda")
    buf[: n * 27] = torch.from_numpy(_preset_period()[:, 0, 0].copy()).cuda()[torch.from_numpy(index).cuda()].repeat_interleave(27)
    buf = buf.view(torch.int32)
    buf[n * 27:] = SENTINEL
    return buf


def _named(got, want_rows, index, named):
    return [(i, PM.same_bits(got[i], want_rows[index[i]])) for i in named]


def _bad(got, want):
    g, w = (np.ascontiguousarray(a).reshape(len(a), -1) for a in (got, want))
    bad = np.flatnonzero(H.differing(g, w).any(axis=1))
    return len(bad), [(int(i), g[i][:6].view(np.uint32).tolist(), w[i][:6].view(np.uint32).tolist()) for i in bad[:3]]


def _weighted_counters(model, index):
    """the sum of the model's per-probe counters over the index list"""
    return np.bincount(index, minlength=PERIOD).astype(np.int64) @ model["counters"]


# ---- A. chunks and carry --------------------------------------------------------------------------------------------------------------
def test_accumulate_into_a_probe_that_straddles_a_chunk_edge(rrt, orc):
    """2^22 + 65 paths at 3 samples, SUM | ACCUM from a preset: the straddler starts its first chunk from the buffer and its second
    from the carry slot, never from the buffer again.  Then the next three samples into the same buffer."""
    from rust_ray_tracing_amd import _lib as L
    sc, _, _, _ = _case(rrt, orc, "cornell")
    samples = 3
    n = (CHUNK + 65 + samples - 1) // samples
    straddler = CHUNK // samples
    assert straddler * samples < CHUNK < (straddler + 1) * samples and n * samples >= CHUNK + 65
    pr, index = _periodic(rrt, orc, n)
    start = _preset_period()
    first = _run(rrt, orc, "cornell", "accum 0..2", pr, samples, 2, stride=n, start=start)
    second = _run(rrt, orc, "cornell", "accum 3..5", pr, samples, 2, stride=n, first_sample=3, start=first["sum"])
    plain = _run(rrt, orc, "cornell", "plain 0..2", pr, samples, 2, stride=n)
    assert not np.isnan(second["sum"]).any() and np.any(first["sum"] != start) and np.any(first["sum"] != plain["sum"])
    assert np.any(second["sum"] != first["sum"]) and index[straddler] % 251 != 0
    d_p = _expand(pr, index)
    d_acc = _preset_buffer(index)
    named = [straddler - 1, straddler, straddler + 1, n - 1]
    for k, want in ((0, first["sum"]), (3, second["sum"])):
        rc, got, st = _bake(rrt, sc, np.empty(n, dtype=PM.PROBE), samples, 2, flags=L.FLAG_SUM | L.FLAG_ACCUM, device=True, d_probes=d_p, d_out=d_acc,
                            first_sample=k)
        assert rc == 0 and st["pixels"] == n * samples
        assert all(ok for _, ok in _named(got, want, index, named)), (k, _named(got, want, index, named))
        assert PM.same_bits(got, want[index]), (k, _bad(got, want[index]))


def test_a_chunk_edge_between_two_probes_ignores_the_carry_slot(rrt, orc):
    """After a straddling call has left a probe's partial sums in the carry slot the next chunk reads, 2^20 + 17 probes at 4 samples:
    path 2^22 is the first of probe 2^20, which must start from +0 (or from the buffer), and the five counters are the model's sums."""
    from rust_ray_tracing_amd import _lib as L
    sc, _, _, _ = _case(rrt, orc, "cornell")
    n3 = (CHUNK + 65 + 2) // 3
    pr3, index3 = _periodic(rrt, orc, n3)
    part = _case(rrt, orc, "cornell")[1].run(pr3[index3[CHUNK // 3]: index3[CHUNK // 3] + 1], CHUNK % 3, 2, stride=n3)["sum"]
    assert CHUNK % 3 == 1 and np.all(part[0, 0] != 0)                               # what the straddler leaves in its slot is not 0
    rc, _, st = _bake(rrt, sc, np.empty(n3, dtype=PM.PROBE), 3, 2, device=True, d_probes=_expand(pr3, index3))
    assert rc == 0 and st["pixels"] == n3 * 3
    samples = 4
    n = (1 << 20) + 17
    assert CHUNK % samples == 0 and CHUNK // samples == 1 << 20 and n * samples > CHUNK      # the edge: between probes 2^20 - 1 and 2^20
    pr, index = _periodic(rrt, orc, n)
    plain = _run(rrt, orc, "cornell", "edge plain", pr, samples, 2, stride=n)
    accum = _run(rrt, orc, "cornell", "edge accum", pr, samples, 2, stride=n, start=_preset_period())
    PM.conditions(plain, PM.PLANTED_NAN)
    counters = _weighted_counters(plain, index)
    assert np.array_equal(plain["counters"], accum["counters"]) and np.all(counters[:4] > 0)                  # cornell has no texture to fetch from
    d_p = _expand(pr, index)
    named = [(1 << 20) - 1, 1 << 20, n - 1]
    for flags, want, d_out in ((L.FLAG_COUNT, plain["mean"], None), (L.FLAG_COUNT | L.FLAG_SUM | L.FLAG_ACCUM, accum["sum"], _preset_buffer(index))):
        rc, got, st = _bake(rrt, sc, np.empty(n, dtype=PM.PROBE), samples, 2, flags=flags, device=True, d_probes=d_p, d_out=d_out)
        assert rc == 0 and st["pixels"] == n * samples and st["stack_overflows"] == 0
        assert all(ok for _, ok in _named(got, want, index, named)), (flags, _named(got, want, index, named))
        assert PM.same_bits(got, want[index]), (flags, _bad(got, want[index]))
        assert {k: st[k] for k in KEYS} == dict(zip(KEYS, counters.tolist())), (flags, st, counters)


@pytest.mark.parametrize("samples", [17, 37])
def test_batch_then_tail_against_the_model(rrt, orc, samples):
    """one batch and a tail of 1; two batches and a tail of 5 -- 65 probes, both entries, mean and sum"""
    from rust_ray_tracing_amd import _lib as L
    assert samples // K_BATCH >= 1 and samples % K_BATCH != 0
    sc, _, _, pr = _case(rrt, orc, "helmet")
    want = _run(rrt, orc, "helmet", ("tail", samples), pr, samples, 4)
    PM.conditions(want, PM.PLANTED_NAN)
    for device in (False, True):
        for flags, key in ((0, "mean"), (L.FLAG_SUM, "sum")):
            rc, got, st = _bake(rrt, sc, pr, samples, 4, flags=flags, device=device)
            assert rc == 0 and st["pixels"] == len(pr) * samples
            assert PM.same_bits(got, want[key]), (samples, device, flags, _bad(got, want[key]))


def test_batch_tail_and_carry_in_one_probe(rrt, orc):
    """2^22 + 65 paths at 37 samples: the straddler adds 21 samples before the edge -- one batch and a tail of 5 -- and 16 behind it,
    exactly one batch that goes on from the carry slot."""
    sc, _, _, _ = _case(rrt, orc, "cornell")
    samples = 37
    before = CHUNK % samples
    assert before == 21 and before // K_BATCH == 1 and before % K_BATCH == 5 and samples - before == K_BATCH
    n = (CHUNK + 65 + samples - 1) // samples
    straddler = CHUNK // samples
    assert straddler * samples + before == CHUNK and n > straddler + 1
    pr, index = _periodic(rrt, orc, n)
    want = _run(rrt, orc, "cornell", "period 37", pr, samples, 1, stride=n)
    PM.conditions(want, PM.PLANTED_NAN)
    rc, got, st = _bake(rrt, sc, np.empty(n, dtype=PM.PROBE), samples, 1, device=True, d_probes=_expand(pr, index))
    assert rc == 0 and st["pixels"] == n * samples
    named = [straddler - 1, straddler, straddler + 1, n - 1]
    assert all(ok for _, ok in _named(got, want["mean"], index, named)), _named(got, want["mean"], index, named)
    assert PM.same_bits(got, want["mean"][index]), _bad(got, want["mean"][index])


def test_staging_that_grows_and_is_used_small_again(rrt, orc):
    """One fresh scene: a small bake, a bake of more than one chunk, the small bake, a gather, the small bake -- the chunk staging and
    the carry slots are the scene's, shared by both entries, and sized by the largest call so far."""
    sc0, model, caller, pr = _case(rrt, orc, "cornell")
    _, mats, texs = PM.case_scene(rrt, "cornell")
    sc, _ = _from_triangles(rrt, caller, mats, texs)
    assert np.array_equal(sc.tris, sc0.tris) and np.array_equal(sc.bvh_nodes, sc0.bvh_nodes)        # the same tree: the same model
    want = _run(rrt, orc, "cornell", "small", pr, 3, 2)
    pts = TB._random_points(caller, 40, 6)
    fresh, _ = _from_triangles(rrt, caller, mats, texs)
    rc, gather_fresh, _ = TB._gather(rrt, fresh, pts, 5, 2, device=True)
    assert rc == 0 and np.any(gather_fresh != 0)

    def small(step):
        for device in (False, True):
            rc, got, _ = _bake(rrt, sc, pr, 3, 2, device=device)
            assert rc == 0 and PM.same_bits(got, want["mean"]), (step, device, _bad(got, want["mean"]))
    small("first")
    n = (CHUNK + 65 + 2) // 3
    prp, index = _periodic(rrt, orc, n)
    big = _run(rrt, orc, "cornell", "plain 0..2", prp, 3, 2, stride=n)
    rc, got, st = _bake(rrt, sc, np.empty(n, dtype=PM.PROBE), 3, 2, device=True, d_probes=_expand(prp, index))
    assert rc == 0 and st["pixels"] == n * 3 and PM.same_bits(got, big["mean"][index])
    small("after the large bake")
    rc, got, _ = TB._gather(rrt, sc, pts, 5, 2, device=True)
    assert rc == 0 and PM.same_bits(got, gather_fresh), TB._bad_rows(got, gather_fresh)
    small("after the gather")


# ---- B. hard probes -------------------------------------------------------------------------------------------------------------------
N_POOL = 4 * 63


def _hard_probes(rrt, orc, kind):
    """(the hard probes, their tags, 4 x as many ordinary ones) on the scene of `kind`"""
    if kind not in _hard:
        sc, _, caller, _ = _case(rrt, orc, kind)
        hard, tags = H.hard_probes(sc.tris, sc.bvh_nodes, H.PROBE_SEED)
        _hard[kind] = (hard, tags, PM.case_probes(caller, n=N_POOL, seed=23))
    return _hard[kind]


def _check(rrt, sc, probes, want_rows, want_counters, samples, depth, shading, arm, what, first_sample, entries=(False, True)):
    """both entries, product and COUNT builds: every coefficient, and on the COUNT build all five counters"""
    from rust_ray_tracing_amd import _lib as L
    for device in entries:
        for flags in (0, L.FLAG_COUNT):
            rc, got, st = _bake(rrt, sc, probes, samples, depth, shading, arm[0], flags, device, first_sample=first_sample, stride=H.HARD_STRIDE,
                                cull_margin=arm[1])
            assert rc == 0 and st["stack_overflows"] == 0 and st["pixels"] == len(probes) * samples, (what, arm, device, flags, rc, st)
            assert H.same_bits_or_both_nan(got, want_rows), (what, arm, device, flags, _bad(got, want_rows))
            if flags:
                assert {k: st[k] for k in KEYS} == dict(zip(KEYS, want_counters.sum(0).tolist())), (what, arm, device, st, want_counters.sum(0))


@pytest.mark.parametrize("kind,shading", [("helmet", 0), ("helmet", 1), ("cornell", 0), ("wgsl_pbr", 1)])
def test_hard_probes(rrt, orc, kind, shading):
    """alone at first_sample 0 (both zero seeds run on stream 1), one to four among ordinary probes at HARD_FIRST_SAMPLE (the late
    zero seed's second sample does), and on cornell at 64 samples: every hard probe a whole wave of the ray kernel"""
    sc, _, _, _ = _case(rrt, orc, kind)
    hard, tags, pool = _hard_probes(rrt, orc, kind)
    samples, depth = 3, 8
    safe = H.origin_safe(hard)
    assert 3 * int((~safe).sum()) >= len(hard) and 6 * int(safe.sum()) >= len(hard)
    mixed, at, rest = H.spread(hard, pool)
    steps = []
    for arm in ARMS:
        kw = dict(shading=shading, cull=arm[0], margin=arm[1], stride=H.HARD_STRIDE)
        alone = _run(rrt, orc, kind, ("hard", 0, shading, arm), hard, samples, depth, **kw)
        late = _run(rrt, orc, kind, ("hard", H.HARD_FIRST_SAMPLE, shading, arm), hard, samples, depth, first_sample=H.HARD_FIRST_SAMPLE, **kw)
        mp = _run(rrt, orc, kind, ("pool", H.HARD_FIRST_SAMPLE, shading, arm), pool, samples, depth, first_sample=H.HARD_FIRST_SAMPLE, **kw)
        for out in (alone, late, mp):
            H.few_nan_rows(out)
        assert 4 * int(alone["hit"].any(axis=1).sum()) >= len(hard) and 4 * int((~alone["hit"]).any(axis=1).sum()) >= len(hard)
        steps.append(int(alone["counters"][:, 1].sum()))
        _check(rrt, sc, hard, alone["mean"], alone["counters"], samples, depth, shading, arm, (kind, "alone"), 0)
        rows, cnt = np.zeros((len(mixed), 9, 3), np.float32), np.zeros((len(mixed), 5), np.int64)
        rows[at], rows[rest], cnt[at], cnt[rest] = late["mean"], mp["mean"], late["counters"], mp["counters"]
        _check(rrt, sc, mixed, rows, cnt, samples, depth, shading, arm, (kind, "spread"), H.HARD_FIRST_SAMPLE)
    if kind == "helmet":
        assert len(set(steps)) == 3, steps                                          # the three arms are three different amounts of work
    if kind == "cornell":
        arm = ARMS[0]
        waves = _run(rrt, orc, kind, ("hard", "waves"), hard, 64, depth, shading=shading, stride=H.HARD_STRIDE)
        H.few_nan_rows(waves)
        _check(rrt, sc, hard, waves["mean"], waves["counters"], 64, depth, shading, arm, (kind, "waves"), 0)


def test_hard_probes_on_a_scene_with_tiny_planes(rrt, orc):
    sc = _tiny_plane_scene(rrt)
    planes = np.abs(np.concatenate([sc.bvh_nodes["bounds_min"], sc.bvh_nodes["bounds_max"]]))
    tiny = [bool(np.any((planes[:, k] != 0) & (planes[:, k] < 2.0 ** -76))) for k in range(3)]
    assert tiny == [True, False, True]                                              # tiny_axes = 0b101, restated from the nodes
    sc.upload(0)
    pr = H.tiny_plane_probes()
    m = PM.Bake(orc, sc)
    for arm in ((REF, 0.0), (CULL, SAFE)):
        with np.errstate(all="ignore"):
            want = m.run(pr, 3, 8, cull=arm[0], margin=arm[1], stride=H.HARD_STRIDE)
        rays = H.probe_rays(pr, want["dirs"])
        only = (H.ray_safe(rays, 0) & ~H.ray_safe(rays, 5)).reshape(len(pr), 3).all(axis=1)
        assert int(only.sum()) >= 12, int(only.sum())                               # probes only the scene's tiny planes take off the fast path
        safe = H.ray_safe(rays, 5)
        assert 4 * int(safe.sum()) >= len(rays) and 4 * int((~safe).sum()) >= len(rays) and 4 * int(want["hit"].sum()) >= len(rays)
        H.few_nan_rows(want)
        _check(rrt, sc, pr, want["mean"], want["counters"], 3, 8, 0, arm, "tiny planes", 0)


# ---- C. lookup ------------------------------------------------------------------------------------------------------------------------
_lookup_cases = []


def _hard_lookup_case(k):
    if not _lookup_cases:
        _lookup_cases.extend(PM.lookup_hard_case(LOOKUP_HARD_SEED))
    return _lookup_cases[k]


@pytest.mark.parametrize("k", range(len(PM.LOOKUP_HARD_NAMES)), ids=[s.replace(" ", "_") for s in PM.LOOKUP_HARD_NAMES])
def test_lookup_hard_cases(rrt, k):
    """every case of PM.lookup_hard_case: with and without its `valid` plane, with and without the clamp, both entries, all its
    points (no multiple of 64) and single points"""
    name = PM.LOOKUP_HARD_NAMES[k]
    grid, sh, valid, P, N = _hard_lookup_case(k)
    assert len(P) % 64 != 0
    planes = (valid,) if name.startswith("non-finite") else (None, valid)            # without its plane that grid is NaN all over
    for v in planes:
        for clamp in (False, True):
            want = PM.lookup(sh, grid, P, N, v, clamp)
            assert 10 * H.nan_rows(want) <= len(want) and not (clamp and (np.isnan(want).any() or np.any(want < 0))) and np.any(want > 0)
            for device in (False, True):
                got = _lookup(rrt, grid, sh, P, N, v, clamp, device)
                assert H.same_bits_or_both_nan(got, want), (name, v is not None, clamp, device, H.bad_rows(got, want))
    want = PM.lookup(sh, grid, P, N, valid, False)
    for i in (0, len(P) // 2, len(P) - 1):                                           # n = 1
        for device in (False, True):
            got = _lookup(rrt, grid, sh, P[i: i + 1], N[i: i + 1], valid, False, device)
            assert H.same_bits_or_both_nan(got, want[i: i + 1]), (name, i, device, got, want[i])


def test_lookup_never_reads_an_invalid_probe(rrt):
    """NaN, +-inf and the sentinel's bits in the coefficients of the invalid probes: the result is the model's, and the result of the
    same call with finite noise in their place, bit for bit -- a corner multiplied by a weight of 0 in place of the skip is a NaN"""
    grid, sh, valid, P, N = _hard_lookup_case(PM.LOOKUP_HARD_NAMES.index("non-finite words behind invalid probes"))
    assert not np.isfinite(sh[valid == 0]).any() and np.isfinite(sh[valid != 0]).all()
    noise = sh.copy()
    noise[valid == 0] = np.random.default_rng(3).normal(0, 1, noise[valid == 0].shape).astype(np.float32)
    for clamp in (False, True):
        want = PM.lookup(sh, grid, P, N, valid, clamp)
        assert 10 * H.nan_rows(want) <= len(want)
        for device in (False, True):
            got = _lookup(rrt, grid, sh, P, N, valid, clamp, device)
            other = _lookup(rrt, grid, noise, P, N, valid, clamp, device)
            assert H.same_bits_or_both_nan(got, want), (clamp, device, H.bad_rows(got, want))
            assert PM.same_bits(got, other), (clamp, device, H.bad_rows(got, other))


def test_lookup_divides_by_a_weight_sum_below_2_to_minus_60(rrt):
    grid, sh, valid, P, N = _hard_lookup_case(PM.LOOKUP_HARD_NAMES.index("one valid corner of tiny weight"))
    want, wsum = PM.lookup(sh, grid, P, N, valid, with_wsum=True)
    tiny = np.flatnonzero((wsum > 0) & (wsum < 2.0 ** -60))
    assert len(tiny) >= 4 and np.all(np.isfinite(want[tiny])) and np.all(want[tiny] != 0)
    for device in (False, True):
        got = _lookup(rrt, grid, sh, P, N, valid, False, device)
        assert PM.same_bits(got[tiny], want[tiny]), (device, got[tiny], want[tiny])
        assert H.same_bits_or_both_nan(got, want), (device, H.bad_rows(got, want))
