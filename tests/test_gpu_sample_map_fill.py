"""-m gpu: mipt_sample_map_fill / mipt_sample_map_fill_device (csrc/sample_map.hip, sample_map_fill_kernel) equal the numpy model of
tests/tools/sample_map_fill_model.py on every u32 count for 1, 2, 4 and 8 rounds, stay within the budget, never fall as rounds grow,
equal mipt_sample_map_device at one round, and the device entry writes nothing but `counts` and a workspace of exactly
mipt_sample_map_fill_workspace_bytes() -- also on a plane of more pixels than one launch has threads (2048 x 256)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import sample_map_fill_model as FM  # noqa: E402
import sample_map_model as SM  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 37, 200)]        # V, H, W: one pixel, less than one block, several blocks in the sums
ROUNDS = (1, 2, 4, 8)
TRIPLES = ((1, 8, 2.0), (0, 16, 1.5), (1, 65535, 700.5), (2, 6, 5.5))
CAP = 2048 * 256


def _planes(shape, seed):
    """ordinary values mixed with NaN, +-inf, negatives, denormals and zeros, and a few pixels far noisier than the rest, which
    saturate in round 1 and leave their share to the later rounds"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    variance = (rng.random(shape) ** 4 * 2.0).astype(F)
    hdr = (rng.random(shape + (3,)) ** 2 * 3.0).astype(F)
    albedo = rng.random(shape + (3,)).astype(F)
    odd = np.array([np.nan, np.inf, -np.inf, -1.0, 1e-42, -1e-42, 0.0, -0.0, 1e-20, 3e38], dtype=F)
    if n > 1:
        flat = variance.reshape(-1)
        loud = rng.choice(n, size=max(1, n // 16), replace=False)
        flat[loud] = (flat[loud] * 4000.0).astype(F)
        for a in (variance, hdr, albedo):
            flat = a.reshape(-1)
            idx = rng.choice(flat.size, size=min(flat.size // 3, 40), replace=False)
            flat[idx] = odd[rng.integers(0, odd.size, idx.size)]
        variance.reshape(-1)[0] = 0.25
        hdr.reshape(-1, 3)[0] = (0.5, 0.5, 0.5)
        albedo.reshape(-1, 3)[0] = (0.5, 0.5, 0.5)
    return variance, hdr, albedo


def _options(L, shape, lo, hi, budget, rounds):
    v, h, w = shape
    opt = L.MiptSampleMapFillOptions()
    opt.width, opt.height, opt.n_views, opt.min_samples, opt.max_samples, opt.budget, opt.rounds = w, h, v, lo, hi, budget, rounds
    return opt


def _host(rrt, variance, hdr, albedo, lo, hi, budget, rounds):
    from rust_ray_tracing_amd import _lib as L
    counts = np.full(variance.size + 2, 0xdeadbeef, dtype=np.uint32)
    bufs = L.MiptSampleMapBuffers()
    bufs.variance, bufs.counts = variance.ctypes.data, counts.ctypes.data + 4
    bufs.hdr = hdr.ctypes.data if hdr is not None else None
    bufs.albedo = albedo.ctypes.data if albedo is not None else None
    L.check(rrt.load().mipt_sample_map_fill(C.byref(_options(L, variance.shape, lo, hi, budget, rounds)), C.byref(bufs), 0), "mipt_sample_map_fill")
    assert counts[0] == 0xdeadbeef and counts[-1] == 0xdeadbeef
    return counts[1:-1].reshape(variance.shape)


def _device(rrt, variance, hdr, albedo, lo, hi, budget, rounds, plain=False):
    """the device entry (plain: mipt_sample_map_device) with guard bands around counts and around a workspace of exactly the size the
    library asks for -> (counts, guards and inputs untouched?)"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    v, h, w = variance.shape
    n = variance.size
    guard = 64
    need = int(lib.mipt_sample_map_workspace_bytes(w, h, v) if plain else lib.mipt_sample_map_fill_workspace_bytes(w, h, v, rounds))
    assert need == (32 if plain else 32 * rounds)
    t = {k: torch.from_numpy(a).cuda() for k, a in (("variance", variance), ("hdr", hdr), ("albedo", albedo)) if a is not None}
    before = {k: a.clone() for k, a in t.items()}
    d_counts = torch.full((guard + n + guard,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    d_work = torch.full((guard + need // 4 + guard,), 0x3c3c3c3c, dtype=torch.int32, device="cuda")
    bufs = L.MiptSampleMapBuffers()
    for k, a in t.items():
        setattr(bufs, k, a.data_ptr())
    bufs.counts = d_counts.data_ptr() + guard * 4
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    work, raw = C.c_void_p(d_work.data_ptr() + guard * 4), C.c_void_p(stream.cuda_stream)
    if plain:
        opt = L.MiptSampleMapOptions()
        opt.width, opt.height, opt.n_views, opt.min_samples, opt.max_samples, opt.budget = w, h, v, lo, hi, budget
        L.check(lib.mipt_sample_map_device(C.byref(opt), C.byref(bufs), work, raw), "mipt_sample_map_device")
    else:
        L.check(lib.mipt_sample_map_fill_device(C.byref(_options(L, variance.shape, lo, hi, budget, rounds)), C.byref(bufs), work, raw),
                "mipt_sample_map_fill_device")
    stream.synchronize()
    c, wk = d_counts.cpu().numpy(), d_work.cpu().numpy()
    clean = (np.all(c[:guard] == 0x5a5a5a5a) and np.all(c[guard + n:] == 0x5a5a5a5a) and np.all(wk[:guard] == 0x3c3c3c3c) and
             np.all(wk[guard + need // 4:] == 0x3c3c3c3c) and all(torch.equal(a.view(torch.int32), before[k].view(torch.int32)) for k, a in t.items()))
    return c[guard:guard + n].view(np.uint32).reshape(variance.shape), bool(clean)


@pytest.mark.parametrize("buffers", ["variance", "hdr", "albedo"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_kernels_equal_the_model(rrt, shape, buffers):
    variance, hdr, albedo = _planes(shape, sum(shape))
    hdr = hdr if buffers != "variance" else None
    albedo = albedo if buffers == "albedo" else None
    moved = 0
    for lo, hi, budget in TRIPLES:
        t, last = SM.total(budget, variance.size), None
        for rounds in ROUNDS:
            want = FM.fill(variance, hdr, albedo, lo, hi, budget, rounds)
            got_h = _host(rrt, variance, hdr, albedo, lo, hi, budget, rounds)
            got_d, clean = _device(rrt, variance, hdr, albedo, lo, hi, budget, rounds)
            assert np.array_equal(got_h, want), (lo, hi, budget, rounds, int(np.count_nonzero(got_h != want)))
            assert np.array_equal(got_d, want) and clean, (lo, hi, budget, rounds, int(np.count_nonzero(got_d != want)))
            assert got_d.min() >= lo and got_d.max() <= hi and int(got_d.sum(dtype=np.uint64)) <= t
            if last is not None:
                assert np.all(got_d >= last)
                moved += int(np.count_nonzero(got_d != last))
            last = got_d
        plain, clean = _device(rrt, variance, hdr, albedo, lo, hi, budget, 1, plain=True)
        assert clean and np.array_equal(plain, FM.fill(variance, hdr, albedo, lo, hi, budget, 1))          # rounds = 1 is mipt_sample_map_device
    assert moved > 0 or variance.size == 1                                   # a condition on the input: later rounds had something to do


def test_hostile_planes(rrt):
    """S == 0 (zeros, NaN, negatives), one noisy pixel, budget == min, budget == max, every pixel saturated after round 1"""
    shape = (2, 37, 200)
    zero = np.zeros(shape, dtype=F)
    zero[0, 0, :4] = [np.nan, -1.0, -np.inf, -0.0]
    one = np.zeros(shape, dtype=F)
    one[1, 20, 100] = 1.0
    few = np.zeros(shape, dtype=F)
    few[:, ::9, ::50] = 0.3
    flat = np.full(shape, 0.5, dtype=F)
    ordinary = _planes(shape, 5)[0]
    cases = [(zero, 1, 8, 3.75), (zero, 0, 8, 0.5), (one, 0, 9, 2.0), (few, 1, 7, 3.0), (flat, 1, 6, 6.0), (flat, 4, 4, 4.0),
             (ordinary, 2, 8, 2.0), (ordinary, 1, 8, 8.0), (ordinary, 0, 3, 2.9)]
    for variance, lo, hi, budget in cases:
        for rounds in (2, 8):
            want = FM.fill(variance, None, None, lo, hi, budget, rounds)
            got, clean = _device(rrt, variance, None, None, lo, hi, budget, rounds)
            assert np.array_equal(got, want) and clean, (lo, hi, budget, rounds, int(np.count_nonzero(got != want)))
            assert np.array_equal(_host(rrt, variance, None, None, lo, hi, budget, rounds), want)
            assert int(got.sum(dtype=np.uint64)) <= SM.total(budget, variance.size)
    assert np.all(FM.fill(zero, None, None, 1, 8, 3.75, 8) == 3) and int(FM.fill(one, None, None, 0, 9, 2.0, 8).sum()) == 9


def test_past_the_grid_cap(rrt):
    """524 799 pixels: 511 threads take a second trip in every pass.  A third of the pixels are loud enough to saturate in round 1,
    in both trips; rounds = 3, so that a pass that reads, one that reads and sums, and the last all walk past the cap."""
    shape = (1, 513, 1023)
    n = int(np.prod(shape))
    assert CAP < n < CAP + 2 * 256
    rng = np.random.default_rng(41)
    variance = (rng.random(shape) ** 4 * 1e-3).astype(F)
    flat = variance.reshape(-1)
    flat[::3] = (4.0 + rng.random(flat[::3].size)).astype(F)
    flat[CAP:CAP + 8] = [np.nan, np.inf, -1.0, 1e-42, 0.0, 3e38, 0.25, 5.0]
    lo, hi, budget = 1, 8, 4.0
    first = FM.fill(variance, None, None, lo, hi, budget, 1)
    sat = first.reshape(-1) == hi
    assert 0.3 * n < sat.sum() < 0.4 * n and sat[CAP:].any() and (~sat[CAP:]).any()      # conditions on the input
    trace = []
    want = FM.fill(variance, None, None, lo, hi, budget, 3, trace)
    assert all(tr["active"] for tr in trace) and np.unique(want.reshape(-1)[CAP:]).size > 2
    assert np.count_nonzero(want.reshape(-1)[CAP:] != first.reshape(-1)[CAP:]) > 100        # the later trips are raised too
    got_d, clean = _device(rrt, variance, None, None, lo, hi, budget, 3)
    assert np.array_equal(got_d, want) and clean, int(np.count_nonzero(got_d != want))
    assert np.array_equal(_host(rrt, variance, None, None, lo, hi, budget, 3), want)
    assert int(first.sum(dtype=np.uint64)) < int(got_d.sum(dtype=np.uint64)) <= SM.total(budget, n)


def test_renderer_mirror(rrt):
    import torch
    variance, hdr, albedo = _planes((2, 37, 200), 77)
    r = rrt.Renderer.new(rrt.RendererOptions(samples=8, max_ray_depth=2, output_image_dimensions=(200, 37), output_image_path="/dev/null"))
    want = FM.fill(variance, hdr, albedo, 1, 8, 2.0, 4)
    assert not np.array_equal(want, SM.sample_map(variance, hdr, albedo, 1, 8, 2.0))
    assert np.array_equal(r.sample_map(variance, hdr, albedo, budget=2.0, rounds=4), want)
    got = r.sample_map(torch.from_numpy(variance).cuda(), torch.from_numpy(hdr).cuda(), torch.from_numpy(albedo).cuda(), budget=2.0, rounds=4)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(r.sample_map(variance, hdr, albedo, budget=2.0, rounds=1), r.sample_map(variance, hdr, albedo, budget=2.0))
