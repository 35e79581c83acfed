"""-m gpu: mipt_sample_map / mipt_sample_map_device equal the numpy model of tests/tools/sample_map_model.py on every u32 count, stay
within the budget, and the device entry writes nothing but `counts` and its workspace -- also on planes of more pixels than one
launch has threads (2048 x 256), where every further pixel is a thread's second trip, and with a sum of weights past 2^32."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import sample_map_model as SM  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 37, 200)]        # V, H, W: one pixel, less than one block, several blocks in the reduction


def _planes(shape, seed):
    """ordinary values mixed with NaN, +-inf, negatives, denormals and zeros"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    variance = (rng.random(shape) ** 4 * 2.0).astype(F)
    hdr = (rng.random(shape + (3,)) ** 2 * 3.0).astype(F)
    albedo = rng.random(shape + (3,)).astype(F)
    odd = np.array([np.nan, np.inf, -np.inf, -1.0, 1e-42, -1e-42, 0.0, -0.0, 1e-20, 3e38], dtype=F)
    if n > 1:
        for a in (variance, hdr, albedo):
            flat = a.reshape(-1)
            idx = rng.choice(flat.size, size=min(flat.size // 3, 40), replace=False)
            flat[idx] = odd[rng.integers(0, odd.size, idx.size)]
        variance.reshape(-1)[0] = 0.25                # at least one ordinary noisy pixel
        hdr.reshape(-1, 3)[0] = (0.5, 0.5, 0.5)
        albedo.reshape(-1, 3)[0] = (0.5, 0.5, 0.5)
    return variance, hdr, albedo


def _host(rrt, variance, hdr, albedo, lo, hi, budget):
    from rust_ray_tracing_amd import _lib as L
    v, h, w = variance.shape
    opt = L.MiptSampleMapOptions()
    opt.width, opt.height, opt.n_views, opt.min_samples, opt.max_samples, opt.budget = w, h, v, lo, hi, budget
    counts = np.full(variance.shape, 0xdeadbeef, dtype=np.uint32)
    bufs = L.MiptSampleMapBuffers()
    bufs.variance, bufs.counts = variance.ctypes.data, counts.ctypes.data
    bufs.hdr = hdr.ctypes.data if hdr is not None else None
    bufs.albedo = albedo.ctypes.data if albedo is not None else None
    L.check(rrt.load().mipt_sample_map(C.byref(opt), C.byref(bufs), 0), "mipt_sample_map")
    return counts


def _device(rrt, variance, hdr, albedo, lo, hi, budget):
    """the device entry with guard bands around counts and the workspace -> (counts, guards untouched?)"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    v, h, w = variance.shape
    n = variance.size
    opt = L.MiptSampleMapOptions()
    opt.width, opt.height, opt.n_views, opt.min_samples, opt.max_samples, opt.budget = w, h, v, lo, hi, budget
    guard = 64
    need = int(lib.mipt_sample_map_workspace_bytes(w, h, v))
    assert need == 32
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
    L.check(lib.mipt_sample_map_device(C.byref(opt), C.byref(bufs), C.c_void_p(d_work.data_ptr() + guard * 4), C.c_void_p(stream.cuda_stream)),
            "mipt_sample_map_device")
    stream.synchronize()
    c, wk = d_counts.cpu().numpy(), d_work.cpu().numpy()
    clean = (np.all(c[:guard] == 0x5a5a5a5a) and np.all(c[guard + n:] == 0x5a5a5a5a) and np.all(wk[:guard] == 0x3c3c3c3c) and
             np.all(wk[guard + need // 4:] == 0x3c3c3c3c) and all(torch.equal(a.view(torch.int32), before[k].view(torch.int32)) for k, a in t.items()))
    return c[guard:guard + n].view(np.uint32).reshape(variance.shape), bool(clean)


@pytest.mark.parametrize("buffers", ["variance", "hdr", "albedo"])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_model(rrt, shape, buffers):
    variance, hdr, albedo = _planes(shape, sum(shape))
    hdr = hdr if buffers != "variance" else None
    albedo = albedo if buffers == "albedo" else None
    for lo, hi, budget in ((1, 8, 2.0), (0, 16, 1.5), (1, 65535, 700.5)):
        want = SM.sample_map(variance, hdr, albedo, lo, hi, budget)
        got_h = _host(rrt, variance, hdr, albedo, lo, hi, budget)
        got_d, clean = _device(rrt, variance, hdr, albedo, lo, hi, budget)
        assert np.array_equal(got_h, want), (lo, hi, budget, int(np.count_nonzero(got_h != want)))
        assert np.array_equal(got_d, want) and clean
        assert int(want.sum(dtype=np.uint64)) <= SM.total(budget, want.size)
        assert int(got_d.sum(dtype=np.uint64)) <= SM.total(budget, want.size)


# ---- past the grid cap: 2048 blocks x 256 threads hold 524 288 pixels, every pixel beyond is a thread's second or later trip ---------
CAP = 2048 * 256
PAST_CAP = [(1, 513, 1023),      # 524 799 pixels: 511 threads take a second trip, the others do not
            (3, 601, 599)]       # 1 080 003 pixels: two whole trips and a ragged third
TRIPLES = ((1, 8, 2.0), (0, 16, 1.5), (1, 65535, 700.5))


@pytest.mark.parametrize("buffers", ["variance", "hdr", "albedo"])
@pytest.mark.parametrize("shape", PAST_CAP, ids=["x".join(map(str, s)) for s in PAST_CAP])
def test_kernels_equal_the_model_past_the_grid_cap(rrt, shape, buffers):
    """both kernels' stride loops: the sum takes in the pixels of the later trips, and every one of them gets its count"""
    assert CAP < int(np.prod(shape)) and (shape != PAST_CAP[0] or int(np.prod(shape)) < CAP + 2 * 256)
    variance, hdr, albedo = _planes(shape, sum(shape))
    hdr = hdr if buffers != "variance" else None
    albedo = albedo if buffers == "albedo" else None
    # special values and noisy pixels behind the first trip too (_planes scatters 40 over the whole plane, which may miss it)
    tail = variance.reshape(-1)[CAP:]
    tail[:8] = [np.nan, np.inf, -1.0, 1e-42, 0.0, 3e38, 0.25, 1.5]
    tail[-3:] = [0.75, np.nan, 2.0]
    for lo, hi, budget in TRIPLES:
        want = SM.sample_map(variance, hdr, albedo, lo, hi, budget)
        assert np.unique(want.reshape(-1)[CAP:]).size > 1                      # the later trips hold more than one answer
        got_h = _host(rrt, variance, hdr, albedo, lo, hi, budget)
        got_d, clean = _device(rrt, variance, hdr, albedo, lo, hi, budget)
        assert np.array_equal(got_h, want), (lo, hi, budget, int(np.count_nonzero(got_h != want)))
        assert np.array_equal(got_d, want) and clean, (lo, hi, budget, int(np.count_nonzero(got_d != want)))
        assert int(want.sum(dtype=np.uint64)) <= SM.total(budget, want.size)


def _saturated(shape, seed):
    """ordinary pixels (_planes) mixed with more than 300 000 whose variance lies between 1e7 and 1e9: q at the clamp of 16 777 215
    for a variance above 16 777 215 (sqrt(v) * 4096 >= 2^24), a little below it for the others"""
    variance = _planes(shape, seed)[0]
    rng = np.random.default_rng(seed + 1)
    flat = variance.reshape(-1)
    idx = rng.choice(flat.size, size=310000, replace=False)
    flat[idx] = rng.uniform(1e7, 1e9, idx.size).astype(F)
    flat[CAP + 5] = F(1e9)                                                   # one at the clamp in the second trip for certain
    return variance


def test_sum_past_2_to_32_past_the_grid_cap(rrt):
    """the 64-bit sum: more than 300 000 pixels at or near the clamp make S about 5e12, in a plane past the cap so that every lane's
    accumulator, the shuffles, the LDS step and the atomic all carry more than 32 bits"""
    shape = PAST_CAP[0]
    variance = _saturated(shape, 11)
    lo, hi, budget = 0, 65535, 700.5
    qi = SM.weights(variance)
    s = int(qi.sum(dtype=np.uint64))
    assert s > 2 ** 32 and int(np.count_nonzero(qi >= SM.QMAX - (1 << 22))) >= 300000        # conditions on the input
    assert int(np.count_nonzero(qi == SM.QMAX)) > 256 and int(np.count_nonzero((qi > 0) & (qi < SM.QMAX))) > 256
    x = qi.astype(np.float64) * (np.float64(SM.total(budget, qi.size) - lo * qi.size) / np.float64(s))
    assert (x >= 1.0).any() and (x < 1.0).any() and (x < hi - lo).all()          # r * qi is neither 0 nor >= span everywhere
    want = SM.sample_map(variance, None, None, lo, hi, budget)
    assert np.unique(want).size > 100                                        # counts differ between pixels
    got_h = _host(rrt, variance, None, None, lo, hi, budget)
    got_d, clean = _device(rrt, variance, None, None, lo, hi, budget)
    assert np.array_equal(got_h, want), int(np.count_nonzero(got_h != want))
    assert np.array_equal(got_d, want) and clean, int(np.count_nonzero(got_d != want))
    assert int(got_d.sum(dtype=np.uint64)) <= SM.total(budget, want.size)


def test_zero_sum_and_equal_clamps_past_the_grid_cap(rrt):
    """S == 0 gives uniform_extra on every trip; min == max gives the clamp on every trip whatever the weights are"""
    shape = PAST_CAP[0]
    zero = np.zeros(shape, dtype=F)
    zero.reshape(-1)[[0, 1, CAP - 1, CAP, CAP + 300, -1]] = [np.nan, -1.0, -np.inf, -0.0, np.nan, -2.5]
    for lo, hi, budget, value in ((1, 8, 3.75, 3), (0, 8, 0.5, 0), (2, 4, 4.0, 4)):
        got, clean = _device(rrt, zero, None, None, lo, hi, budget)
        assert np.all(got == value) and clean and np.array_equal(got, SM.sample_map(zero, None, None, lo, hi, budget))
        assert np.array_equal(_host(rrt, zero, None, None, lo, hi, budget), got)
    for variance in (np.full(shape, 0.5, dtype=F), _planes(shape, 13)[0], _saturated(shape, 17)):
        for entry in (_host, lambda *a: _device(*a)[0]):
            got = entry(rrt, variance, None, None, 4, 4, 4.0)
            assert np.all(got == 4) and np.array_equal(got, SM.sample_map(variance, None, None, 4, 4, 4.0))


def test_zero_sum_saturation_and_min_zero(rrt):
    shape = (2, 37, 200)
    zero = np.zeros(shape, dtype=F)
    zero[0, 0, :4] = [np.nan, -1.0, -np.inf, -0.0]
    for lo, hi, budget, value in ((1, 8, 3.75, 3), (0, 8, 0.5, 0), (2, 4, 4.0, 4)):
        got, clean = _device(rrt, zero, None, None, lo, hi, budget)
        assert np.all(got == value) and clean and np.array_equal(got, SM.sample_map(zero, None, None, lo, hi, budget))
        assert np.array_equal(_host(rrt, zero, None, None, lo, hi, budget), got)
    # every pixel saturates at max: equal weights and a budget of max
    flat = np.full(shape, 0.5, dtype=F)
    got, clean = _device(rrt, flat, None, None, 1, 6, 6.0)
    want = SM.sample_map(flat, None, None, 1, 6, 6.0)
    assert np.array_equal(got, want) and clean and int(got.sum()) <= SM.total(6.0, flat.size)
    got, clean = _device(rrt, flat, None, None, 4, 4, 4.0)  # min == max: a span of 0, every pixel at the clamp
    assert np.all(got == 4) and clean and np.array_equal(got, SM.sample_map(flat, None, None, 4, 4, 4.0))
    few = np.zeros(shape, dtype=F)
    few[:, ::9, ::50] = 0.3                                 # every noisy pixel saturates at max, the others stay at min
    got, clean = _device(rrt, few, None, None, 1, 7, 3.0)
    assert np.all(got[few > 0] == 7) and np.all(got[few == 0] == 1) and clean
    assert np.array_equal(got, SM.sample_map(few, None, None, 1, 7, 3.0))
    one = np.zeros(shape, dtype=F)
    one[1, 20, 100] = 1.0                                   # the clamp itself: one pixel would take the whole budget
    got, clean = _device(rrt, one, None, None, 0, 9, 2.0)
    assert got[1, 20, 100] == 9 and int(got.sum()) == 9 and clean
    assert np.array_equal(got, SM.sample_map(one, None, None, 0, 9, 2.0))


def test_renderer_mirror(rrt):
    import torch
    variance, hdr, albedo = _planes((2, 37, 200), 77)
    r = rrt.Renderer.new(rrt.RendererOptions(samples=8, max_ray_depth=2, output_image_dimensions=(200, 37), output_image_path="/dev/null"))
    want = SM.sample_map(variance, hdr, albedo, 1, 8, 2.0)
    assert np.array_equal(r.sample_map(variance, hdr, albedo, budget=2.0), want)
    got = r.sample_map(torch.from_numpy(variance).cuda(), torch.from_numpy(hdr).cuda(), torch.from_numpy(albedo).cuda(), budget=2.0)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy().view(np.uint32), want)
    assert np.all(r.sample_map(variance) == 1)             # budget defaults to min_samples
    with pytest.raises(ValueError):
        r.sample_map(variance, None, albedo)
