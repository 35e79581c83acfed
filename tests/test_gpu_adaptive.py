"""-m gpu: mipt_render_adaptive / mipt_render_adaptive_device -- a batch render with one sample count per pixel.  The contract: a
pixel traced with n samples holds, bit for bit (u32 patterns, NaN matched to NaN), what mipt_render writes for its camera with
samples = n; a pixel with 0 is not traced, holds +0 and is not counted.  The reference is mipt_render at every distinct n, assembled
per pixel -- existing code, held to the oracle elsewhere -- and, once, the oracle itself."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

from test_gpu_batch import CONFIGS as BATCH_CONFIGS
from test_gpu_batch import COUNTERS, LT, _poses, _same, _scene, _table

pytestmark = pytest.mark.gpu

CONFIGS = dict(BATCH_CONFIGS, wgpu_reference=(1, 0, 0.0))       # shading x traversal: the batch file's three and the fourth corner
W, H, N_VIEWS, DEPTH, CAP = 24, 20, 2, 4, 5                     # three tile columns, a ragged last tile row
LEVELS = (1, 2, 3, 5)                                           # the distinct n of the plane below
POISON = 0x7fc0dead                                             # a NaN pattern no render produces


def _counts():
    """seeded random from {0, 1, 2, 3, 5, 9} (9 exercises the clamp at CAP), one full 8x8 tile all zero, pixel (0,0) forced to 5 and
    the last pixel to 0"""
    rng = np.random.default_rng(2026)
    c = rng.choice(np.array([0, 1, 2, 3, 5, 9], dtype=np.uint32), size=(N_VIEWS, H, W))
    c[1, 8:16, 8:16] = 0
    c[0, 0, 0] = 5
    c[-1, -1, -1] = 0
    return np.ascontiguousarray(c, dtype=np.uint32)


def _options(rrt, config, seed_mode, samples=CAP, flags=0, w=W, h=H, depth=DEPTH):
    shading, trav, margin = CONFIGS[config]
    return rrt.make_options(w, h, samples, depth, seed_mode=seed_mode, traversal=trav, flags=flags, cull_margin=margin, shading=shading,
                            sample_begin=7 if seed_mode == 1 else 0)


@functools.lru_cache(maxsize=None)
def _reference(config, seed_mode, flags=0):
    """{n: (hdr [V,H,W,3], rgba8 [V,H,W,4] | None)} from mipt_render per view at samples = n; computed once per configuration"""
    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc, cam = _scene("cornell")
    hnd = sc.upload(0)
    cams = _poses(rrt, cam, N_VIEWS, 0.8, 91)
    out = {}
    for n in LEVELS:
        o = _options(rrt, config, seed_mode, samples=n, flags=flags)
        hdr = np.zeros((N_VIEWS, H, W, 3), dtype=np.float32)
        px = None if flags & L.FLAG_SUM else np.zeros((N_VIEWS, H, W, 4), dtype=np.uint8)
        for v, c in enumerate(cams):
            L.check(lib.mipt_render(hnd, L.ptr(c.uniform), C.byref(o), L.ptr(hdr[v]), L.ptr(px[v]) if px is not None else None, None), "mipt_render")
        for a in (hdr, px):
            if a is not None:
                a.setflags(write=False)
        out[n] = (hdr, px)
    return out


def _assemble(ref, counts, zero_hdr=None):
    """the frame the contract asks for: per pixel the reference at min(count, CAP); a zero count gives +0 (or zero_hdr's pixel)"""
    n = np.minimum(counts, CAP)
    hdr = np.zeros(counts.shape + (3,), dtype=np.float32) if zero_hdr is None else zero_hdr.copy()
    px = np.zeros(counts.shape + (4,), dtype=np.uint8)
    px[..., 3] = 255                                            # the epilogue over a zero pixel: black, opaque
    for k in LEVELS:
        hdr[n == k] = ref[k][0][n == k]
        if ref[k][1] is not None:
            px[n == k] = ref[k][1][n == k]
    return hdr, px


def _cams(rrt):
    sc, cam = _scene("cornell")
    return sc, _poses(rrt, cam, N_VIEWS, 0.8, 91)


@pytest.mark.parametrize("seed_mode", [0, 1])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_adaptive_pixels_equal_single_renders(rrt, config, seed_mode):
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc, cams = _cams(rrt)
    hnd = sc.upload(0)
    table = _table(cams)
    counts = _counts()
    want_hdr, want_px = _assemble(_reference(config, seed_mode), counts)
    o = _options(rrt, config, seed_mode)
    # host entry
    hdr = np.full((N_VIEWS, H, W, 3), np.nan, dtype=np.float32)
    px = np.full((N_VIEWS, H, W, 4), 7, dtype=np.uint8)
    st = L.MiptStats()
    L.check(lib.mipt_render_adaptive(hnd, L.ptr(table), N_VIEWS, C.byref(o), L.ptr(counts), L.ptr(hdr), L.ptr(px), C.byref(st)), "mipt_render_adaptive")
    assert _same(hdr, want_hdr) and np.array_equal(px, want_px)
    assert np.all(hdr.view(np.uint32)[counts == 0] == 0)      # +0, not -0
    assert st.pixels == int(np.count_nonzero(counts)) and st.kernel_ms > 0
    # device entry on a non-null stream, the outputs pre-filled with a poison pattern: an unwritten pixel shows
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    d_counts = torch.from_numpy(counts.view(np.int32)).to(dev)
    d_hdr = torch.full((N_VIEWS, H, W, 3), POISON, dtype=torch.int32, device=dev)
    d_px = torch.full((N_VIEWS, H, W, 4), 0x5a, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    st2 = L.MiptStats()
    L.check(lib.mipt_render_adaptive_device(hnd, L.ptr(table), N_VIEWS, C.byref(o), d_counts.data_ptr(), d_hdr.data_ptr(), d_px.data_ptr(),
                                            C.c_void_p(stream.cuda_stream), C.byref(st2)), "mipt_render_adaptive_device")
    stream.synchronize()
    assert _same(d_hdr.cpu().numpy().view(np.float32), want_hdr) and np.array_equal(d_px.cpu().numpy(), want_px)
    assert st2.pixels == st.pixels


def test_adaptive_pixels_equal_the_oracle(rrt, orc):
    """the same case against the CPU oracle directly: pixel-stream seeds, culled at MIPT_CULL_MARGIN_SAFE, one oracle frame per n"""
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc, cams = _cams(rrt)
    hnd = sc.upload(0)
    table = _table(cams)
    counts = _counts()
    o = _options(rrt, "cpu_culled", 0)
    hdr = np.zeros((N_VIEWS, H, W, 3), dtype=np.float32)
    L.check(lib.mipt_render_adaptive(hnd, L.ptr(table), N_VIEWS, C.byref(o), L.ptr(counts), L.ptr(hdr), None, None), "mipt_render_adaptive")
    n = np.minimum(counts, CAP)
    for k in LEVELS:
        for v, c in enumerate(cams):
            ref, _, _ = orc.render(sc.tris, sc.bvh_nodes, sc.materials_array(), sc.textures, c.uniform, W, H, k, DEPTH, cull=1,
                                   cull_margin=L.CULL_MARGIN_SAFE, want_rgba8=False)
            assert _same(hdr[v][n[v] == k], ref[n[v] == k]), (k, v)
    assert np.all(hdr[n == 0] == 0)


def test_sum_accum_adds_every_pixel_exactly_once(rrt):
    """SUM | ACCUM on a pre-filled device buffer: prefill + the SUM render at the pixel's n, and the prefill itself where n == 0; a
    pixel traced twice, or a zero pixel written, fails here"""
    import torch
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc, cams = _cams(rrt)
    hnd = sc.upload(0)
    table = _table(cams)
    counts = _counts()
    ref = _reference("cpu_culled", 1, L.FLAG_SUM)
    prefill = np.random.default_rng(5).random((N_VIEWS, H, W, 3)).astype(np.float32)
    sums, _ = _assemble(ref, counts)
    want = (prefill + sums).astype(np.float32)                  # one rounded f32 add per channel, as the kernel's
    want[np.minimum(counts, CAP) == 0] = prefill[counts == 0]
    d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    d_hdr = torch.from_numpy(prefill).cuda()
    o = _options(rrt, "cpu_culled", 1, flags=L.FLAG_SUM | L.FLAG_ACCUM)
    torch.cuda.synchronize()
    L.check(lib.mipt_render_adaptive_device(hnd, L.ptr(table), N_VIEWS, C.byref(o), d_counts.data_ptr(), d_hdr.data_ptr(), None, None, None),
            "mipt_render_adaptive_device")
    assert _same(d_hdr.cpu().numpy(), want)
    # SUM alone: the undivided sums, zeros elsewhere
    o2 = _options(rrt, "cpu_culled", 1, flags=L.FLAG_SUM)
    hdr = np.full((N_VIEWS, H, W, 3), np.nan, dtype=np.float32)
    L.check(lib.mipt_render_adaptive(hnd, L.ptr(table), N_VIEWS, C.byref(o2), L.ptr(counts), L.ptr(hdr), None, None), "mipt_render_adaptive")
    assert _same(hdr, sums)


def test_counters_are_the_sums_over_the_traced_paths(rrt):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc, cams = _cams(rrt)
    hnd = sc.upload(0)
    table = _table(cams)
    counts = np.zeros((N_VIEWS, H, W), dtype=np.uint32)
    counts[0], counts[1] = 2, 3
    singles = []
    for v, n in enumerate((2, 3)):
        o = _options(rrt, "cpu_culled", 0, samples=n, flags=L.FLAG_COUNT)
        st = L.MiptStats()
        buf = np.zeros((H, W, 3), dtype=np.float32)
        L.check(lib.mipt_render(hnd, L.ptr(cams[v].uniform), C.byref(o), L.ptr(buf), None, C.byref(st)), "mipt_render")
        singles.append(st.as_dict())
    o = _options(rrt, "cpu_culled", 0, flags=L.FLAG_COUNT)
    st = L.MiptStats()
    hdr = np.zeros((N_VIEWS, H, W, 3), dtype=np.float32)
    L.check(lib.mipt_render_adaptive(hnd, L.ptr(table), N_VIEWS, C.byref(o), L.ptr(counts), L.ptr(hdr), None, C.byref(st)), "mipt_render_adaptive")
    got = st.as_dict()
    for k in COUNTERS:
        assert got[k] == singles[0][k] + singles[1][k], k
    assert got["max_stack"] == max(s["max_stack"] for s in singles)
    holes = _counts()
    L.check(lib.mipt_render_adaptive(hnd, L.ptr(table), N_VIEWS, C.byref(o), L.ptr(holes), L.ptr(hdr), None, C.byref(st)), "mipt_render_adaptive")
    assert st.pixels == int(np.count_nonzero(holes)) < holes.size


def test_more_pixels_than_resident_lanes(rrt):
    """640x544 = 348 160 pixels against 327 680 resident lanes at 5 blocks per CU: lanes refill, the only case where the order in
    which pixels are handed out matters"""
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc, cam = _scene("cornell")
    hnd = sc.upload(0)
    cams = _poses(rrt, cam, 2, 0.8, 93)[:1]
    table = _table(cams)
    w, h = 640, 544
    counts = np.random.default_rng(11).integers(0, 3, size=(1, h, w)).astype(np.uint32)
    counts[0, :, 300:364] = 2
    o = rrt.make_options(w, h, 2, 2, seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED)
    hdr = np.zeros((1, h, w, 3), dtype=np.float32)
    st = L.MiptStats()
    L.check(lib.mipt_render_adaptive(hnd, L.ptr(table), 1, C.byref(o), L.ptr(counts), L.ptr(hdr), None, C.byref(st)), "mipt_render_adaptive")
    want = np.zeros_like(hdr)
    for n in (1, 2):
        on = rrt.make_options(w, h, n, 2, seed_mode=L.SEED_PER_SAMPLE, traversal=L.TRAVERSAL_CULLED)
        ref = np.zeros((h, w, 3), dtype=np.float32)
        L.check(lib.mipt_render(hnd, L.ptr(cams[0].uniform), C.byref(on), L.ptr(ref), None, None), "mipt_render")
        want[0][counts[0] == n] = ref[counts[0] == n]
    assert _same(hdr, want)
    assert st.pixels == int(np.count_nonzero(counts))


# ---- launches larger than the lanes in flight, with lanes that move from view to view ------------------------------------------------
# The test above passes the lanes in flight by 6 % with one view.  These cross the two thresholds of tests/tools/launch_thresholds.py
# (MID: lanes refill, leaf_period 1; FULL: leaf_period 4, a quarter of the work in flight, a ragged tail) with hundreds to thousands
# of views of the file's W x H frame, three distinct cameras cycled with stride 2 from camera 1, so that a lane's next pixel has another
# view, another camera and another row of the count plane.
BIG_CAMERAS, BIG_LEVELS = 3, (1, 2, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def _big_reference(config, seed_mode):
    """mipt_render of each of the three cameras at samples = 1 ... CAP -> (hdr [3, CAP + 1, H, W, 3] with zeros at level 0, rgba8
    [3, CAP + 1, H, W, 4] with opaque black at level 0, counters {(camera, level): dict} of the counting twin, whose frames are checked
    to be the product build's); computed once per configuration and left unchanged"""
    import rust_ray_tracing_amd as rrt
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc, cam = _scene("cornell")
    hnd = sc.upload(0)
    cams = _poses(rrt, cam, BIG_CAMERAS + 1, 0.8, 91)[:BIG_CAMERAS]         # the scene's own and two seeded poses, all distinct
    hdr = np.zeros((BIG_CAMERAS, CAP + 1, H, W, 3), dtype=np.float32)
    px = np.zeros((BIG_CAMERAS, CAP + 1, H, W, 4), dtype=np.uint8)
    px[:, 0, ..., 3] = 255
    stats = {}
    for c, camera in enumerate(cams):
        for n in BIG_LEVELS:
            o = _options(rrt, config, seed_mode, samples=n)
            L.check(lib.mipt_render(hnd, L.ptr(camera.uniform), C.byref(o), L.ptr(hdr[c, n]), L.ptr(px[c, n]), None), "mipt_render")
            oc = _options(rrt, config, seed_mode, samples=n, flags=L.FLAG_COUNT)
            twin, st = np.zeros((H, W, 3), dtype=np.float32), L.MiptStats()
            L.check(lib.mipt_render(hnd, L.ptr(camera.uniform), C.byref(oc), L.ptr(twin), None, C.byref(st)), "mipt_render")
            assert _same(twin, hdr[c, n]), (c, n)
            stats[c, n] = st.as_dict()
    assert not _same(hdr[0, 1], hdr[1, 1]) and not _same(hdr[1, 1], hdr[2, 1]) and not _same(hdr[0, 1], hdr[2, 1])
    hdr.setflags(write=False); px.setflags(write=False)
    return cams, hdr, px, stats


def _big_counts(n_views, seed):
    """[n_views, H, W] seeded from {0, 1, 2, 3, 4, 5, 9} (9 is clamped to CAP); in a seeded fifth of all (view, tile) pairs the whole
    8x8 tile is zero, in another fifth zero pixels and full ones alternate: fetches that skip fall in every part of the queue"""
    rng = np.random.default_rng(seed)
    c = rng.choice(np.array([0, 1, 2, 3, 4, 5, 9], dtype=np.uint32), size=(n_views, H, W))
    ty, tx = (H + 7) // 8, (W + 7) // 8
    kind = rng.integers(0, 5, size=(n_views, ty, tx))
    kind_px = np.repeat(np.repeat(kind, 8, axis=1), 8, axis=2)[:, :H, :W]
    yy, xx = np.mgrid[0:H, 0:W]
    checker = np.where((yy + xx) % 2 == 0, 0, 9).astype(np.uint32)
    c = np.where(kind_px == 0, 0, np.where(kind_px == 1, checker[None], c))
    c[0, 0, 0], c[-1, -1, -1] = 5, 0
    return np.ascontiguousarray(c, dtype=np.uint32)


def _run_big_adaptive(lib, hnd, table, n, o, counts, device, prefill_bits):
    """one call; the frame starts as `prefill_bits` in every word and ends in canary words -> (hdr, rgba8, stats dict, seconds)"""
    from rust_ray_tracing_amd import _lib as L
    st = L.MiptStats()
    n_f, n_b, tail = n * H * W * 3, n * H * W * 4, 64
    if device:
        import torch
        d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
        d_hdr = torch.full((n_f + tail,), prefill_bits, dtype=torch.int32, device="cuda")
        d_hdr[n_f:] = 0x4640E400
        d_px = torch.full((n_b + tail,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.mipt_render_adaptive_device(hnd, L.ptr(table), n, C.byref(o), d_counts.data_ptr(), d_hdr.data_ptr(), d_px.data_ptr(), None, C.byref(st))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        hdr, px = d_hdr.cpu().numpy().view(np.uint32), d_px.cpu().numpy()
    else:
        hdr = np.full(n_f + tail, prefill_bits, dtype=np.uint32)
        hdr[n_f:] = 0x4640E400
        px = np.full(n_b + tail, 0x5A, dtype=np.uint8)
        t0 = time.perf_counter()
        rc = lib.mipt_render_adaptive(hnd, L.ptr(table), n, C.byref(o), L.ptr(counts), L.ptr(hdr), L.ptr(px), C.byref(st))
        dt = time.perf_counter() - t0
    assert rc == 0, lib.mipt_last_error()
    assert np.all(hdr[n_f:] == 0x4640E400) and np.all(px[n_b:] == 0x5A), "written behind the last view"
    return hdr[:n_f].view(np.float32).reshape(n, H, W, 3), px[:n_b].reshape(n, H, W, 4), st.as_dict(), dt


@pytest.mark.parametrize("config,seed_mode", [("cpu_culled", 1), ("cpu_reference", 0)])
@pytest.mark.parametrize("size", ["mid", "full"])
def test_more_views_than_resident_lanes(rrt, size, config, seed_mode):
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    t0 = time.perf_counter()
    cams, ref_hdr, ref_px, ref_st = _big_reference(config, seed_mode)
    t_singles = time.perf_counter() - t0
    sc, _ = _scene("cornell")
    hnd = sc.upload(0)
    n_cu = LT.device_n_cu()
    n = LT.views_for(LT.mid(n_cu) if size == "mid" else LT.full(n_cu), W, H)
    (LT.check_mid if size == "mid" else LT.check_full)(n_cu, n * LT.view_work(W, H))
    cam_of_view = (2 * np.arange(n) + 1) % BIG_CAMERAS
    table = np.ascontiguousarray(_table(cams)[cam_of_view])
    yy, xx = np.mgrid[0:H, 0:W]
    t_call = t_cmp = 0.0

    def check(counts, flags, device, what):
        nonlocal t_call, t_cmp
        o = _options(rrt, config, seed_mode, flags=flags)
        hdr, px, st, dt = _run_big_adaptive(lib, hnd, table, n, o, counts, device, POISON)
        t_call += dt
        t0 = time.perf_counter()
        level = np.minimum(counts, CAP)
        want_hdr = ref_hdr[cam_of_view[:, None, None], level, yy[None], xx[None]]
        want_px = ref_px[cam_of_view[:, None, None], level, yy[None], xx[None]]
        g, wn = hdr.view(np.uint32), want_hdr.view(np.uint32)
        same = ((g == wn) | (np.isnan(hdr) & np.isnan(want_hdr))).all(axis=-1)
        bad = np.argwhere(~same)
        assert len(bad) == 0, (what, len(bad), [(tuple(int(x) for x in b), int(counts[tuple(b)])) for b in bad[:6]])   # (view, y, x), its count
        assert np.all(g[counts == 0] == 0)                                 # the prefill's +0: never traced, never written
        assert np.array_equal(px, want_px), what
        assert st["pixels"] == int(np.count_nonzero(counts)) and st["stack_overflows"] == 0 and st["kernel_ms"] > 0, (what, st["pixels"])
        t_cmp += time.perf_counter() - t0
        return st

    # a seeded plane, the product build through the host entry and the counting twin through the device entry
    counts = _big_counts(n, 2027)
    assert 0.2 < np.count_nonzero(counts) / counts.size < 0.9 and (counts.reshape(n, -1).max(axis=1) == 0).sum() < n // 8
    st = check(counts, 0, False, "seeded plane, product build, host entry")
    assert st["rays"] == 0 and st["tri_tests"] == 0
    check(counts, L.FLAG_COUNT, True, "seeded plane, counting twin, device entry")
    # one level per view, 0 and the clamped 9 among them: the launch's counters are the sums of the single renders' counters
    level_of_view = np.array([0, 3, 9, 1, 5, 2, 4], dtype=np.uint32)[(5 * np.arange(n) + 2) % 7]
    flat = np.ascontiguousarray(np.broadcast_to(level_of_view[:, None, None], (n, H, W)))
    for device in (False, True):
        st = check(flat, L.FLAG_COUNT, device, f"one level per view, counting twin, device={device}")
        traced = [(int(cam_of_view[v]), int(min(level_of_view[v], CAP))) for v in range(n) if level_of_view[v]]
        for k in ("rays", "inner_steps", "tri_tests", "hits", "texel_fetches"):
            assert st[k] == sum(ref_st[key][k] for key in traced), (k, device)
        assert st["max_stack"] == max(ref_st[key]["max_stack"] for key in set(traced))
    print(f"adaptive-{size}-{config}: {n} views of {W}x{H} = {n * LT.view_work(W, H)} work items on {n_cu} CUs: singles {t_singles:.2f} s, "
          f"four adaptive calls {t_call:.2f} s, compare {t_cmp:.2f} s")


def test_all_zero_plane_and_the_shared_workspace(rrt):
    """an all-zero plane is MIPT_OK, a zero frame and pixels == 0; and the scene renders with mipt_render bit-identically before and
    after adaptive calls of other grid sizes: the spill workspace is still sized and shared in one place"""
    from rust_ray_tracing_amd import _lib as L
    lib = rrt.load()
    sc, cams = _cams(rrt)
    hnd = sc.upload(0)
    table = _table(cams)
    o1 = rrt.make_options(160, 90, 2, 6, traversal=L.TRAVERSAL_CULLED, flags=L.FLAG_COUNT)
    before, st_b = np.zeros((90, 160, 3), dtype=np.float32), L.MiptStats()
    L.check(lib.mipt_render(hnd, L.ptr(cams[0].uniform), C.byref(o1), L.ptr(before), None, C.byref(st_b)), "mipt_render")
    o = _options(rrt, "cpu_culled", 0)
    zeros = np.zeros((N_VIEWS, H, W), dtype=np.uint32)
    hdr = np.full((N_VIEWS, H, W, 3), np.nan, dtype=np.float32)
    px = np.full((N_VIEWS, H, W, 4), 9, dtype=np.uint8)
    st = L.MiptStats()
    assert lib.mipt_render_adaptive(hnd, L.ptr(table), N_VIEWS, C.byref(o), L.ptr(zeros), L.ptr(hdr), L.ptr(px), C.byref(st)) == L.OK
    assert np.all(hdr.view(np.uint32) == 0) and st.pixels == 0 and st.rays == 0
    assert np.all(px[..., :3] == 0) and np.all(px[..., 3] == 255)
    big = np.full((1, 544, 640), 1, dtype=np.uint32)           # a larger grid than any launch before it on this handle
    ob = rrt.make_options(640, 544, 1, 2, traversal=L.TRAVERSAL_CULLED)
    out = np.zeros((1, 544, 640, 3), dtype=np.float32)
    L.check(lib.mipt_render_adaptive(hnd, L.ptr(table), 1, C.byref(ob), L.ptr(big), L.ptr(out), None, None), "mipt_render_adaptive")
    after, st_a = np.zeros_like(before), L.MiptStats()
    L.check(lib.mipt_render(hnd, L.ptr(cams[0].uniform), C.byref(o1), L.ptr(after), None, C.byref(st_a)), "mipt_render")
    assert _same(after, before)
    for k in COUNTERS + ("max_stack",):
        assert getattr(st_a, k) == getattr(st_b, k), k


def test_renderer_mirror(rrt):
    """Renderer.render_adaptive: numpy counts through the host entry, an int32 tensor through the device entry, the same frame"""
    import torch
    sc, cams = _cams(rrt)
    r = rrt.Renderer.new(rrt.RendererOptions(samples=CAP, max_ray_depth=DEPTH, output_image_dimensions=(W, H), output_image_path="/dev/null",
                                             seed_mode=1, traversal=1))
    counts = _counts()
    hdr, px, st = r.render_adaptive(sc, counts, cams, sample_begin=7, want_rgba8=True)
    want_hdr, want_px = _assemble(_reference("cpu_culled", 1), counts)
    assert _same(hdr, want_hdr) and np.array_equal(px, want_px) and st["pixels"] == int(np.count_nonzero(counts))
    t_hdr, t_px, st2 = r.render_adaptive(sc, torch.from_numpy(counts.view(np.int32)).cuda(), cams, sample_begin=7, want_rgba8=True)
    assert _same(t_hdr.cpu().numpy(), want_hdr) and np.array_equal(t_px.cpu().numpy(), want_px) and st2["pixels"] == st["pixels"]
    with pytest.raises(ValueError):
        r.render_adaptive(sc, counts[:, :-1], cams)
