"""-m gpu: the hot pixels are pure scheduling.  A plain single-view launch measures the rays of every pixel of its local 8x8 tiles (slot =
local tile * 64 + pixel of the tile; the tile costs of tests/test_gpu_tile_order.py are their sums); the next launch with the same key and
camera on the same scene handle hands out the H most expensive slots first, one by one, and skips them in the pass over the ordered tiles
behind them.  H = min(2 x the resident lanes of the measuring launch, a quarter of the local slots): the quarter at every small size
here.  Whatever the list, a frame's bits are a fresh handle's and every pixel is written once: 72x40 is 45 tiles; 70x37 has ragged edges
(slots that are no pixel and cost 0); 256x144 has more slots than one block of the selection kernels owns (8 192), so the counts of
several blocks are scanned; 2560x1440 is the one size at which the lanes decide H, not the quarter -- and there H differs between the
culled and the un-culled traversal (5 and 4 blocks per CU), which the key does not tell apart.  Costs, list, H and "ran with the list"
are read from the handle through libmipt_diag.so; the selection kernels are also run on made-up costs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPP, DEPTH = 4, 8


def _scene(rrt, kind):
    from rust_ray_tracing_amd import synth
    tris, mats, texs, cam = synth.cornell_box() if kind == "cornell" else synth.helmet_scene(n_target=2000, tex_size=64)
    sc = rrt.Scene.from_arrays(tris, mats, texs)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    return sc, cam


def _render(rrt, sc, w, h, n_pixels=None, traversal=None, **kw):
    """One mipt_render on the scene's current handle into a buffer full of NaN: (frame as u32 bits, stats)."""
    from rust_ray_tracing_amd import _lib as L
    buf = np.full((n_pixels if n_pixels else w * h) * 3, np.nan, dtype=np.float32)
    o = rrt.make_options(w, h, SPP, DEPTH, traversal=L.TRAVERSAL_CULLED if traversal is None else traversal, **kw)
    st = L.MiptStats()
    L.check(rrt.load().mipt_render(sc.upload(0), L.ptr(sc.camera.uniform), C.byref(o), L.ptr(buf), None, C.byref(st)), "mipt_render")
    return buf.view(np.uint32).copy(), st.as_dict()


def _fresh(rrt, sc, w, h, **kw):
    sc.release()                                     # the next upload() makes a new handle: no state
    return _render(rrt, sc, w, h, **kw)


def _host_hot(cost, n_hot, samples=SPP):
    """The list the selection must give: bucket min(1023, floor(cost * 16 / samples)) descending, slot index ascending, cut at n_hot."""
    scale = np.float32(16.0) / np.float32(samples)
    b = np.minimum(np.floor(cost.astype(np.float32) * scale), np.float32(1023.0)).astype(np.int64)
    return np.argsort(1023 - b, kind="stable")[:n_hot].astype(np.uint32)


def _hot_state(rrt, sc):
    """(slots, H, entries the last launch took from the list before it, pixel cost, hot list) of the scene's current handle."""
    diag = rrt.load_diag()
    info = (C.c_uint32 * 3)()
    assert diag.mipt_diag_scene_hot_pixels(sc.upload(0), None, 0, None, 0, C.byref(info)) == 0, diag.mipt_diag_last_error()
    n, h = int(info[0]), int(info[1])
    cost, hot = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(h, 1), dtype=np.uint32)
    assert diag.mipt_diag_scene_hot_pixels(sc.upload(0), cost.ctypes.data, n, hot.ctypes.data, h, C.byref(info)) == 0, diag.mipt_diag_last_error()
    return n, h, int(info[2]), cost[:n], hot[:h]


def _tile_state(rrt, sc):
    """(valid, used, tile cost) through the tile order's hook."""
    diag = rrt.load_diag()
    info = (C.c_uint32 * 3)()
    assert diag.mipt_diag_scene_tile_order(sc.upload(0), None, None, 0, C.byref(info)) == 0, diag.mipt_diag_last_error()
    n = int(info[0])
    cost, order = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
    assert diag.mipt_diag_scene_tile_order(sc.upload(0), cost.ctypes.data, order.ctypes.data, n, C.byref(info)) == 0, diag.mipt_diag_last_error()
    return bool(info[1]), bool(info[2]), cost[:n]


@pytest.mark.parametrize("w,h", [(72, 40), (70, 37), (256, 144)])
@pytest.mark.parametrize("kind", ["cornell", "helmet"])
def test_hot_frames_equal_a_fresh_handles(rrt, kind, w, h):
    from rust_ray_tracing_amd import _lib as L
    sc, _ = _scene(rrt, kind)
    n_tiles = ((w + 7) // 8) * ((h + 7) // 8)
    _, s_count = _fresh(rrt, sc, w, h, flags=L.FLAG_COUNT)
    f1, s1 = _fresh(rrt, sc, w, h)                   # plain order, measures
    n, n_hot, used, pc1, hot1 = _hot_state(rrt, sc)
    valid, _, tc1 = _tile_state(rrt, sc)
    assert valid and n == n_tiles * 64 and n_hot == n // 4 and used == 0
    assert int(pc1.sum(dtype=np.uint64)) == s_count["rays"] and np.array_equal(pc1.reshape(n_tiles, 64).sum(axis=1, dtype=np.uint32), tc1)
    # a slot costs something exactly when it is a pixel of the image: at least one ray per path
    gt = np.arange(n_tiles)
    px = ((gt % ((w + 7) // 8)) * 8)[:, None] + (np.arange(64) & 7)[None, :]
    py = ((gt // ((w + 7) // 8)) * 8)[:, None] + (np.arange(64) >> 3)[None, :]
    inside = ((px < w) & (py < h)).reshape(-1)
    assert np.array_equal(pc1 >= SPP, inside) and np.array_equal(pc1 == 0, ~inside)
    assert np.array_equal(hot1, _host_hot(pc1, n_hot)) and len(np.unique(hot1)) == n_hot
    f2, s2 = _render(rrt, sc, w, h)                  # hot pixels of frame 1 first
    _, n_hot2, used2, pc2, hot2 = _hot_state(rrt, sc)
    assert used2 == n_hot and _tile_state(rrt, sc)[1]
    assert n_hot2 == n_hot and np.array_equal(pc2, pc1) and np.array_equal(hot2, hot1)   # the same frame costs the same
    f3, s3 = _render(rrt, sc, w, h)
    for f, s in ((f1, s1), (f2, s2), (f3, s3)):
        assert s["pixels"] == w * h and not np.isnan(f.view(np.float32)).any()
    assert np.array_equal(f2, f1) and np.array_equal(f3, f1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 40_000])
def test_selection_kernels_equal_host_selection(rrt, n):
    """One slot, partial groups of 64, several blocks of 8 192 slots; random costs, all costs equal (the cut falls inside the one bucket:
    the lowest slot indices win), a few heavy slots among empty ones, costs beyond the last bucket, and costs whose cut bucket holds
    several times the places left, spread over the whole range of slots; H = 1, a quarter, one short of everything, everything."""
    diag = rrt.load_diag()
    rng = np.random.default_rng(n)
    top = SPP * 70                                       # rays per path up to 70: buckets up to 1 023 and the clamp above it
    straddle = np.where(rng.random(n) < 0.1, SPP * 40, np.where(rng.random(n) < 0.6, SPP * 9, rng.integers(0, SPP * 9, n)))
    cases = [rng.integers(0, top, n), np.full(n, 777), np.where(rng.random(n) < 0.05, rng.integers(0, top, n), 0),
             rng.integers(top - 20, 2 ** 31, n), straddle]
    for k, c in enumerate(cases):
        cost = c.astype(np.uint32)
        for n_hot in sorted({1, max(1, n // 4), max(1, n - 1), n}):
            hot = np.zeros(n_hot, dtype=np.uint32)
            bits = np.zeros((n + 63) // 64 * 2, dtype=np.uint32)
            assert diag.mipt_debug_hot_select(cost.ctypes.data, n, SPP, n_hot, hot.ctypes.data, bits.ctypes.data) == 0, diag.mipt_diag_last_error()
            want = _host_hot(cost, n_hot)
            assert np.array_equal(hot, want), (n, k, n_hot)
            flags = np.zeros(len(bits) * 32, dtype=bool)
            flags[want] = True
            assert np.array_equal(np.unpackbits(bits.view(np.uint8), bitorder="little").astype(bool), flags), (n, k, n_hot)
    assert diag.mipt_debug_hot_select(cost.ctypes.data, n, SPP, n + 1, hot.ctypes.data, bits.ctypes.data) == -1
    assert diag.mipt_debug_hot_select(cost.ctypes.data, n, SPP, 0, hot.ctypes.data, bits.ctypes.data) == -1


def test_one_tile_and_a_rank_without_tiles(rrt):
    """8x8 is one tile: H is capped at 16 of its 64 slots; rank 1 of 2 owns no tile, renders nothing and leaves rank 0's state alone."""
    from rust_ray_tracing_amd import _lib as L
    sc, _ = _scene(rrt, "cornell")
    n = int(rrt.load().mipt_packed_pixels(8, 8, 2))
    kw = dict(n_pixels=n, flags=L.FLAG_PACKED, tile_world=2)
    f0, s0 = _fresh(rrt, sc, 8, 8, tile_rank=0, **kw)
    slots, n_hot, used, pc, hot = _hot_state(rrt, sc)
    assert (slots, n_hot, used) == (64, 16, 0) and np.array_equal(hot, _host_hot(pc, 16))
    _, s1 = _render(rrt, sc, 8, 8, tile_rank=1, **kw)
    assert s0["pixels"] == 64 and s1["pixels"] == 0
    slots_b, n_hot_b, used_b, pc_b, hot_b = _hot_state(rrt, sc)
    assert (slots_b, n_hot_b, used_b) == (64, 16, 0) and np.array_equal(pc_b, pc) and np.array_equal(hot_b, hot)
    f0b, s0b = _render(rrt, sc, 8, 8, tile_rank=0, **kw)
    assert np.array_equal(f0b[:192], f0[:192]) and not np.isnan(f0b[:192].view(np.float32)).any() and s0b["pixels"] == 64 and _hot_state(rrt, sc)[2] == 16


def test_packed_two_rank_shard(rrt):
    from rust_ray_tracing_amd import _lib as L
    sc, _ = _scene(rrt, "helmet")
    w, h = 72, 40
    n = int(rrt.load().mipt_packed_pixels(w, h, 2))
    own = lambda rank: ((45 + 1 - rank) // 2) * 64 * 3            # words of the rank's own tiles: 23 and 22 of the 45 (the rest is not written)
    for rank in (0, 1):
        kw = dict(n_pixels=n, flags=L.FLAG_PACKED, tile_rank=rank, tile_world=2)
        ref, sr = _fresh(rrt, sc, w, h, **kw)
        again, sa = _render(rrt, sc, w, h, **kw)     # with the hot list
        slots, n_hot, used, _, _ = _hot_state(rrt, sc)
        assert slots == own(rank) // 3 and used == n_hot == slots // 4
        assert sr["pixels"] == sa["pixels"] == own(rank) // 3 and np.array_equal(again[:own(rank)], ref[:own(rank)])
        assert not np.isnan(again[:own(rank)].view(np.float32)).any()
    # both ranks in turn on one handle: every change of rank is a change of key
    sc.release()
    for i, rank in enumerate((0, 0, 1, 1, 0)):
        kw = dict(n_pixels=n, flags=L.FLAG_PACKED, tile_rank=rank, tile_world=2)
        f, _ = _render(rrt, sc, w, h, **kw)
        sc2, _ = _scene(rrt, "helmet")
        ref, _ = _render(rrt, sc2, w, h, **kw)
        sc2.release()
        assert np.array_equal(f[:own(rank)], ref[:own(rank)]), rank
        slots, n_hot, used, pc, hot = _hot_state(rrt, sc)
        assert used == (n_hot if i in (1, 3) else 0), i             # with the list exactly when the rank is the launch before's
        assert np.array_equal(hot, _host_hot(pc, n_hot)), i         # and the list is this rank's own


def test_camera_change_and_size_change_and_back(rrt):
    """Another camera or size is another key: plain order, a new measurement, a list of the new frame's costs -- never the stale one."""
    sc, cam = _scene(rrt, "helmet")
    a_fresh, _ = _fresh(rrt, sc, 72, 40)
    b_fresh, _ = _fresh(rrt, sc, 44, 27)
    sc.release()
    lists = {}
    for i, wh in enumerate(((72, 40), (72, 40), (44, 27), (44, 27), (72, 40), (72, 40))):
        f, s = _render(rrt, sc, *wh)
        slots, n_hot, used, pc, hot = _hot_state(rrt, sc)
        assert s["pixels"] == wh[0] * wh[1] and np.array_equal(f, a_fresh if wh == (72, 40) else b_fresh), i
        assert used == (n_hot if i % 2 else 0) and n_hot == slots // 4 and np.array_equal(hot, _host_hot(pc, n_hot)), i
        assert np.array_equal(lists.setdefault(wh, hot), hot), i
    assert not np.array_equal(lists[(72, 40)][:len(lists[(44, 27)])], lists[(44, 27)])
    # the camera moves on the warmed handle
    sc.set_camera(rrt.Camera(position=tuple(float(x) + 0.05 for x in cam[0]), pitch=cam[1] - 7.0, yaw=cam[2] + 11.0))
    g_warm, sw = _render(rrt, sc, 72, 40)
    _, n_hot, used, pc_g, hot_g = _hot_state(rrt, sc)
    assert used == 0 and np.array_equal(hot_g, _host_hot(pc_g, n_hot)) and not np.array_equal(hot_g, lists[(72, 40)])
    g_again, _ = _render(rrt, sc, 72, 40)
    assert _hot_state(rrt, sc)[2] == n_hot and np.array_equal(g_again, g_warm)
    g_fresh, _ = _fresh(rrt, sc, 72, 40)
    assert sw["pixels"] == 72 * 40 and np.array_equal(g_warm, g_fresh) and not np.array_equal(g_fresh, a_fresh)


def test_both_traversal_modes_in_turn_on_one_handle(rrt):
    """The traversal mode is not part of the key, yet it sets the grid (5 blocks per CU culled, 4 un-culled) and so, where the quarter
    does not cap it, H: at 2560x1440 (921 600 = a quarter of the slots) a 256-CU device makes a list of 655 360 behind a culled launch
    and of 524 288 behind an un-culled one.  A launch runs with the list AND the H of the launch before it, whatever its own grid: the
    frames are a fresh handle's bit for bit, no pixel is left out, and each list is the host selection at its own H."""
    from rust_ray_tracing_amd import _lib as L
    sc, _ = _scene(rrt, "helmet")
    w, h = 2560, 1440
    modes = {"culled": L.TRAVERSAL_CULLED, "reference": L.TRAVERSAL_REFERENCE}
    ref = {m: _fresh(rrt, sc, w, h, traversal=t)[0] for m, t in modes.items()}
    sc.release()
    made, before = {}, 0
    for i, m in enumerate(("reference", "culled", "reference", "culled", "culled")):
        f, s = _render(rrt, sc, w, h, traversal=modes[m])
        slots, n_hot, used, pc, hot = _hot_state(rrt, sc)
        assert s["pixels"] == w * h and np.array_equal(f, ref[m]), (i, m)                  # NaN-free too: ref is, and the bits are equal
        assert used == before, (i, m)                                                      # the list and the H of the launch before
        assert slots == w * h and 0 < n_hot < slots // 4 and np.array_equal(hot, _host_hot(pc, n_hot)), (i, m)
        assert made.setdefault(m, n_hot) == n_hot
        before = n_hot
    assert not np.isnan(ref["culled"].view(np.float32)).any() and not np.isnan(ref["reference"].view(np.float32)).any()
    assert made["culled"] > made["reference"]                                              # the case this test is about
