"""-m gpu: what keeps the cost-ordered list alive, slot by slot.  A plain single-view launch measures the rays of every slot (local tile
* 64 + pixel of the tile).  Where `samples` and `samples * (max_ray_depth + 1)` fit their fields (12 and 20 bits) the lane carries its
pixel's rays in its sample counter and stores them once, beside the frame, into a buffer that is zeroed only when it is new or the
image's shape changes; else every path adds its rays with an atomic into a buffer zeroed for the launch, as every launch did before.
libmipt_diag.so can force the second path on a handle, so both run on the same options here and must agree word for word.  Behind the
launch the tile sort is queued only where a launch can read its result: the diagnostics make the order on demand.  The scratch table of
the selection kernels is sized by the largest key a handle has seen and reused by every smaller one.  All of it is scheduling: frames
are a fresh handle's bit for bit.
The scene is the 20 k-triangle atrium; 70x38 has ragged tiles on both sides, 264x200 is 52 800 slots, seven blocks of the selection
kernels with a partly filled last one."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RAGGED = (70, 38)
PACK_SAMPLES, PACK_RAYS = (1 << 12) - 1, (1 << 20) - 1      # the largest sample count and samples * (max_ray_depth + 1) that pack


@pytest.fixture(scope="module")
def arrays():
    from rust_ray_tracing_amd import synth
    return synth.make_scene("atrium", n_target=20000, tex_size=32)


def _scene(rrt, arrays):
    tris, mats, texs, cam = arrays
    sc = rrt.Scene.from_arrays(tris, mats, texs)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    return sc


def _render(rrt, sc, w, h, spp, depth, n_pixels=None, **kw):
    """One mipt_render on the scene's current handle into a buffer full of NaN: (frame as u32 bits, stats)."""
    from rust_ray_tracing_amd import _lib as L
    buf = np.full((n_pixels if n_pixels else w * h) * 3, np.nan, dtype=np.float32)
    o = rrt.make_options(w, h, spp, depth, traversal=L.TRAVERSAL_CULLED, **kw)
    st = L.MiptStats()
    L.check(rrt.load().mipt_render(sc.upload(0), L.ptr(sc.camera.uniform), C.byref(o), L.ptr(buf), None, C.byref(st)), "mipt_render")
    return buf.view(np.uint32).copy(), st.as_dict()


def _atomics(rrt, sc, on=True):
    diag = rrt.load_diag()
    assert diag.mipt_diag_scene_cost_atomics(sc.upload(0), 1 if on else 0) == 0, diag.mipt_diag_last_error()


def _state(rrt, sc):
    """Read from the scene's current handle: slots, H, hot entries taken, pixel cost, list length, list entries taken, list, bitmap."""
    diag = rrt.load_diag()
    info = (C.c_uint32 * 3)()
    assert diag.mipt_diag_scene_hot_pixels(sc.upload(0), None, 0, None, 0, C.byref(info)) == 0, diag.mipt_diag_last_error()
    n, h = int(info[0]), int(info[1])
    cost, hot = np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32), np.zeros(max(h, 1), dtype=np.uint32)
    assert diag.mipt_diag_scene_hot_pixels(sc.upload(0), cost.ctypes.data, n, hot.ctypes.data, h, C.byref(info)) == 0, diag.mipt_diag_last_error()
    li = (C.c_uint32 * 2)()
    assert diag.mipt_diag_scene_list(sc.upload(0), None, 0, C.byref(li)) == 0, diag.mipt_diag_last_error()
    m = int(li[0])
    lst = np.full(max(m, 1), 0xFFFFFFFF, dtype=np.uint32)
    assert diag.mipt_diag_scene_list(sc.upload(0), lst.ctypes.data, m, C.byref(li)) == 0, diag.mipt_diag_last_error()
    bits = np.zeros(n // 32, dtype=np.uint32)
    assert diag.mipt_diag_scene_hot_bits(sc.upload(0), bits.ctypes.data, len(bits)) == 0, diag.mipt_diag_last_error()
    assert np.array_equal(hot[:h], lst[:h])
    return dict(n=n, hot_n=h, hot_used=int(info[2]), cost=cost[:n], list_n=m, list_used=int(li[1]), list=lst[:m],
                bits=np.unpackbits(bits.view(np.uint8), bitorder="little").astype(bool))


def _tile_state(rrt, sc):
    """(valid, used, tile cost, tile order) through the tile order's hook."""
    diag = rrt.load_diag()
    info = (C.c_uint32 * 3)()
    assert diag.mipt_diag_scene_tile_order(sc.upload(0), None, None, 0, C.byref(info)) == 0, diag.mipt_diag_last_error()
    n = int(info[0])
    cost, order = np.zeros(max(n, 1), dtype=np.uint32), np.full(max(n, 1), 0xFFFFFFFF, dtype=np.uint32)
    assert diag.mipt_diag_scene_tile_order(sc.upload(0), cost.ctypes.data, order.ctypes.data, n, C.byref(info)) == 0, diag.mipt_diag_last_error()
    return bool(info[1]), bool(info[2]), cost[:n], order[:n]


def _host_sort(cost, per_path):
    """A stable counting sort: bucket min(1023, floor(cost * 16 / per_path)) descending, index ascending within a bucket."""
    scale = np.float32(16.0) / np.float32(per_path)
    b = np.minimum(np.floor(cost.astype(np.float32) * scale), np.float32(1023.0)).astype(np.int64)
    return np.argsort(1023 - b, kind="stable").astype(np.uint32)


def _inside(w, h, world=1, rank=0):
    """Per local slot of rank `rank`: is it a pixel of the image?"""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    gt = np.arange(rank, tx * ty, world)
    px = ((gt % tx) * 8)[:, None] + (np.arange(64) & 7)[None, :]
    py = ((gt // tx) * 8)[:, None] + (np.arange(64) >> 3)[None, :]
    return ((px < w) & (py < h)).reshape(-1)


def _check_upkeep(rrt, sc, w, h, spp):
    """The state behind the last launch against the host sort of the costs read back; returns the state."""
    s = _state(rrt, sc)
    inside = _inside(w, h)
    n = len(inside)
    assert s["n"] == n and s["hot_n"] == n // 4 and s["list_n"] == n
    assert np.array_equal(s["cost"] == 0, ~inside), "a slot reads 0 exactly when it is no pixel"
    assert np.array_equal(s["list"], _host_sort(s["cost"], spp)) and s["bits"].all() and len(s["bits"]) == n
    n_img = w * h
    assert inside[s["list"][:n_img]].all() and not inside[s["list"][n_img:]].any(), "the list ends with exactly the slots that are no pixels"
    valid, _, tile_cost, order = _tile_state(rrt, sc)
    assert valid and np.array_equal(tile_cost, s["cost"].reshape(-1, 64).sum(axis=1, dtype=np.uint32))
    assert np.array_equal(order, _host_sort(tile_cost, 64 * spp)), "the tile order made on demand: the launch queued no sort"
    return s


@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("depth", [2, 64])
@pytest.mark.parametrize("seed_mode", [0, 1])
def test_packed_costs_equal_the_atomic_path(rrt, arrays, seed_mode, depth, spp):
    from rust_ray_tracing_amd import _lib as L
    w, h = RAGGED
    sc = _scene(rrt, arrays)
    _, counted = _render(rrt, sc, w, h, spp, depth, seed_mode=seed_mode, flags=L.FLAG_COUNT)
    f_pack, _ = _render(rrt, sc, w, h, spp, depth, seed_mode=seed_mode)
    packed = _check_upkeep(rrt, sc, w, h, spp)
    sc.release()
    _atomics(rrt, sc)
    f_atom, _ = _render(rrt, sc, w, h, spp, depth, seed_mode=seed_mode)
    atomic = _check_upkeep(rrt, sc, w, h, spp)
    sc.release()
    assert np.array_equal(packed["cost"], atomic["cost"]) and np.array_equal(packed["list"], atomic["list"])
    assert int(packed["cost"].sum(dtype=np.uint64)) == counted["rays"]
    assert np.array_equal(f_pack, f_atom) and not np.isnan(f_pack.view(np.float32)).any()


@pytest.mark.parametrize("spp,depth", [(PACK_SAMPLES, 2), (PACK_SAMPLES + 1, 2), (1023, 1024), (1024, 1023)])
def test_both_sides_of_the_hosts_choice(rrt, arrays, spp, depth):
    """4 095 samples pack and 4 096 do not; 1 023 x (1 024 + 1) = 2^20 - 1 rays pack and 1 024 x (1 023 + 1) = 2^20 do not.  One tile."""
    assert spp * (depth + 1) in (PACK_SAMPLES * 3, (PACK_SAMPLES + 1) * 3, PACK_RAYS, PACK_RAYS + 1)
    sc = _scene(rrt, arrays)
    fresh, st = _render(rrt, sc, 8, 8, spp, depth)
    first = _state(rrt, sc)
    again, _ = _render(rrt, sc, 8, 8, spp, depth)             # every work index from the list
    second = _state(rrt, sc)
    sc.release()
    _atomics(rrt, sc)
    f_atom, _ = _render(rrt, sc, 8, 8, spp, depth)
    atomic = _state(rrt, sc)
    sc.release()
    assert st["pixels"] == 64 and second["list_used"] == 64 and not np.isnan(fresh.view(np.float32)).any()
    assert np.array_equal(again, fresh) and np.array_equal(f_atom, fresh)
    assert (first["cost"] >= spp).all() and (first["cost"] <= spp * max(depth, 1)).all()
    assert np.array_equal(first["cost"], atomic["cost"]) and np.array_equal(second["cost"], atomic["cost"])
    assert np.array_equal(first["list"], _host_sort(first["cost"], spp)) and np.array_equal(first["list"], atomic["list"])


def test_slots_outside_the_image_stay_zero_without_the_memset(rrt, arrays):
    """Three launches of the ragged image, a larger one whose pixels cover every slot of the small one, the small one again."""
    spp, depth = 2, 6
    sc = _scene(rrt, arrays)
    small = None
    for i, (w, h) in enumerate((RAGGED, RAGGED, RAGGED, (96, 56), RAGGED, RAGGED)):
        f, st = _render(rrt, sc, w, h, spp, depth)
        s = _check_upkeep(rrt, sc, w, h, spp)
        assert st["pixels"] == w * h and s["list_used"] == (s["n"] if i in (1, 2, 5) else 0), i
        if (w, h) == RAGGED:
            small = small or (f, s)
            assert np.array_equal(f, small[0]) and np.array_equal(s["cost"], small[1]["cost"]) and np.array_equal(s["list"], small[1]["list"]), i
        else:
            assert (s["cost"][:len(small[1]["cost"])] > 0).all(), "the larger image has a pixel in every slot of the smaller one"
    sc.release()


def test_a_small_key_behind_a_large_one_on_one_handle(rrt, arrays):
    """264x200 is seven blocks of the selection kernels, 70x38 one: the small key's kernels run in the scratch table the large one left
    full -- at 1 spp and depth 64, where a pixel that runs the full depth falls into the top bucket -- and the list made there must still be the host sort
    of the costs, and the launch that takes its work from it must still trace every pixel once."""
    spp, depth = 1, 64
    sc = _scene(rrt, arrays)
    fresh = {}
    for w, h in ((264, 200), RAGGED):
        fresh[(w, h)], _ = _render(rrt, sc, w, h, spp, depth)
        sc.release()
    for i, (w, h) in enumerate(((264, 200), (264, 200), RAGGED, RAGGED, RAGGED, (264, 200), RAGGED, RAGGED)):
        f, st = _render(rrt, sc, w, h, spp, depth)
        s = _check_upkeep(rrt, sc, w, h, spp)
        assert st["pixels"] == w * h and np.array_equal(f, fresh[(w, h)]) and not np.isnan(f.view(np.float32)).any(), i
        assert s["list_used"] == (s["n"] if i in (1, 3, 4, 7) else 0), i
    sc.release()


@pytest.mark.parametrize("w,h", [RAGGED, (264, 200)])
def test_upkeep_equals_a_host_counting_sort(rrt, arrays, w, h):
    """Per-sample seeds with a stepping sample_begin: the view, hence the key, stays and the costs really change from launch to launch."""
    spp, depth = 2, 8
    sc = _scene(rrt, arrays)
    costs = []
    for i in range(3):
        _, st = _render(rrt, sc, w, h, spp, depth, seed_mode=1, sample_begin=1 + i * spp)
        s = _check_upkeep(rrt, sc, w, h, spp)
        assert st["pixels"] == w * h and s["list_used"] == (s["n"] if i else 0) and s["hot_used"] == (s["hot_n"] if i else 0), i
        costs.append(s["cost"])
    assert not np.array_equal(costs[0], costs[1]) and not np.array_equal(costs[1], costs[2])
    sc.release()


@pytest.mark.parametrize("world,rank", [(1, 0), (3, 0), (3, 2)])
@pytest.mark.parametrize("seed_mode", [0, 1])
def test_frames_equal_a_fresh_handles(rrt, arrays, seed_mode, world, rank):
    from rust_ray_tracing_amd import _lib as L
    w, h = RAGGED
    spp, depth = 3, 8
    kw = dict(seed_mode=seed_mode)
    inside = _inside(w, h, world, rank)
    n_slots, own = len(inside), int(inside.sum())
    words = np.ones(w * h * 3, dtype=bool)                    # the words of the buffer the launch writes: the whole frame, or,
    if world > 1:                                             # rank-packed, the slots of the rank's tiles that are pixels
        n_packed = int(rrt.load().mipt_packed_pixels(w, h, world))
        kw.update(n_pixels=n_packed, flags=L.FLAG_PACKED, tile_rank=rank, tile_world=world)
        words = np.zeros(n_packed * 3, dtype=bool)
        words[:n_slots * 3] = np.repeat(inside, 3)
    sc = _scene(rrt, arrays)
    fresh, st = _render(rrt, sc, w, h, spp, depth, **kw)
    sc.release()
    assert st["pixels"] == own and not np.isnan(fresh[words].view(np.float32)).any()
    for i in range(3):
        f, s = _render(rrt, sc, w, h, spp, depth, **kw)
        state = _state(rrt, sc)
        assert s["pixels"] == own and np.array_equal(f[words], fresh[words]), i
        assert state["n"] == state["list_n"] == n_slots and state["list_used"] == (n_slots if i else 0), i
        assert np.array_equal(state["list"], _host_sort(state["cost"], spp)), i
        assert np.array_equal(state["cost"] == 0, ~_inside(w, h, world, rank)), i
    sc.release()
