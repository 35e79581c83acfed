"""-m gpu: the list behind the hot pixels holds every local slot in cost order, and it is pure scheduling.  A plain single-view launch
measures the rays of every slot (tests/test_gpu_hot_pixels.py); the selection kernels behind it write the complete stable counting
sort of the slots -- 1 024 buckets of rays per path x 16 descending, slot index ascending within a bucket, so the slots of cost 0
(which are no pixels of the image) come last -- and the next launch with the same key and camera takes every work index from that
list: no walk over the tiles is left.  The first H entries are the hot list as it always was.  Whatever the list holds, a frame's bits
are a fresh handle's and every pixel is written once: 72x40 is 45 tiles; 70x37 has ragged edges (slots that are listed, cost nothing
and are skipped); 256x144 has more slots than one block of the selection kernels owns.  The key leaves out the ray depth and a geometry
update does not touch the state: both leave a list of costs that are no longer the frame's, and the frame must not care."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEPTH = 8
SIZES = [(72, 40), (70, 37), (256, 144)]


def _arrays(kind):
    from rust_ray_tracing_amd import synth
    return synth.cornell_box() if kind == "cornell" else synth.helmet_scene(n_target=2000, tex_size=64)


def _scene(rrt, kind, tris=None):
    t, mats, texs, cam = _arrays(kind)
    sc = rrt.Scene.from_arrays(t if tris is None else tris, mats, texs)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    return sc


def _render(rrt, sc, w, h, spp=4, depth=DEPTH, n_pixels=None, traversal=None, **kw):
    """One mipt_render on the scene's current handle into a buffer full of NaN: (frame as u32 bits, stats)."""
    from rust_ray_tracing_amd import _lib as L
    buf = np.full((n_pixels if n_pixels else w * h) * 3, np.nan, dtype=np.float32)
    o = rrt.make_options(w, h, spp, depth, traversal=L.TRAVERSAL_CULLED if traversal is None else traversal, **kw)
    st = L.MiptStats()
    L.check(rrt.load().mipt_render(sc.upload(0), L.ptr(sc.camera.uniform), C.byref(o), L.ptr(buf), None, C.byref(st)), "mipt_render")
    return buf.view(np.uint32).copy(), st.as_dict()


def _fresh(rrt, sc, w, h, **kw):
    sc.release()                                     # the next upload() makes a new handle: no state
    return _render(rrt, sc, w, h, **kw)


def _host_list(cost, samples):
    """The complete order the selection must give: bucket min(1023, floor(cost * 16 / samples)) descending, slot index ascending."""
    scale = np.float32(16.0) / np.float32(samples)
    b = np.minimum(np.floor(cost.astype(np.float32) * scale), np.float32(1023.0)).astype(np.int64)
    return np.argsort(1023 - b, kind="stable").astype(np.uint32)


def _state(rrt, sc):
    """(slots, H, hot entries taken, pixel cost, hot list, list length, list entries taken, list) of the scene's current handle."""
    diag = rrt.load_diag()
    info = (C.c_uint32 * 3)()
    assert diag.mipt_diag_scene_hot_pixels(sc.upload(0), None, 0, None, 0, C.byref(info)) == 0, diag.mipt_diag_last_error()
    n, h = int(info[0]), int(info[1])
    cost, hot = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(h, 1), dtype=np.uint32)
    assert diag.mipt_diag_scene_hot_pixels(sc.upload(0), cost.ctypes.data, n, hot.ctypes.data, h, C.byref(info)) == 0, diag.mipt_diag_last_error()
    li = (C.c_uint32 * 2)()
    assert diag.mipt_diag_scene_list(sc.upload(0), None, 0, C.byref(li)) == 0, diag.mipt_diag_last_error()
    m = int(li[0])
    lst = np.full(max(m, 1), 0xFFFFFFFF, dtype=np.uint32)
    assert diag.mipt_diag_scene_list(sc.upload(0), lst.ctypes.data, m, C.byref(li)) == 0, diag.mipt_diag_last_error()
    if m > 1:
        assert diag.mipt_diag_scene_list(sc.upload(0), lst.ctypes.data, m - 1, C.byref(li)) == -1      # a buffer one word short is refused
    return n, h, int(info[2]), cost[:n], hot[:h], m, int(li[1]), lst[:m]


def _inside(w, h):
    """Per slot of a one-rank frame: is it a pixel of the image?"""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    gt = np.arange(tx * ty)
    px = ((gt % tx) * 8)[:, None] + (np.arange(64) & 7)[None, :]
    py = ((gt // tx) * 8)[:, None] + (np.arange(64) >> 3)[None, :]
    return ((px < w) & (py < h)).reshape(-1)


@pytest.mark.parametrize("seed_mode", [0, 1])
@pytest.mark.parametrize("spp", [4, 3])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("kind", ["cornell", "helmet"])
def test_full_list_frames_equal_a_fresh_handles(rrt, kind, w, h, spp, seed_mode):
    sc = _scene(rrt, kind)
    kw = dict(spp=spp, seed_mode=seed_mode)
    f1, s1 = _fresh(rrt, sc, w, h, **kw)              # plain order, measures
    n, n_hot, used, pc, hot, m, took, lst = _state(rrt, sc)
    inside = _inside(w, h)
    assert n == len(inside) and n_hot == n // 4 and used == 0 and took == 0
    assert m == n, "the list holds every local slot"
    want = _host_list(pc, spp)
    assert np.array_equal(lst, want) and np.array_equal(lst[:n_hot], hot)
    # every slot once; the image's pixels are exactly the entries that cost something, and they come before all the others
    assert np.array_equal(np.sort(lst), np.arange(n, dtype=np.uint32))
    n_img = int(inside.sum())
    assert n_img == w * h and inside[lst[:n_img]].all() and not inside[lst[n_img:]].any() and (pc[lst[n_img:]] == 0).all()
    frames = [(f1, s1)]
    for _ in range(2):                                # frames 2 and 3: every work index from the list
        frames.append(_render(rrt, sc, w, h, **kw))
        _, n_hot2, used2, pc2, hot2, m2, took2, lst2 = _state(rrt, sc)
        assert (n_hot2, used2, m2, took2) == (n_hot, n_hot, n, n)
        assert np.array_equal(pc2, pc) and np.array_equal(lst2, lst) and np.array_equal(hot2, hot)      # the same frame costs the same
    for f, s in frames:
        assert s["pixels"] == w * h and not np.isnan(f.view(np.float32)).any()
        assert np.array_equal(f, f1)


def test_one_sample_per_pixel(rrt):
    sc = _scene(rrt, "helmet")
    w, h = 70, 37
    f1, s1 = _fresh(rrt, sc, w, h, spp=1)
    f2, s2 = _render(rrt, sc, w, h, spp=1)
    n, _, _, pc, _, m, took, lst = _state(rrt, sc)
    assert m == n == took and np.array_equal(lst, _host_list(pc, 1))
    assert s1["pixels"] == s2["pixels"] == w * h and np.array_equal(f2, f1) and not np.isnan(f2.view(np.float32)).any()


def test_packed_two_rank_shard(rrt):
    from rust_ray_tracing_amd import _lib as L
    sc = _scene(rrt, "helmet")
    w, h = 72, 40
    n_packed = int(rrt.load().mipt_packed_pixels(w, h, 2))
    own = lambda rank: ((45 + 1 - rank) // 2) * 64               # slots of the rank's own tiles: 23 and 22 of the 45
    for rank in (0, 1):
        kw = dict(n_pixels=n_packed, flags=L.FLAG_PACKED, tile_rank=rank, tile_world=2)
        ref, sr = _fresh(rrt, sc, w, h, **kw)
        again, sa = _render(rrt, sc, w, h, **kw)
        n, n_hot, used, pc, hot, m, took, lst = _state(rrt, sc)
        assert n == own(rank) == m == took and used == n_hot == n // 4
        assert np.array_equal(lst, _host_list(pc, 4)) and np.array_equal(lst[:n_hot], hot)
        assert sr["pixels"] == sa["pixels"] == own(rank) and np.array_equal(again[:own(rank) * 3], ref[:own(rank) * 3])
        assert not np.isnan(again[:own(rank) * 3].view(np.float32)).any()
    # both ranks in turn on one handle: every change of rank is a change of key, and the list is the rank's own
    sc.release()
    for i, rank in enumerate((0, 0, 1, 1, 0)):
        kw = dict(n_pixels=n_packed, flags=L.FLAG_PACKED, tile_rank=rank, tile_world=2)
        f, _ = _render(rrt, sc, w, h, **kw)
        sc2 = _scene(rrt, "helmet")
        ref, _ = _render(rrt, sc2, w, h, **kw)
        sc2.release()
        assert np.array_equal(f[:own(rank) * 3], ref[:own(rank) * 3]), i
        n, _, _, pc, _, m, took, lst = _state(rrt, sc)
        assert m == n == own(rank) and took == (n if i in (1, 3) else 0), i
        assert np.array_equal(lst, _host_list(pc, 4)), i


def test_both_traversal_modes_in_turn_on_one_handle(rrt):
    """The traversal mode is not part of the key: a launch takes the list of the launch before it, whichever mode made it."""
    from rust_ray_tracing_amd import _lib as L
    sc = _scene(rrt, "helmet")
    w, h = 70, 37
    modes = {"culled": L.TRAVERSAL_CULLED, "reference": L.TRAVERSAL_REFERENCE}
    ref = {m: _fresh(rrt, sc, w, h, traversal=t)[0] for m, t in modes.items()}
    sc.release()
    for i, m in enumerate(("reference", "culled", "reference", "culled", "culled")):
        f, s = _render(rrt, sc, w, h, traversal=modes[m])
        n, _, _, pc, _, ln, took, lst = _state(rrt, sc)
        assert s["pixels"] == w * h and np.array_equal(f, ref[m]), (i, m)
        assert ln == n and took == (n if i else 0) and np.array_equal(lst, _host_list(pc, 4)), (i, m)
    assert not np.isnan(ref["culled"].view(np.float32)).any() and not np.isnan(ref["reference"].view(np.float32)).any()


@pytest.mark.parametrize("kind", ["cornell", "helmet"])
def test_stale_costs_after_a_change_of_depth(rrt, kind):
    """max_ray_depth is not in the key: a depth-5 (depth-1) frame runs in the order of the depth-8 (depth-5) costs and is a fresh
    handle's frame of its own depth; the list made behind it is its own frame's."""
    sc = _scene(rrt, kind)
    w, h = 72, 40
    want = {d: _fresh(rrt, sc, w, h, depth=d)[0] for d in (8, 5, 1)}
    sc.release()
    for i, depth in enumerate((8, 8, 5, 5, 1, 1, 8)):
        f, s = _render(rrt, sc, w, h, depth=depth)
        n, _, _, pc, _, m, took, lst = _state(rrt, sc)
        assert s["pixels"] == w * h and np.array_equal(f, want[depth]) and not np.isnan(f.view(np.float32)).any(), i
        assert m == n and took == (n if i else 0) and np.array_equal(lst, _host_list(pc, 4)), i


def test_stale_costs_after_a_geometry_update(rrt):
    """mipt_scene_update_triangles leaves the state alone: the frame after it runs in the old geometry's order and is still the
    frame of a handle that got the same update without ever having rendered."""
    w, h = 70, 37
    ref = _scene(rrt, "helmet")
    ref.upload(0)
    moved = ref.tris.copy()                           # the scene's own order of triangles, the same on every handle made this way
    k0, k1 = len(moved) // 3, len(moved) // 3 + len(moved) // 4
    moved["vertices"]["position"][k0:k1] += np.array([0.25, -0.5, 0.125], dtype=np.float32)   # a contiguous quarter moves as one piece
    ref.tris = moved.copy()
    ref.update_device(0)
    want, _ = _render(rrt, ref, w, h)
    ref.release()
    sc = _scene(rrt, "helmet")
    before, _ = _render(rrt, sc, w, h)
    _render(rrt, sc, w, h)
    assert _state(rrt, sc)[6] == _state(rrt, sc)[0]
    sc.tris = moved.copy()
    sc.update_device(0)
    assert not np.array_equal(before, want)
    for i in range(2):
        f, s = _render(rrt, sc, w, h)
        n, _, _, pc, _, m, took, lst = _state(rrt, sc)
        assert s["pixels"] == w * h and np.array_equal(f, want) and not np.isnan(f.view(np.float32)).any(), i
        assert m == n == took and np.array_equal(lst, _host_list(pc, 4)), i
    sc.release()
