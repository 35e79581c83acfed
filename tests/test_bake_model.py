"""CPU: the second statement of the texel model (tests/tools/bake_model.py::texels_indexed -- pairs enumerated from the exact box
clause) against the first (::texels, the brute force over all triangles per texel), on the bytes and in `info`: on every small layout
of tests/test_gpu_bake.py and on the sliver layouts, where the box clause decides texels, with a NaN triangle, a triangle of three
times the atlas and random triangles mixed in.  The GPU tests hold the kernels to texels_indexed where the brute force is too slow."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bake_model as B  # noqa: E402
import test_gpu_bake as G  # noqa: E402  (the layouts; nothing of it runs on a device here)


def _same(tris, w, h, **kw):
    want, winfo = B.texels(tris, w, h)
    stats = {}
    got, info = B.texels_indexed(tris, w, h, stats=stats, **kw)
    assert B.same_bits(got, want), (w, h, G._bad_texels(got, want))
    assert info == winfo
    assert int(stats["owned"].sum()) == winfo["covered"] and stats["pairs"] >= winfo["covered"]
    return want, winfo, stats


@pytest.mark.parametrize("w,h", G.QUAD_SIZES)
def test_indexed_model_on_the_quad(rrt, w, h):
    want, winfo, _ = _same(G._layout_tris(rrt, G._quad_layout(w, h)), w, h)
    assert winfo["covered"] >= 1 and set((want["prim"][want["prim"] != B.NONE] & B.TRI_MASK).tolist()) == ({20} if (w, h) == (1, 1) else {20, 41})


def test_indexed_model_on_identical_uvs_and_on_unusable_triangles(rrt):
    want, _, _ = _same(G._layout_tris(rrt, {40: G.IDENTICAL_TRI, 5: G.IDENTICAL_TRI}), 16, 16)
    assert set((want["prim"][want["prim"] != B.NONE] & B.TRI_MASK).tolist()) == {5}
    want, winfo, _ = _same(G._layout_tris(rrt, G.DEGENERATE), 24, 20)
    assert winfo["degenerate"] == 3 and set((want["prim"][want["prim"] != B.NONE] & B.TRI_MASK).tolist()) == {30, 44}


def _mixed_slivers(rrt, w, h, n, k):
    """the slivers of the GPU test with a NaN corner, a triangle of three times the atlas and 20 random triangles over [-0.2, 1.2]^2
    at seeded indices among them"""
    tris = G._sliver_tris(rrt, w, h, n, k)
    rng = np.random.default_rng(41)
    where = rng.choice(n, 22, replace=False)
    for i in where[:20]:
        G._set_uv(tris, i, rng.uniform(-0.2, 1.2, (3, 2)))
    G._set_uv(tris, where[20], [(0.3, 0.2), (float("nan"), 0.7), (0.1, 0.9)])
    G._set_uv(tris, where[21], [(-1.0, -1.0), (2.0, -0.9), (-0.8, 2.0)])
    return tris, where


@pytest.mark.parametrize("w,h,n,k", [(96, 96, 128, 2), (97, 31, 128, 2)])
def test_indexed_model_on_slivers(rrt, w, h, n, k):
    tris, where = _mixed_slivers(rrt, w, h, n, k)
    want, winfo, stats = _same(tris, w, h)
    loose, _ = B.texels(tris, w, h, box=False)
    plain, _ = B.texels(G._sliver_tris(rrt, w, h, n, k), w, h)
    plain_loose, _ = B.texels(G._sliver_tris(rrt, w, h, n, k), w, h, box=False)
    assert int((plain["prim"] != plain_loose["prim"]).sum()) >= 8            # the clause decides texels of the slivers themselves
    assert int((want["prim"] != loose["prim"]).sum()) >= 1
    assert winfo["degenerate"] >= 2 and stats["owned"][where[21]] > 0 and stats["owned"][where[:20]].sum() > 0
    # slices that end inside a triangle's pairs, and one pair at a time across a whole small box
    _same(tris, w, h, chunk=997)
    small = tris[:12]
    _same(small, w, h, chunk=1)


def test_box_keyword_changes_nothing_without_slivers(rrt):
    tris = G._layout_tris(rrt, G._quad_layout(32, 32))
    a, ai = B.texels(tris, 32, 32)
    b, bi = B.texels(tris, 32, 32, box=False)
    assert B.same_bits(a, b) and ai == bi


def test_big_layout_classes_are_unambiguous(rrt):
    """the layout of the GPU test past cover_kernel's lanes, at a size the CPU takes in a second: every triangle falls into one of the
    three classes of box whatever the kernel's padding does, the indexed model equals the brute force on sampled texels"""
    n = 40000
    tris = G._soup(rrt, n, seed=14)
    uv = G._big_uvs(n)
    tris["vertices"]["tex_coord_x"], tris["vertices"]["tex_coord_y"] = uv[..., 0], uv[..., 1]
    cls = G._classes(tris, G.BIG_W, G.BIG_H)
    assert not np.any(cls < 0) and int((cls == 2).sum()) >= 36 and int((cls == 1).sum()) >= n // 17
    want, winfo = B.texels_indexed(tris, G.BIG_W, G.BIG_H)
    assert winfo["degenerate"] >= 64
    index = np.sort(np.random.default_rng(15).choice(G.BIG_W * G.BIG_H, 512, replace=False)).astype(np.uint32)
    brute, _ = B.texels(tris, G.BIG_W, G.BIG_H, index)
    assert B.same_bits(brute, want[index])
