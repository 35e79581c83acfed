"""CPU: the scenes and rays of tests/tools/traverse_cases.py, held to what they are for on the models alone.

tests/test_gpu_traverse_corpus.py compares three kernels with the models on these inputs.  It could pass without ever popping a
child-ref entry if the inputs never stacked the big leaf, so every reach is asserted here first, on the oracle's builder and on
query_model.traverse's event list: which node the bunch is, that it is stacked after the swap (left) or without it (right) and popped,
that it is entered as the near child, that rays hit several of its triangles, miss everything, end early under occlusion, take both
slab paths; for the corpus, the leaf sizes, pop depths and stack heights that DESIGN section 21 quotes.  The asserts are conditions on
the inputs, not measurements of the kernels: if a seed misses one, the seed or the recipe changes, never the condition."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import bvh_corpus as bc  # noqa: E402
import features_model as F  # noqa: E402
import query_model as Q  # noqa: E402
import traverse_cases as T  # noqa: E402

ALL_SIZES = T.LEAF_SIZES + (T.LEAF_SIZE_BIG,)
FRAME = (24, 16)


# ---- the event list is an addition: answers and counters are what they were without it -------------------------------------------------
def test_events_change_nothing_and_add_up(rrt, orc):
    c = T.leaf_case(rrt, orc, 64, "left")
    sc, rays = c["sc"], c["rays"]
    plain = Q.per_ray(orc.load(), sc.tris, sc.bvh_nodes, rays)
    hits, occ, per, events = c["ref"]
    assert Q.same_bits(hits, plain[0]) and np.array_equal(occ, plain[1])
    assert all(np.array_equal(per[k], plain[2][k]) for k in per)
    for i, ev in enumerate(events):                          # every pop of a leaf was a push of it, and the stack height is the counter's
        pushed = sorted(e[1] for e in ev if e[0] == "push")
        popped = sorted(e[1] for e in ev if e[0] == "pop")
        assert all(p in pushed for p in popped), i
        assert max([e[4] for e in ev if e[0] == "push"] or [0]) <= per["max_stack"][i]


# ---- left and right: which node, which form, which way in -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["left", "right"])
@pytest.mark.parametrize("m", ALL_SIZES)
def test_bunch_is_the_first_or_the_second_child(rrt, orc, m, shape):
    """On the ORACLE's builder the bunch is node 1 (left) or node 2 (right), one leaf of m; the host builder, whose tree the GPU file
    uploads, gives the same tree"""
    tris = T.leaf_tris(m, shape)
    _, ref_nodes = orc.bvh_build(tris)
    nd = T.as_nodes(ref_nodes)
    assert T.bunch_node(ref_nodes, m) == (1 if shape == "left" else 2)
    assert nd["num_tris"][0] == 0 and nd["first_tri_or_child"][0] == 1 and nd["num_tris"].max() == m
    assert nd["num_tris"][3 - T.bunch_node(ref_nodes, m)] == 0                       # the remainder is an inner node: an inner entry is stacked for it
    c = T.leaf_case(rrt, orc, m, shape)
    assert bc.first_difference(c["sc"].bvh_nodes, ref_nodes) is None
    assert len(set(int(x) for x in c["sc"].tris["material_id"][c["first"]: c["first"] + m])) == len(T.PALETTE) >= 7
    mats = c["sc"].materials_array()
    assert len({tuple(x["base_color"]) for x in mats}) == len(mats) and len({tuple(x["emission"]) for x in mats}) == len(mats)


@pytest.mark.parametrize("shape", ["left", "right"])
@pytest.mark.parametrize("m", ALL_SIZES)
def test_leaf_scene_rays_reach_every_way_into_the_bunch(rrt, orc, m, shape):
    c = T.leaf_case(rrt, orc, m, shape)
    sc, rays, family, node = c["sc"], c["rays"], c["family"], c["node"]
    n = len(rays)
    assert 40 <= n <= 120
    hits, occ, per, events = c["ref"]
    popped, entered, swaps = T.leaf_events(events, node)
    # child 0 is stacked only after the swap, child 1 only without it; either is also entered as the near child
    assert swaps == {shape == "left"}
    assert popped.sum() >= 8 and entered.sum() >= 8 and not np.any(popped & entered)
    assert all(e[2] == m for ev in events for e in ev if e[1] == node)                # the form: inline up to 63, child-ref from 64
    assert popped[family == "a"].sum() >= 8 and entered[family == "b"].sum() >= 8 and popped[family == "d"].sum() >= 4
    # the stacked inner entry of the remainder is popped too (family b leaves through it)
    assert np.all(per["max_stack"][family == "b"] >= 1)
    # both slab paths
    safe = T.ray_safe(rays, T.tiny_axes(sc.bvh_nodes))
    assert 3 * safe.sum() >= n and 3 * (~safe).sum() >= n
    assert np.all(np.abs(rays["direction"][~safe]).max(axis=1) > 2.0)
    # hits, misses, several winners
    bunch = T.in_bunch(c, hits, m)
    assert 4 * bunch.sum() >= n and 10 * (hits["prim"] == Q.NONE).sum() >= n
    assert len(set(int(p) for p in hits["prim"][bunch] & 0x01FFFFFF)) >= 3
    assert np.all(hits["prim"][family == "c"] == Q.NONE) and np.all(per["tri_tests"][family == "c"] == 0)
    # family (d): t_max on both sides of the closest hit
    d = family == "d"
    assert 0 < (hits["prim"][d] != Q.NONE).sum() < d.sum()
    # under occlusion a ray ends inside the big leaf, before its last triangle
    _, occ_any, per_any, _ = T.trace(orc.load(), sc.tris, sc.bvh_nodes, rays, anyhit=True)
    assert np.any((occ_any != 0) & bunch & (per_any["tri_tests"] < per["tri_tests"]))
    for arm in ((True, 0.0), (True, 0.0078125)):                                     # the culled arms stack and pop it as well
        ev = T.trace(orc.load(), sc.tris, sc.bvh_nodes, rays, cull=arm[0], margin=arm[1])[3]
        assert T.leaf_events(ev, node)[0].sum() >= 8


@pytest.mark.parametrize("m", ALL_SIZES)
def test_root_scene_is_one_leaf(rrt, orc, m):
    _, ref_nodes = orc.bvh_build(T.leaf_tris(m, "root"))
    nd = T.as_nodes(ref_nodes)
    assert len(nd) == 1 and nd["num_tris"][0] == m
    c = T.leaf_case(rrt, orc, m, "root")
    assert bc.first_difference(c["sc"].bvh_nodes, ref_nodes) is None and c["node"] == 0
    hits, _, per, events = c["ref"]
    assert 4 * (hits["prim"] != Q.NONE).sum() >= len(hits) and (hits["prim"] == Q.NONE).any()
    assert all(ev == [("enter", 0, m)] for ev in events) and np.all(per["tri_tests"] == m) and np.all(per["inner_steps"] == 0)
    safe = T.ray_safe(c["rays"])
    assert 3 * safe.sum() >= len(safe) and 3 * (~safe).sum() >= len(safe)


# ---- the two cameras of the first-hit and trace tests -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["left", "right"])
@pytest.mark.parametrize("m", [63, 64, 65, 300])
def test_cameras_stack_the_bunch_and_enter_it(rrt, orc, m, shape):
    c = T.leaf_case(rrt, orc, m, shape)
    sc = c["sc"]
    cams = T.leaf_cameras(sc.tris, sc.bvh_nodes, m)
    seen = []
    for cam in cams:
        rays = F.camera_rays(orc, sc, cam, FRAME[0], FRAME[1], 0)[0]
        hits, _, _, events = T.trace(orc.load(), sc.tris, sc.bvh_nodes, rays)
        seen.append(T.leaf_events(events, c["node"]) + (T.in_bunch(c, hits, m), hits))
    assert seen[0][0].sum() >= 8 and seen[0][2] == {shape == "left"}                 # from the remainder's side: stacked and popped
    assert seen[1][1].sum() >= 8                                                     # from the other side: the near child
    for s in seen:
        assert s[3].sum() >= 16 and (s[4]["prim"] == Q.NONE).sum() >= 16             # the bunch and the sky in both frames


# ---- the corpus ----------------------------------------------------------------------------------------------------------------------
_corpus = {}


def _corpus_case(orc, name):
    """(oracle's triangles, nodes, rays, the reference arm's trace), once"""
    if name not in _corpus:
        tris, rays = T.corpus_input(name)
        ref_tris, ref_nodes = orc.bvh_build(tris)
        _corpus[name] = (ref_tris, T.as_nodes(ref_nodes), rays, T.trace(orc.load(), ref_tris, ref_nodes, rays))
    return _corpus[name]


@pytest.mark.parametrize("name", T.CORPUS)
def test_corpus_rays_cross_the_tree(orc, name):
    tris, nodes, rays, (hits, occ, per, events) = _corpus_case(orc, name)
    assert 40 <= len(rays) <= 120 or name == "spiral"
    assert per["stack_overflows"].sum() == 0
    assert np.all(per["inner_steps"] >= 1)                                           # every ray crosses the root's box
    if name != "special_denormal" and name != "size2049_zero_area":                  # slivers and zero areas: no ray hits one, the counters compare
        assert 4 * occ.sum() >= len(rays)
    else:
        assert per["tri_tests"].sum() > 1000 and occ.sum() == 0


def _largest_leaf(nodes):
    i = int(np.argmax(nodes["num_tris"]))
    return i, int(nodes["first_tri_or_child"][i]), int(nodes["num_tris"][i])


@pytest.mark.parametrize("name,size", [("size513_copies", 135), ("size2049_copies", 606)])
def test_copies_leaf_is_popped_and_ties_go_to_the_first(orc, name, size):
    tris, nodes, rays, (hits, occ, per, events) = _corpus_case(orc, name)
    node, first, n = _largest_leaf(nodes)
    assert n == size and n >= 64                                                      # DESIGN section 21 quotes the size
    popped, entered, _ = T.leaf_events(events, node)
    assert popped.sum() >= 4
    if name == "size2049_copies":                                                    # more than 500 triangles, from a stack of at least 4 entries
        assert n > 500 and max(e[3] for ev in events for e in ev if e[0] == "pop" and e[1] == node) >= 4
        assert bc.census(nodes)["levels"] >= 17
    # rays whose closest t is shared: the winner is a copy, and the first copy in visit order
    P = tris["vertices"]["position"].reshape(len(tris), -1)
    prim = hits["prim"] & 0x01FFFFFF
    shared = 0
    for i in np.flatnonzero((hits["prim"] != Q.NONE) & (prim >= first) & (prim < first + n)):
        same = first + np.flatnonzero((P[first: first + n] == P[prim[i]]).all(axis=1))
        if len(same) > 1:
            assert prim[i] == same[0], (i, prim[i], same[:4])
            shared += 1
    assert shared >= 2


@pytest.mark.parametrize("name", ["size513_copies", "size2049_copies"])
def test_close_camera_sees_the_copies(rrt, orc, name):
    """the second camera of the GPU file's first-hit and trace tests on a `copies` soup: pixels whose winner is one of several
    coincident triangles, so that `<=` in a leaf step (the last copy wins, with another material) changes the frame"""
    tris, _ = T.corpus_input(name)
    sc = rrt.Scene.from_arrays(np.array(tris), T.materials())
    frame, counters, _ = F.frame(orc, sc, T.corpus_camera(tris, at_first=True), FRAME[0], FRAME[1], 0)
    P = sc.tris["vertices"]["position"].reshape(len(sc.tris), -1)
    copies = np.flatnonzero((P == tris["vertices"]["position"][0].reshape(-1)).all(axis=1))
    assert len(copies) >= 64 and len(set(int(x) for x in sc.tris["material_id"][copies])) == len(T.PALETTE)
    prim = frame["prim"].reshape(-1)
    on_copy = (prim != Q.NONE) & np.isin(prim & 0x01FFFFFF, copies)
    assert on_copy.sum() >= 16 and np.all((prim[on_copy] & 0x01FFFFFF) == copies[0])   # the first in visit order
    assert counters["max_stack"] >= 4


def test_spiral_goes_past_the_lds_entries_into_the_spill_slots(orc):
    _, nodes, rays, (hits, occ, per, events) = _corpus_case(orc, "spiral")
    assert bc.census(nodes)["levels"] >= 70
    assert per["max_stack"].max() >= 17 and per["stack_overflows"].sum() == 0
    assert per["max_stack"].max() == 36                                              # the figure DESIGN section 21 quotes
    assert (per["max_stack"] >= 17).sum() >= 4 and occ.sum() >= 8
    _, _, per_any, _ = T.trace(orc.load(), _corpus[("spiral")][0], nodes, rays, anyhit=True)
    assert per_any["max_stack"].max() >= 17                                          # an occluded ray stops with spilled entries stacked


def test_spiral_cameras_look_down_every_level(rrt, orc):
    """the cameras of the GPU file's trace (spiral) and first-hit (spiral_small) tests: every pixel hits, from a stack as deep as the rays'"""
    tris, _ = T.corpus_input("spiral")
    sc = rrt.Scene.from_arrays(np.array(tris), T.materials())
    _, _, st = orc.render(sc.tris, sc.bvh_nodes, sc.materials_array(), [], T.corpus_camera(tris, through_core="spiral"), 40, 24, 2, 4)
    assert st["max_stack"] >= 17 and st["max_stack"] == 36 and st["stack_overflows"] == 0 and st["hits"] >= 40 * 24
    tris, _ = T.corpus_input("spiral_small")
    sc = rrt.Scene.from_arrays(np.array(tris), T.materials())
    frame, counters, _ = F.frame(orc, sc, T.corpus_camera(tris, through_core="spiral_small"), FRAME[0], FRAME[1], 0)
    assert counters["hits"] >= 16 and counters["max_stack"] >= 8
    tris, _ = T.corpus_input("size513_copies")
    sc = rrt.Scene.from_arrays(np.array(tris), T.materials())
    frame, counters, _ = F.frame(orc, sc, T.corpus_camera(tris), FRAME[0], FRAME[1], 0)
    assert 16 <= counters["hits"] < FRAME[0] * FRAME[1] and len(np.unique(frame["prim"])) >= 8


def test_zero_area_triangles_are_tested_with_det_zero(orc):
    tris, nodes, rays, (hits, occ, per, events) = _corpus_case(orc, "size2049_zero_area")
    assert per["tri_tests"].sum() > 0 and occ.sum() == 0
    P = tris["vertices"]["position"]
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    assert not e1.any()                                                              # two corners coincide
    with np.errstate(all="ignore"):
        for r in rays[np.isfinite(rays["direction"]).all(axis=1)][:32]:              # ray.rs:24-26 in f32: det = dot(e1, cross(d, e2))
            d = r["direction"]
            c = np.stack([d[1] * e2[:, 2] - d[2] * e2[:, 1], d[2] * e2[:, 0] - d[0] * e2[:, 2], d[0] * e2[:, 1] - d[1] * e2[:, 0]], axis=1)
            det = (e1[:, 0] * c[:, 0] + e1[:, 1] * c[:, 1]) + e1[:, 2] * c[:, 2]
            assert np.all(det == 0)


def test_signed_zeros_and_denormal_boxes_are_in_the_trees(orc):
    _, nodes, rays, _ = _corpus_case(orc, "special_zeros")
    b = np.concatenate([nodes["bounds_min"], nodes["bounds_max"]])
    assert np.any((b == 0) & np.signbit(b)) and np.any((b == 0) & ~np.signbit(b))
    _, nodes, rays, _ = _corpus_case(orc, "special_denormal")
    w = (nodes["bounds_max"] - nodes["bounds_min"])[:, 1:]
    assert np.any((w > 0) & (w < np.finfo(np.float32).tiny))
    assert T.tiny_axes(nodes) == 6 and not T.ray_safe(T.Q.make_rays([[0, 0, 0]], [[1, 1, 1]]), 6)[0]


def test_left_out_entries_are_the_ones_past_the_scene_limits():
    out = [k for k in bc.ENTRIES if k.startswith("overflow")] + ["special_huge", "special_nan"]
    assert not set(out) & set(T.CORPUS) and all(k in bc.ENTRIES for k in T.CORPUS)
    for name in ("special_huge", "overflow64"):
        assert np.abs(bc.make(name)["vertices"]["position"]).max() > 2.0 ** 40
    assert np.isnan(bc.make("special_nan")["vertices"]["position"]).any()
