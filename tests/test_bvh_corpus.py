"""CPU: the BVH corpus (tests/tools/bvh_corpus.py) against the oracle, and the corpus against its own purpose.

1. For every entry the host builder (mipt_bvh_build) equals the oracle's restatement of BVH::build byte for byte -- node array (sign of
   a zero bound aside) and triangle order; entries past the host builder's threading threshold also with 1 and 7 threads.
2. The census of the ORACLE's trees meets the conditions the corpus exists for: every class of the device builder as a parent with
   k = 1, with n - k = 1 and with an even split, every class as a leaf that is not the root, roots at every class and chunk edge, child
   counts on and next to a chunk edge, a tree taller than two renumbering runs, a wide level between runs, nodes with a single usable
   axis, planes deciding on axis 1 and on axis 2.  These are conditions on the INPUTS: a generator edited so that a case is lost fails
   here, on the CPU, before tests/test_gpu_bvh_corpus.py would silently check less.
3. The LARGE entries (574 674 to 3.4 M triangles, past the caps of the device builder's and the layout's launches) have the HOST
   builder as their reference on the GPU, because the oracle takes 23 s and more for one of them.  Here the host builder is held to
   the oracle on the smallest, to itself with one thread on two more, and the census of the host trees meets the conditions each
   entry exists for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import bvh_corpus as bc  # noqa: E402

NAMES = list(bc.ENTRIES)


def _host(rrt, tris, threads=0):
    sc = rrt.Scene.from_arrays(tris, [rrt.material_default()], threads=threads)
    return sc.tris, sc.bvh_nodes


def _assert_same(tris, nodes, ref_tris, ref_nodes, what):
    bad = bc.first_difference(nodes, ref_nodes)
    if bad is not None:
        raise AssertionError(f"{what}: node arrays differ first at {bc.describe(bc.census(ref_nodes), bad)}")
    assert tris.tobytes() == ref_tris.tobytes(), f"{what}: same nodes, other triangle order"


@pytest.mark.parametrize("name", NAMES)
def test_host_builder_matches_oracle(rrt, orc, name):
    tris, ref_tris, ref_nodes = bc.reference(orc, name)
    _assert_same(*_host(rrt, tris), ref_tris, ref_nodes, name)
    if len(tris) >= bc.HOST_TASK_MIN:
        for threads in (1, 7):
            _assert_same(*_host(rrt, tris, threads), ref_tris, ref_nodes, f"{name}, {threads} threads")


def test_sizes(orc):
    sizes = {n: len(bc.reference(orc, n)[0]) for n in NAMES}
    assert max(sizes.values()) <= 50000
    assert sizes["wide"] >= bc.HOST_TASK_MIN and sizes["chunk_three"] >= bc.HOST_TASK_MIN      # the host builder's threads get work


def test_subsets_name_corpus_entries():
    assert set(bc.REBUILD) <= set(bc.RESIDENT) <= set(bc.ENTRIES)
    for name in bc.RESIDENT:                                   # a resident scene refuses a bound that is not finite or lies beyond 2^40
        p = bc.make(name)["vertices"]["position"]
        assert np.isfinite(p).all() and np.abs(p).max() < 2.0 ** 40, name


def test_class_of_edges():
    assert [bc.class_of(n) for n in (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 512, 513, 2048, 2049, 50000)] == \
        ["SUB", "SUB", "TINY", "TINY", "G16", "G16", "G32", "G32", "W64", "W64", "W128", "W128", "W512", "W512", "W2048", "W2048", "BIG", "BIG"]
    assert sorted(set(bc.class_of(n) for n in range(1, 3000))) == sorted(bc.CLASSES)


@pytest.fixture(scope="module")
def corpus(orc):
    """name -> census of the oracle's tree, for the whole corpus"""
    out = {}
    for name in NAMES:
        _, ref_tris, ref_nodes = bc.reference(orc, name)
        out[name] = bc.census(ref_nodes, ref_tris)
    return out


def _parents(rows):
    """class index, k, n - k, n of rows (k, n - k)"""
    n = rows.sum(axis=1)
    edges = np.array(bc.CLASS_EDGES)
    cls = np.searchsorted(edges, n, side="left")                 # n <= 4 -> 0 (SUB) ... n > 2 048 -> 8 (BIG)
    return cls, rows[:, 0], rows[:, 1], n


def test_census_splits(corpus):
    rows = np.concatenate([c["inner"][:, 1:] for c in corpus.values()])
    cls, k, r, n = _parents(rows)
    assert all(bc.class_of(int(x)) == bc.CLASSES[int(c)] for x, c in zip(n[:: max(1, len(n) // 5000)], cls[:: max(1, len(n) // 5000)]))
    for ci, cname in enumerate(bc.CLASSES):
        m = cls == ci
        assert (k[m] == 1).any(), f"no {cname} parent with k = 1"
        assert (r[m] == 1).any(), f"no {cname} parent with n - k = 1"
        assert (np.minimum(k[m], r[m]) / n[m] >= 0.3).any(), f"no {cname} parent with an even split"
    # in BIG, where the partition spans chunks, the one-sided splits have to come with more than one chunk too
    big = n > bc.CHUNK
    assert ((k == 1) & big).any() and ((r == 1) & big).any()


def test_census_leaves(corpus, orc):
    from rust_ray_tracing_amd import NODE
    seen = set()
    for c in corpus.values():
        lv = c["leaves"]
        lv = lv[lv[:, 0] != 0]
        seen |= {bc.class_of(int(x)) for x in np.unique(lv[:, 1])}
    assert seen == set(bc.CLASSES), f"no leaf below the root in {sorted(set(bc.CLASSES) - seen)}"
    # one leaf per class above SUB for each way of refusing: every axis skipped (bunchM) and best_cost >= parent_cost (bunchM_cost)
    for m in (6, 12, 24, 48, 100, 300, 1000, 3000):
        for name in (f"bunch{m}", f"bunch{m}_cost"):
            lv = corpus[name]["leaves"]
            assert ((lv[:, 1] == m) & (lv[:, 0] != 0)).any(), f"{name}: the bunch is not one leaf of {m} below the root"
    # the cost case is refused by the cost alone: its axis 0 is usable and its partition would split
    _, ref_tris, _ = bc.reference(orc, "bunch300_cost")
    c = corpus["bunch300_cost"]
    leaf = int(c["leaves"][c["leaves"][:, 1] == 300][0, 0])
    first = int(np.ascontiguousarray(bc.reference(orc, "bunch300_cost")[2]).view(NODE).reshape(-1)[leaf]["first_tri_or_child"])
    x = ref_tris["vertices"]["position"][first: first + 300, :, 0]
    assert len(np.unique((x.min(axis=1) + x.max(axis=1)) / np.float32(2))) == 300


def test_census_root_sizes(corpus):
    roots = {int(c["count"][0]) for c in corpus.values()}
    assert set(bc.ROOT_SIZES) <= roots, sorted(set(bc.ROOT_SIZES) - roots)
    assert bc.ROOT_SIZES == (4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 512, 513, 2048, 2049, 8192, 8193, 16384, 16385)


def test_census_chunk_edges(corpus):
    rows = np.concatenate([c["inner"][:, 1:] for c in corpus.values()])
    k, n = rows[:, 0], rows.sum(axis=1)
    big = n > 2048
    assert (big & (k % bc.CHUNK == 0)).any(), "no BIG parent with k on a chunk edge"
    assert (big & (k > 1) & (k % bc.CHUNK == 1)).any() and (big & (k % bc.CHUNK == bc.CHUNK - 1)).any(), "no BIG parent with k next to a chunk edge"
    # and as told: 8 192 of 16 384, 8 192 of 8 193
    assert tuple(corpus["chunk_8192_of_16384"]["inner"][0][1:]) == (8192, 8192)
    assert tuple(corpus["chunk_8192_of_8193"]["inner"][0][1:]) == (8192, 1)
    assert tuple(corpus["chunk_8193_then_8191"]["inner"][0][1:]) == (8193, 8191)
    assert tuple(corpus["chunk_8191_then_3000"]["inner"][0][1:]) == (8191, 3000)


def test_census_deep_tree(corpus):
    """more than 2 x 32 levels of at most 4 096 nodes, counted in the levels the device builder's loop really has"""
    c = corpus["spiral"]
    assert c["build_levels"] >= 2 * bc.RUN_LEVELS + 1 and c["levels"] >= c["build_levels"] and c["build_widths"].max() <= bc.RUN_NODES
    assert corpus["spiral_small"]["build_levels"] > bc.RUN_LEVELS and corpus["spiral_small"]["build_widths"].max() <= bc.RUN_NODES
    assert int(c["count"][0]) <= 50000


def test_census_wide_level_between_runs(corpus):
    found = []
    for name, c in corpus.items():
        wide = np.flatnonzero(c["build_widths"] > bc.RUN_NODES)
        if len(wide) and wide[0] > 0 and wide[-1] < c["build_levels"] - 1:
            found.append(name)
    assert "wide" in found and "chunk_three" in found, found


def test_census_axes(corpus):
    one_axis, axis1, axis2 = [], [], []
    for name, c in corpus.items():
        if "usable" not in c:
            continue
        u, d = c["usable"], c["decides"]
        n = c["inner"][:, 1] + c["inner"][:, 2]
        if ((u.sum(axis=1) == 1) & (n > bc.SUB_MAX)).any():
            one_axis.append(name)
        contested = (u.sum(axis=1) >= 2) & (n > bc.SUB_MAX)
        if (contested & d[:, 1] & ~d[:, 0] & ~d[:, 2]).any():
            axis1.append(name)
        if (contested & d[:, 2] & ~d[:, 0] & ~d[:, 1]).any():
            axis2.append(name)
    for m in (6, 12, 24, 48, 100, 300, 1000, 3000):
        assert f"bunch{m}_z" in one_axis, (m, one_axis)               # a node of every class with axes 0 and 1 unusable
    assert "bunch300_y" in one_axis
    assert "chain_y" in axis1 and "chain_z" in axis2, (axis1, axis2)
    assert "bunch300_yz" in axis1 or "bunch300_yz" in axis2


# ---- the LARGE entries: the host builder as the GPU file's reference, and what its trees reach ----------------------------------------
LARGE = list(bc.LARGE)


def test_large_host_builder_matches_oracle(rrt, orc):
    """The host builder equals the oracle on `large_soup`, 574 674 triangles.  One entry only: the oracle's build of it takes about
    23 s, and 40 s and more for each of the other three, which are therefore held to the host builder with one thread instead
    (below) -- the single-threaded build is the plain recursion, the default one hands subtrees to threads."""
    tris, ref_tris, ref_nodes = bc.reference(orc, "large_soup")
    _, host_tris, host_nodes = bc.reference_host(rrt, "large_soup")
    _assert_same(host_tris, host_nodes, ref_tris, ref_nodes, "large_soup")


@pytest.mark.parametrize("name", ["large_halves", "large_edge"])
def test_large_host_builder_one_thread(rrt, name):
    tris, ref_tris, ref_nodes = bc.reference_host(rrt, name)
    _assert_same(*_host(rrt, tris, 1), ref_tris, ref_nodes, f"{name}, 1 thread against the default")


def test_large_positions(rrt):
    """what test_subsets_name_corpus_entries asks of a resident scene's input"""
    assert set(bc.LARGE_REBUILD) <= set(bc.LARGE_RESIDENT) <= set(bc.LARGE) and not set(bc.LARGE) & set(bc.ENTRIES)
    for name in LARGE + ["late_leaf"]:
        p = bc.reference_host(rrt, name)[0]["vertices"]["position"]
        assert np.isfinite(p).all() and np.abs(p).max() < 2.0 ** 40, name


def test_late_leaf(rrt, orc):
    """`late_leaf`, for check_nodes' second trip: host builder == oracle (140 053 triangles), and the one leaf above four triangles
    is a node past the first trip of that grid."""
    tris, ref_tris, ref_nodes = bc.reference(orc, "late_leaf")
    _, host_tris, host_nodes = bc.reference_host(rrt, "late_leaf")
    _assert_same(host_tris, host_nodes, ref_tris, ref_nodes, "late_leaf")
    lv = bc.census_host(rrt, "late_leaf")["leaves"]
    above = lv[lv[:, 1] > bc.SUB_MAX]
    assert len(above) == 1 and above[0, 1] == bc.LATE_LEAF and above[0, 0] >= bc.GRID_1024, above


@pytest.fixture(scope="module")
def large(rrt):
    """name -> census of the HOST builder's tree"""
    return {name: bc.census_host(rrt, name) for name in LARGE}


def _chunks(n):
    return -(-int(n) // bc.CHUNK)


def _lone_pairs(rrt, nodes):
    """A lower bound of the number of mate-less pair records (what append_lone copies) in the host restatement of the record order:
    they are the order's tail, every one a pair of two leaves, and they start on an even record."""
    import ctypes as C
    nodes = np.ascontiguousarray(nodes)
    out = np.zeros(len(nodes) + 1, dtype=np.uint32)
    n = C.c_uint32(0)
    assert rrt.load_diag().mipt_internal_pair_order(nodes.ctypes.data, len(nodes), out.ctypes.data, out.size, C.byref(n)) == 0
    order = out[: n.value]
    pad = order == 0xffffffff
    k = np.where(pad, 0, order).astype(np.int64)
    two_leaves = (nodes["num_tris"][2 * k + 1] > 0) & (nodes["num_tris"][2 * k + 2] > 0) & ~pad
    other = np.flatnonzero(~two_leaves)
    start = int(other[-1]) + 1 if len(other) else 0
    return len(order) - (start + (start & 1))


def test_large_census(rrt, large):
    """Conditions on the inputs, by the launch they are for.  Not measurements: an edited generator fails here."""
    for name in LARGE:                                          # make_proxies, extract_order, gather_tris, check_nodes; the scans over triangles and pairs
        c = large[name]
        assert c["count"][0] > bc.GRID_2048 and len(c["count"]) > bc.GRID_1024 and len(c["inner"]) > bc.SCAN_ONE_TRIP, name
    c = large["large_soup"]                                     # big_scan: one node of more than a step; write_new_of, write_pairs
    assert _chunks(c["count"][0]) >= bc.BIG_SCAN_STEP + 1
    assert len(c["inner"]) > bc.GRID_2048
    c = large["large_halves"]                                   # big_scan: three steps, and two nodes of two steps side by side; write_tris
    assert _chunks(c["count"][0]) >= 2 * bc.BIG_SCAN_STEP + 1
    assert _chunks(c["count"][1]) >= bc.BIG_SCAN_STEP + 1 and _chunks(c["count"][2]) >= bc.BIG_SCAN_STEP + 1
    assert c["depth"][1] == 1 and c["depth"][2] == 1
    assert c["count"][0] > bc.GRID_4096
    assert np.bincount(c["depth"][c["inner"][:, 0]]).max() > bc.SCAN_ONE_TRIP      # the scan over one level's pairs loops too
    c = large["large_edge"]                                     # big_scan: k on the step edge
    assert c["count"][0] == 2 ** 20 + 1 and _chunks(c["count"][0]) == 2 * bc.BIG_SCAN_STEP + 1
    assert tuple(c["inner"][0]) == (0, bc.BIG_SCAN_STEP * bc.CHUNK, bc.BIG_SCAN_STEP * bc.CHUNK + 1)
    c = large["large_clusters"]                                 # big_setup's second strip; sizes_level, bases_level; append_lone
    big = np.bincount(c["depth"][c["count"] > bc.CLASS_EDGES[-1]])
    assert big.max() >= bc.BIG_SETUP_STRIP + 1 + 64, big        # with room: a few clusters may split otherwise after an edit
    assert c["build_widths"].max() > bc.GRID_2048
    assert _lone_pairs(rrt, bc.reference_host(rrt, "large_clusters")[2]) > bc.GRID_1024
