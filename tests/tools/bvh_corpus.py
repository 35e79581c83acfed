"""A deterministic corpus of triangle soups for the BVH builders, and a census of the trees they give.

The device builder (csrc/bvh_build_device.hip) sorts nodes into nine classes by triangle count and splits each class with its own
kernel; the host builder (csrc/bvh_build.cpp) and the oracle (oracle/pt_oracle.c) restate the reference's BVH::build.  Random soups
reach only the middle of every class: balanced splits, leaves of at most four triangles, trees of about twenty levels.  The generators
here place inputs where a builder can be wrong without those soups noticing -- a node that refuses to split, a split that peels off
one triangle, a root exactly at a class edge, a child count exactly on a chunk edge, a tree taller than one renumbering run -- and
`census` reads off a reference tree which of those a soup really reached, so tests/test_bvh_corpus.py can hold the corpus to its
purpose on the CPU before tests/test_gpu_bvh_corpus.py holds the device builder to the corpus.

Every generator is seeded and returns float32 vertex positions of shape (n, 3, 3); `triangles` turns them into TRIANGLE records whose
other fields name the input index, so two copies of one triangle still differ in their bytes and a wrong order among them shows.
`soup` / `apply_mode` are also what tests/tools/soak_bvh_device.py draws from: one statement of those distributions."""
import numpy as np

CLASSES = ("SUB", "TINY", "G16", "G32", "W64", "W128", "W512", "W2048", "BIG")
CLASS_EDGES = (4, 8, 16, 32, 64, 128, 512, 2048)    # the largest triangle count of each class but BIG
CHUNK = 8192                                        # a BIG node is split by one workgroup per CHUNK triangles
SUB_MAX = 4                                         # a node this small is finished, subtree and all, by one thread: its descendants are not levels of the builder's loop
RUN_LEVELS, RUN_NODES = 32, 4096                    # the renumbering takes up to RUN_LEVELS consecutive levels of at most RUN_NODES nodes in one launch
HOST_TASK_MIN = 1 << 15                             # the host builder hands subtrees this large to threads
ROOT_SIZES = tuple(s for e in CLASS_EDGES for s in (e, e + 1)) + (CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1)


def class_of(n):
    """The device builder's class of a node with n triangles.  A restatement of `node_class` (and the header comment) of
    csrc/bvh_build_device.hip, kept here so the corpus can be judged on the CPU: EDIT IT TOGETHER WITH node_class."""
    if n > 2048:
        return "BIG"
    if n > 512:
        return "W2048"
    if n > 128:
        return "W512"
    if n > 64:
        return "W128"
    if n > 32:
        return "W64"
    if n > 16:
        return "G32"
    if n > 8:
        return "G16"
    return "TINY" if n > 4 else "SUB"


def triangles(pos):
    """TRIANGLE records for positions (n, 3, 3).  tex_coord_x of the three corners carries the input index (exact in f32 at these sizes)."""
    from rust_ray_tracing_amd import TRIANGLE
    pos = np.asarray(pos, dtype=np.float32)
    t = np.zeros(len(pos), dtype=TRIANGLE)
    t["vertices"]["position"] = pos
    t["vertices"]["tex_coord_x"] = np.arange(len(pos), dtype=np.float32)[:, None]
    return t


def canon(nodes):
    """Node array as bytes with the sign of a zero bound dropped: f32::min(+0, -0) may return either, and no slab test can tell."""
    from rust_ray_tracing_amd import NODE
    n = np.ascontiguousarray(nodes).view(NODE).reshape(-1).copy()
    for k in ("bounds_min", "bounds_max"):
        n[k] = n[k] + np.float32(0.0)
    return n.tobytes()


# ---- the census ---------------------------------------------------------------------------------------------------------------------
def census(nodes, tris=None):
    """What a reference node array (BVH::build's order: children after their parent, side by side) holds.  Returns a dict:
      levels, widths             number of levels and nodes per level of the whole tree
      build_levels, build_widths the same for the nodes the device builder's level loop places: the root and the children of nodes with
                                 more than SUB_MAX triangles (smaller nodes are finished by one thread and never become a level)
      count, depth, parent       per node: triangles below it, level, parent index (-1 for the root)
      inner                      int array (m, 3): node index, k, n - k of every inner node (class_of(k + n - k) is its class)
      leaves                     int array (l, 2): node index, triangle count of every leaf
    and, given the reference's reordered triangles,
      usable                     bool (m, 3): axes of an inner node whose centroid range is not a point (bvh.rs:78)
      decides                    bool (m, 3): axes on which every centroid of the left child is below every centroid of the right one"""
    from rust_ray_tracing_amd import NODE
    nd = np.ascontiguousarray(nodes).view(NODE).reshape(-1)
    n_nodes = len(nd)
    num, child = nd["num_tris"].tolist(), nd["first_tri_or_child"].tolist()
    count, first, depth, parent = list(num), list(child), [0] * n_nodes, [-1] * n_nodes
    for i in range(n_nodes - 1, -1, -1):                   # children sit behind their parent
        if num[i] == 0:
            l = child[i]
            count[i] = count[l] + count[l + 1]
            first[i] = first[l]
    for i in range(n_nodes):
        if num[i] == 0:
            l = child[i]
            depth[l] = depth[l + 1] = depth[i] + 1
            parent[l] = parent[l + 1] = i
    count, first, depth, parent = (np.array(a, dtype=np.int64) for a in (count, first, depth, parent))
    is_inner = nd["num_tris"] == 0
    ii = np.flatnonzero(is_inner)
    left = nd["first_tri_or_child"][ii].astype(np.int64)
    out = dict(levels=int(depth.max()) + 1, widths=np.bincount(depth), count=count, depth=depth, parent=parent,
               inner=np.stack([ii, count[left], count[left + 1]], axis=1) if len(ii) else np.zeros((0, 3), np.int64),
               leaves=np.stack([np.flatnonzero(~is_inner), count[~is_inner]], axis=1))
    placed = np.ones(n_nodes, dtype=bool)
    placed[1:] = count[parent[1:]] > SUB_MAX
    for i in range(1, n_nodes):                            # below a finished subtree nothing is placed (parents come first)
        placed[i] = placed[i] and placed[parent[i]]
    out["build_widths"] = np.bincount(depth[placed])
    out["build_levels"] = len(out["build_widths"])
    if tris is not None and len(ii):
        p = tris["vertices"]["position"]
        c = (np.fmin.reduce(p, axis=1) + np.fmax.reduce(p, axis=1)) / np.float32(2.0)      # scene.rs:114-126, in f32
        c = np.concatenate([c, c[-1:]])                                                     # reduceat wants every index inside
        span = np.stack([first, first + count], axis=1).reshape(-1)
        cmin, cmax = np.fmin.reduceat(c, span, axis=0)[::2], np.fmax.reduceat(c, span, axis=0)[::2]
        out["usable"] = cmin[ii] != cmax[ii]
        out["decides"] = cmax[left] < cmin[left + 1]
    return out


def describe(cen, index):
    """One line about node `index` of a censused tree, for a failure message: which class's kernel made it."""
    if index >= len(cen["count"]):
        return f"node {index} is past the reference's {len(cen['count'])} nodes"
    par = int(cen["parent"][index])
    me = f"node {index} (level {int(cen['depth'][index])}, {int(cen['count'][index])} triangles, class {class_of(int(cen['count'][index]))})"
    if par < 0:
        return me + " is the root"
    row = cen["inner"][np.searchsorted(cen["inner"][:, 0], par)]
    return me + f" is a child of node {par}, class {class_of(int(row[1] + row[2]))}, split (k, n - k) = ({int(row[1])}, {int(row[2])})"


# ---- the soak's distributions ---------------------------------------------------------------------------------------------------------
MODES = ("plain", "ties", "flat", "copies", "zero_area")


def soup(rng, n, scale=1.0, spread=1.0):
    """Gaussian centroids (sigma scale * spread), Gaussian corners around them with a per-triangle size up to `scale`.  float64."""
    return rng.standard_normal((n, 1, 3)) * scale * spread + rng.standard_normal((n, 3, 3)) * scale * rng.random((n, 1, 1))


def apply_mode(rng, p, mode, scale=1.0):
    """The soak's five modes, on a float64 soup `p` (changed in place where the mode allows, and returned):
       0 plain;  1 coordinates quantised to scale / 2: ties in every `<`, identical centroids;  2 one axis constant: an axis the
       builder must skip;  3 about 30 % of the triangles are copies of triangle 0;  4 zero-area triangles (two corners coincide)."""
    n = len(p)
    if mode == 1:
        p = np.round(p / scale * 2) * scale / 2
    if mode == 2:
        p[:, :, int(rng.integers(0, 3))] = 0.25 * scale
    if mode == 3:
        p[rng.random(n) < 0.3] = p[0]
    if mode == 4:
        p[:, 1] = p[:, 0]
    return p


# ---- generators ---------------------------------------------------------------------------------------------------------------------
def at_size(n, mode, seed=0):
    """A soup of exactly n triangles in one of the soak's modes: the ROOT sits at a chosen size, for the class edges (4|5 ... 2 048|2 049)
    and the chunk edges (8 192|8 193, 16 384|16 385), where a lane's slot count, a group's width or a chunk's tail changes."""
    rng = np.random.default_rng([seed, n, mode])
    return apply_mode(rng, soup(rng, n), mode).astype(np.float32)


def _small_tris(rng, c, size):
    """Triangles of about `size` around float64 centroids c (n, 3)."""
    return (c[:, None, :] + rng.uniform(-1.0, 1.0, (len(c), 3, 3)) * size).astype(np.float32)


def _rest(rng, count, far=1000.0):
    """`count` small triangles far out on +x, `far` apart: the separable remainder that makes a bunch arrive as a child."""
    c = np.stack([far * (1.0 + np.arange(count)), rng.uniform(-1, 1, count), rng.uniform(-1, 1, count)], axis=1)
    return _small_tris(rng, c, 0.1)


def bunch(m, vary=(), stop="axes", rest=5, seed=0):
    """m triangles no builder may split, plus `rest` separable ones, shuffled.  The root splits the remainder off, so the bunch reaches
    the class of m as a CHILD and must come out as one leaf of m triangles.
      stop="axes", vary=():  bounds midpoints bit-identical on all three axes, extents all different: every axis is skipped (bvh.rs:78).
      stop="axes", vary=(a,) or (a, b): the midpoints differ on those axes only (by exact steps of 1/64): the bunch is an inner node with
                             one or two axes unusable, and the binned planes of a later axis have to decide.
      stop="cost":           midpoints two ulps apart on x inside boxes 2^-6 wide there and 2^20 wide on y and z: every child box has the
                             parent's area (2^40: the thin axis's share is below half an ulp of it), the 7 candidate costs equal the parent's
                             exactly, and `best_cost >= parent_cost` (bvh.rs:94) keeps the leaf although the partition would split."""
    rng = np.random.default_rng([seed, m, len(vary), stop == "cost"])
    i = np.arange(m, dtype=np.float64)
    lo, hi = np.zeros((m, 3)), np.zeros((m, 3))
    if stop == "axes":
        centre, half = np.array([2.0, 3.0, 5.0]), 0.5 + i / 4096.0           # every corner a multiple of 2^-12 below 64: exact in f32
        for a in range(3):
            mid = centre[a] + (rng.permutation(m) / 64.0 if a in vary else 0.0)
            lo[:, a], hi[:, a] = mid - half, mid + half
    else:
        mid = 1.0 + i * 2.0 ** -22
        lo[:, 0], hi[:, 0] = mid - 2.0 ** -7, mid + 2.0 ** -7
        lo[:, 1:], hi[:, 1:] = -2.0 ** 19, 2.0 ** 19
    p = np.stack([np.stack([lo[:, 0], lo[:, 1], lo[:, 2]], 1), np.stack([hi[:, 0], hi[:, 1], lo[:, 2]], 1),
                  np.stack([lo[:, 0], hi[:, 1], hi[:, 2]], 1)], axis=1).astype(np.float32)
    p = np.concatenate([p, _rest(rng, rest)])
    return p[rng.permutation(len(p))]


def outlier(n, side, axis=0, seed=0):
    """n - 1 small triangles in a unit cube and one 1 000 away on `axis`, below (side="lo": the split has k = 1) or above ("hi":
    n - k = 1): the closed-form partition with one element on a side, a lone hole or no hole at all."""
    rng = np.random.default_rng([seed, n, side == "hi", axis])
    c = rng.uniform(0.0, 1.0, (n, 3))
    c[int(rng.integers(0, n)), axis] = -1000.0 if side == "lo" else 1000.0
    return _small_tris(rng, c, 0.02)


def clusters(sizes, axis=0, gap=100.0, seed=0):
    """Unit-cube clusters of the given sizes, `gap` apart along `axis`, shuffled.  With two clusters every candidate plane falls in the gap,
    the first one wins and the root's k is sizes[0] -- told, not drawn: exactly on a chunk edge (8 192 of 16 384, 8 192 of 8 193), one
    off it, or an even split of any class."""
    rng = np.random.default_rng([seed, axis] + list(sizes))
    c = rng.uniform(0.0, 1.0, (sum(sizes), 3))
    c[:, axis] += np.repeat(np.arange(len(sizes)) * gap, sizes)
    return _small_tris(rng, c, 0.02)[rng.permutation(len(c))]


def chain(n, decades, axis=0, seed=0, lo=1.0):
    """Centroids in geometric progression over `decades` decades along `axis` (from `lo` up), triangle size and the other two coordinates
    in proportion, shuffled.  The surface-area heuristic keeps cutting the sparse far end off, so the tree is a tall stack of narrow
    levels: more than one renumbering run of RUN_LEVELS levels, with dfs / base / size handed from run to run.  axis = 1 or 2 turns the
    long axis, so the axis-major / plane-minor choice is not always made on axis 0."""
    rng = np.random.default_rng([seed, n, int(decades), axis])
    x = lo * 10.0 ** (decades * (np.arange(n) + 0.5) / n)
    c = rng.uniform(-0.01, 0.01, (n, 3)) * x[:, None]
    c[:, axis] = x
    p = (c[:, None, :] + rng.uniform(-1.0, 1.0, (n, 3, 3)) * (0.002 * x)[:, None, None]).astype(np.float32)
    return p[rng.permutation(n)]


def spiral(m, core, seed=0, ratio=9.0, lo=1e-9):
    """A tree far taller than one renumbering run, from few triangles: a plain soup of `core` triangles shrunk into a cube of side `lo`,
    and 3 m lone triangles at lo * ratio^i (i = 1..m) out on +x, -y and +z.  With ratio >= 9 the outermost triangle of an axis lies
    beyond all seven planes of its axis and everything else below the first, so every level peels ONE triangle off a node that still
    holds the whole core (n - k = 1 on x and z, k = 1 on y, in the class of the core), the three axes take turns by cost, and the tree
    has 3 m levels of two nodes on top of the core's own.  What bounds m: a resident scene refuses a bound beyond 2^40 (include/mipt.h),
    so lo * ratio^m stays below it (1e-9 * 9^22 = 0.98e12 < 1.1e12), and lo itself stays far above the square root of the smallest f32,
    so that no area of the core underflows."""
    rng = np.random.default_rng([seed, m, core])
    c = [rng.uniform(0.0, 1.0, (core, 3)) * lo]
    size = [np.full(core, 0.02 * lo)]
    for axis, sign in ((0, 1.0), (1, -1.0), (2, 1.0)):
        r = lo * ratio ** np.arange(1, m + 1)
        a = rng.uniform(-0.01, 0.01, (m, 3)) * r[:, None]
        a[:, axis] = sign * r
        c.append(a)
        size.append(0.01 * r)
    c, size = np.concatenate(c), np.concatenate(size)
    p = (c[:, None, :] + rng.uniform(-1.0, 1.0, (len(c), 3, 3)) * size[:, None, None]).astype(np.float32)
    return p[rng.permutation(len(p))]


def specials(kind, n=300, seed=0):
    """Soups at the edges of f32:
      "denormal"  x as a plain soup, y and z a few hundred denormal steps (2^-149) wide: every box area and cost is a denormal number
      "zeros"     quantised soup whose zero coordinates carry random signs, and an axis that is +-0.0 throughout: min / max of mixed zeros
                  (the node arrays are compared after `canon`), an unusable axis whose range is [-0.0, +0.0]
      "huge"      two groups around -2^40 and +2^40, where a coordinate step is 2^17
      "overflow"  corners around 3e19: every area is inf, no plane is usable and the split falls back to 0.0 on axis 0 (bvh.rs:94-108)
      "nan"       a plain soup with ONE vertex coordinate NaN: f32::min / max skip it, the triangle keeps the bounds of its other corners"""
    rng = np.random.default_rng([seed, n, sum(map(ord, kind))])
    if kind == "denormal":
        p = soup(rng, n)
        p[:, :, 1:] = rng.integers(-400, 400, (n, 3, 2)) * 2.0 ** -149
        return p.astype(np.float32)
    if kind == "zeros":
        p = apply_mode(rng, soup(rng, n), 1).astype(np.float32)
        p[:, :, int(rng.integers(0, 3))] = 0.0
        flip = (p == 0.0) & (rng.random(p.shape) < 0.5)
        p[flip] = np.float32(-0.0)
        return p
    if kind == "huge":
        return (soup(rng, n, 2.0 ** 20, 4.0) + rng.choice([-2.0 ** 40, 2.0 ** 40], (n, 1, 1))).astype(np.float32)
    if kind == "overflow":
        return (rng.standard_normal((n, 1, 3)) * 3e19 + rng.standard_normal((n, 3, 3)) * 1e18).astype(np.float32)
    if kind == "nan":
        p = soup(rng, n).astype(np.float32)
        p[n // 3, 1, 2] = np.nan
        return p
    raise ValueError(kind)


# ---- the corpus ---------------------------------------------------------------------------------------------------------------------
def _entries():
    e = {}
    for s in ROOT_SIZES:                                         # every root size in every mode up to 2 049; the chunk edges in two modes each
        for mode in (range(5) if s <= 2049 else ((s % 5), (s + 2) % 5)):
            e[f"size{s}_{MODES[mode]}"] = (at_size, (s, mode))
    ms = (6, 12, 24, 48, 100, 300, 1000, 3000)                   # one size inside each class above SUB
    for m in ms:
        e[f"bunch{m}"] = (bunch, (m,))
        e[f"bunch{m}_cost"] = (bunch, (m, (), "cost"))
        e[f"bunch{m}_z"] = (bunch, (m, (2,)))
        e[f"bunch{m}_yz"] = (bunch, (m, (1, 2)))
        e[f"outlier{m}_lo"] = (outlier, (m, "lo"))
        e[f"outlier{m}_hi"] = (outlier, (m, "hi", m % 3))
        e[f"halves{m}"] = (clusters, ((m // 2, m - m // 2), m % 3))
    e["bunch300_y"] = (bunch, (300, (1,)))
    e["outlier3_lo"] = (outlier, (3, "lo"))
    e["outlier3_hi"] = (outlier, (3, "hi"))
    e["outlier9000_lo"] = (outlier, (9000, "lo", 1))               # one-sided splits of a node of more than one chunk
    e["outlier20000_hi"] = (outlier, (20000, "hi", 2))
    e["chunk_8192_of_16384"] = (clusters, ((CHUNK, CHUNK),))
    e["chunk_8192_of_8193"] = (clusters, ((CHUNK, 1),))
    e["chunk_8193_then_8191"] = (clusters, ((CHUNK + 1, CHUNK - 1), 1))
    e["chunk_8191_then_3000"] = (clusters, ((CHUNK - 1, 3000), 2))
    e["chunk_three"] = (clusters, ((CHUNK, 2 * CHUNK, CHUNK + 1),))
    e["spiral"] = (spiral, (22, 5000))                           # 66 levels of two nodes whose parent is BIG, then the core's
    e["spiral_small"] = (spiral, (12, 40))
    e["chain_x"] = (chain, (8000, 6))
    e["chain_y"] = (chain, (3000, 4, 1))
    e["chain_z"] = (chain, (3000, 4, 2))
    e["wide"] = (at_size, (45000, 0))                            # past the host's threading threshold; a level wider than a run takes
    for kind in ("denormal", "zeros", "huge", "nan"):
        e[f"special_{kind}"] = (specials, (kind,))
    e["special_zeros_big"] = (specials, ("zeros", 9000))
    for s in (5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 512, 513, 2048, 2049):
        e[f"overflow{s}"] = (specials, ("overflow", s))
    return e


ENTRIES = _entries()
# the GPU file's second and third passes: one leaf case per class, the chunk edges, the deep chains
RESIDENT = tuple(f"bunch{m}" for m in (6, 12, 24, 48, 100, 300, 1000, 3000)) + ("bunch3000_cost", "chunk_8192_of_16384", "chunk_8192_of_8193",
                                                                              "chunk_8193_then_8191", "spiral", "chain_x", "chain_y")
REBUILD = ("spiral", "chunk_8192_of_16384", "bunch300")


# ---- past the caps --------------------------------------------------------------------------------------------------------------------
# Four entries whose trees take the loops of the device builder and of the layout kernels (csrc/scene_device.hip) on their second
# trip: grid-stride loops over capped grids, big_scan's steps of BIG_SCAN_STEP chunks, big_setup's strips of BIG_SETUP_STRIP nodes.
# The oracle needs 23 s and more for one of them, so their reference is the host builder (`reference_host`), which
# tests/test_bvh_corpus.py holds to the oracle on the smallest and to itself with one thread on the others; the same file asserts on
# the host trees that every entry reaches what it is here for (DESIGN section 21 names the launch each one passes).
BIG_SCAN_STEP = 64                                  # chunks of a BIG node that big_scan takes per step, with the prefix carried on
BIG_SETUP_STRIP = 1024                              # BIG nodes of one level that big_setup takes per strip, with the chunk count carried on
GRID_2048 = 2048 * 256                              # threads of make_proxies, extract_order, sizes_level, bases_level, write_new_of, write_pairs
GRID_4096 = 4096 * 256                              # ... of write_tris (gather_tris: seven 16-byte pieces per triangle over as many)
GRID_1024 = 1024 * 256                              # ... of check_nodes, append_lone
SCAN_ONE_TRIP = 512 * 256                           # the layout's scans (kScanGrid workgroups of 256): up to this many elements every workgroup
                                                    # takes one tile; past it the workgroups loop and carry their prefix from tile to tile
LARGE_CLUSTERS = 1600                               # clusters of 2 049 in `large_clusters`

LARGE = {
    "large_soup": (at_size, (70 * CHUNK + 1234, 0)),                         # a root of 71 chunks; more pair records than GRID_2048
    "large_halves": (clusters, ((66 * CHUNK + 5, 65 * CHUNK - 3),)),          # a root of 132 chunks over two children past BIG_SCAN_STEP
    "large_edge": (clusters, ((64 * CHUNK, 64 * CHUNK + 1),)),                # 2^20 + 1 triangles; the root's k lies on big_scan's step edge
    "large_clusters": (clusters, ((2049,) * LARGE_CLUSTERS,)),                # more BIG nodes in a level than BIG_SETUP_STRIP
}
LATE_LEAF = 48                                      # triangles of the one large leaf of `late_leaf`


def late_leaf(n=140000, m=LATE_LEAF, seed=0):
    """A plain soup of n triangles around x = -50 000 and, where `bunch` puts them, m triangles no builder may split plus 5 lone ones.
    Every plane of the root falls between the two groups, so the soup is the root's left child and fills the node array up to about
    2 n; the leaf of m comes behind it, past the GRID_1024 nodes that check_nodes' grid takes in its first trip, and every leaf before
    it holds at most four triangles: the largest leaf is found in the second trip or not at all."""
    rng = np.random.default_rng([seed, n, m])
    p = soup(rng, n)
    p[:, :, 0] -= 50000.0
    p = np.concatenate([p.astype(np.float32), bunch(m, seed=seed)])
    return p[rng.permutation(len(p))]


LARGE_RESIDENT = ("large_soup", "large_halves", "large_clusters")            # through the resident setup, tree and layout
LARGE_REBUILD = ("large_soup",)


def make(name):
    """The corpus entry `name` (of ENTRIES or LARGE, or "late_leaf") as TRIANGLE records in input order."""
    fn, args = (late_leaf, ()) if name == "late_leaf" else ENTRIES[name] if name in ENTRIES else LARGE[name]
    return triangles(fn(*args))


_reference = {}


def reference(orc, name):
    """(input triangles, the oracle's reordered triangles, the oracle's node array) of entry `name`; built once, never changed."""
    if name not in _reference:
        tris = make(name)
        ref_tris, ref_nodes = orc.bvh_build(tris)
        for a in (tris, ref_tris, ref_nodes):
            a.setflags(write=False)
        _reference[name] = (tris, ref_tris, ref_nodes)
    return _reference[name]


_reference_host = {}
reference_host_seconds = {}                         # name -> (generation, host build): what the first test to ask for an entry paid


def reference_host(rrt, name):
    """(input triangles, the HOST builder's reordered triangles, its node array) of entry `name`, with the default thread count; built
    once, never changed.  The reference of the LARGE entries, for which the oracle is too slow."""
    if name not in _reference_host:
        import time
        t0 = time.perf_counter()
        tris = make(name)
        t1 = time.perf_counter()
        sc = rrt.Scene.from_arrays(tris, [rrt.material_default()])
        reference_host_seconds[name] = (t1 - t0, time.perf_counter() - t1)
        out = (tris, sc.tris, sc.bvh_nodes)
        for a in out:
            a.setflags(write=False)
        _reference_host[name] = out
    return _reference_host[name]


_census_host = {}


def census_host(rrt, name):
    """The census of `reference_host`'s tree: a Python loop over the nodes (seconds at these sizes), so made once per entry."""
    if name not in _census_host:
        _census_host[name] = census(reference_host(rrt, name)[2])
    return _census_host[name]


def first_difference(nodes, ref_nodes):
    """Index of the first node whose canonical bytes differ (the shorter array's length if one is a prefix of the other), or None."""
    a = np.frombuffer(canon(nodes), dtype=np.uint8).reshape(-1, 32)
    b = np.frombuffer(canon(ref_nodes), dtype=np.uint8).reshape(-1, 32)
    m = min(len(a), len(b))
    bad = np.flatnonzero((a[:m] != b[:m]).any(axis=1))
    if len(bad):
        return int(bad[0])
    return None if len(a) == len(b) else m
