"""CPU restatement of the REFIT of mipt_scene_update_triangles (csrc/scene_update.hip), for the tests.

The tree keeps its shape; every bound becomes what Node::grow_by_tri (reference src/bvh.rs:185-193) folds over the node's triangles,
starting from Node::default's +-f32::MAX (bvh.rs:174-181), with f32::min / f32::max (a NaN coordinate is ignored).  A leaf folds the
triangles of its range; an inner node is the union of its two children.  Here the nodes are walked from the highest index down --
BVH::build pushes children after their parent (bvh.rs:121,131-132), so a child is always final before its parent -- which is a
different order of work from the device's level-by-level records, and the result must be the same (sign of a zero aside).

`per_node_fold` is the independent check: every node folded directly over all triangles its subtree references."""
import numpy as np

F32_MAX = np.float32(3.4028235e38)


def _tri_boxes(tris):
    pos = np.asarray(tris["vertices"]["position"], dtype=np.float32)
    return np.fmin(np.fmin.reduce(pos, axis=1), F32_MAX), np.fmax(np.fmax.reduce(pos, axis=1), -F32_MAX)


def refit(nodes, tris):
    """nodes with refit bounds; `tris` in the tree's order"""
    out = nodes.copy()
    lo, hi = _tri_boxes(tris)
    for i in range(len(out) - 1, -1, -1):
        n = int(out["num_tris"][i])
        f = int(out["first_tri_or_child"][i])
        if n > 0:
            out["bounds_min"][i] = np.fmin(np.fmin.reduce(lo[f:f + n], axis=0), F32_MAX)
            out["bounds_max"][i] = np.fmax(np.fmax.reduce(hi[f:f + n], axis=0), -F32_MAX)
        else:
            out["bounds_min"][i] = np.fmin(out["bounds_min"][f], out["bounds_min"][f + 1])
            out["bounds_max"][i] = np.fmax(out["bounds_max"][f], out["bounds_max"][f + 1])
    return out


def node_depths(nodes):
    """depth of every node by a breadth-first frontier from node 0 (-1: not reachable from the root)"""
    first, inner = nodes["first_tri_or_child"].astype(np.int64), nodes["num_tris"] == 0
    depth = np.full(len(nodes), -1, dtype=np.int64)
    frontier, d = np.zeros(1, dtype=np.int64), 0
    while frontier.size:
        assert (depth[frontier] == -1).all(), "a node is reached twice"
        depth[frontier] = d
        f = first[frontier[inner[frontier]]]
        frontier, d = np.concatenate([f, f + 1]), d + 1
    return depth


def refit_by_levels(nodes, tris):
    """`refit` without a Python loop over the nodes, for trees of a million triangles: the leaves in one segmented fold (their
    ranges must partition the triangles), then the inner nodes one level at a time from the deepest.  The same fmin / fmax and the
    same +-F32_MAX clamps as `refit`; every node must be reachable from node 0."""
    out = nodes.copy()
    lo, hi = _tri_boxes(tris)
    first, count = out["first_tri_or_child"].astype(np.int64), out["num_tris"].astype(np.int64)
    leaves = np.flatnonzero(count > 0)
    leaves = leaves[np.argsort(first[leaves], kind="stable")]
    start = first[leaves]
    assert start[0] == 0 and np.array_equal(start[1:], start[:-1] + count[leaves[:-1]]) and start[-1] + count[leaves[-1]] == len(tris), \
        "the leaves' ranges do not partition the triangles"
    out["bounds_min"][leaves] = np.fmin(np.fmin.reduceat(lo, start, axis=0), F32_MAX)
    out["bounds_max"][leaves] = np.fmax(np.fmax.reduceat(hi, start, axis=0), -F32_MAX)
    depth = node_depths(out)
    assert (depth >= 0).all(), "a node is not reachable from the root"
    inner = count == 0
    for d in range(int(depth.max()) - 1, -1, -1):
        i = np.flatnonzero(inner & (depth == d))
        f = first[i]
        out["bounds_min"][i] = np.fmin(out["bounds_min"][f], out["bounds_min"][f + 1])
        out["bounds_max"][i] = np.fmax(out["bounds_max"][f], out["bounds_max"][f + 1])
    return out


def subtree_triangles(nodes, i):
    """indices of the triangles the leaves under node i reference"""
    stack, out = [i], []
    while stack:
        k = stack.pop()
        n, f = int(nodes["num_tris"][k]), int(nodes["first_tri_or_child"][k])
        if n > 0:
            out.extend(range(f, f + n))
        else:
            stack.extend((f, f + 1))
    return np.array(out, dtype=np.int64)


def per_node_fold(nodes, tris, which=None):
    """(bounds_min, bounds_max) of the nodes `which` (default all), each folded over its own subtree's triangles"""
    lo, hi = _tri_boxes(tris)
    which = range(len(nodes)) if which is None else which
    mn, mx = [], []
    for i in which:
        t = subtree_triangles(nodes, i)
        mn.append(np.fmin(np.fmin.reduce(lo[t], axis=0), F32_MAX))
        mx.append(np.fmax(np.fmax.reduce(hi[t], axis=0), -F32_MAX))
    return np.array(mn, dtype=np.float32), np.array(mx, dtype=np.float32)


def same_nodes(a, b):
    """equal node arrays; a bound may differ in the sign of a zero (-0.0 == 0.0 compares equal)"""
    return (len(a) == len(b) and np.array_equal(a["first_tri_or_child"], b["first_tri_or_child"]) and np.array_equal(a["num_tris"], b["num_tris"])
            and np.array_equal(a["bounds_min"], b["bounds_min"]) and np.array_equal(a["bounds_max"], b["bounds_max"]))
