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
