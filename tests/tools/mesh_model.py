"""numpy float32 model of the mesh expansion rule (include/mipt.h, "resident indexed meshes") and the helper that turns fat triangles
into an indexed mesh.  Every operator of the rule is its own numpy call on float32 arrays, so nothing is fused and every
intermediate is rounded once -- what mipt_mesh_expand and the expansion kernel must reproduce bit for bit."""
import numpy as np

F = np.float32
PART = np.dtype([("first_tri", "<u4"), ("n_tris", "<u4"), ("material_id", "<u4"), ("reserved", "<u4")])
VERTEX = np.dtype([("position", "<f4", 3), ("tex_coord_x", "<f4"), ("normal", "<f4", 3), ("tex_coord_y", "<f4")])
TRIANGLE = np.dtype([("vertices", VERTEX, 3), ("material_id", "<u4"), ("_pad", "u1", 12)])


def _cross(a, b):                                            # vec3.rs:137-143
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1).astype(F)


def _length(v):                                              # vec3.rs:94-96
    return np.sqrt(((v[..., 0] * v[..., 0]) + (v[..., 1] * v[..., 1])) + (v[..., 2] * v[..., 2])).astype(F)


def _combine(c0, c1, c2, v):
    """c0*v.x + c1*v.y + c2*v.z per component, in the order of mat4.rs:146-149; c*: [n,3] (per corner), v: [n,3]"""
    return ((c0 * v[:, 0:1]) + (c1 * v[:, 1:2])) + (c2 * v[:, 2:3])


def transform(matrices, part_of, pos, nrm):
    """matrices [n_parts,16] (Mat4f data[col][row]); part_of [n]: the part of every corner; pos, nrm [n,3] float32"""
    m = np.asarray(matrices, dtype=F).reshape(-1, 4, 4)
    a0, a1, a2, tr = m[:, 0, :3], m[:, 1, :3], m[:, 2, :3], m[:, 3, :3]
    c0, c1, c2 = _cross(a1, a2), _cross(a2, a0), _cross(a0, a1)          # once per part
    with np.errstate(all="ignore"):
        p = (_combine(a0[part_of], a1[part_of], a2[part_of], pos) + tr[part_of]).astype(F)
        l0 = _length(nrm)
        c = _combine(c0[part_of], c1[part_of], c2[part_of], nrm).astype(F)
        l1 = _length(c)
        ok = (l1 > F(0)) & np.isfinite(l1)
        s = np.divide(l0, l1, out=np.ones_like(l0), where=ok)
        n = np.where(ok[:, None], c * s[:, None], c).astype(F)
    return p, n


def _gather(arr, idx, width):
    """rows arr[idx] as uint32 words; zeros where idx is out of range (unwrap_or(&[0.0; _]), scene.rs:56-65)"""
    out = np.zeros((len(idx), width), dtype=np.uint32)
    if arr is None or len(arr) == 0:
        return out
    a = np.ascontiguousarray(arr, dtype=F).reshape(-1, width).view(np.uint32)
    ok = idx < len(a)
    out[ok] = a[idx[ok].astype(np.int64)]
    return out


def expand(positions, normals, tex_coords, indices, parts, normal_indices=None, tex_coord_indices=None, transforms=None):
    """The rule.  Raises ValueError for a position index out of range (naming the first offending index entry)."""
    ip = np.asarray(indices, dtype=np.uint32).reshape(-1)
    i_n = ip if normal_indices is None else np.asarray(normal_indices, dtype=np.uint32).reshape(-1)
    i_t = ip if tex_coord_indices is None else np.asarray(tex_coord_indices, dtype=np.uint32).reshape(-1)
    n_pos = 0 if positions is None else len(np.asarray(positions).reshape(-1, 3))
    bad = np.flatnonzero(ip >= n_pos)
    if len(bad):
        raise ValueError(f"position index out of range at index entry {bad[0]}")
    n_tris = len(ip) // 3
    pos = _gather(positions, ip, 3)
    nrm = _gather(normals, i_n, 3)
    tex = _gather(tex_coords, i_t, 2)
    parts = np.asarray(parts, dtype=PART)
    part_of_tri = np.repeat(np.arange(len(parts)), parts["n_tris"].astype(np.int64))
    assert len(part_of_tri) == n_tris
    if transforms is not None:
        p, n = transform(transforms, np.repeat(part_of_tri, 3), pos.view(F), nrm.view(F))
        pos, nrm = np.ascontiguousarray(p).view(np.uint32), np.ascontiguousarray(n).view(np.uint32)
    out = np.zeros(n_tris, dtype=TRIANGLE)
    w = out.view(np.uint32).reshape(n_tris, 28)
    v = w[:, :24].reshape(n_tris, 3, 8)
    v[:, :, 0:3] = pos.reshape(n_tris, 3, 3)
    v[:, :, 3] = tex[:, 0].reshape(n_tris, 3)
    v[:, :, 4:7] = nrm.reshape(n_tris, 3, 3)
    v[:, :, 7] = tex[:, 1].reshape(n_tris, 3)
    w[:, 24] = parts["material_id"][part_of_tri]
    return out


def _dedup(rows):
    """unique rows BY BIT PATTERN (-0.0 != 0.0, NaNs do not collapse): (unique float32 rows, index of every input row)"""
    w = np.ascontiguousarray(rows).view(np.uint32)
    if len(w) < 100000:
        u, inv = np.unique(w, axis=0, return_inverse=True)
        return u.view(F), inv.reshape(-1).astype(np.uint32)
    # the same result (rows in lexicographic order of their words) through a key sort: np.unique(axis=0) takes minutes at 30 M rows
    order = np.lexsort(w.T[::-1])
    s = w[order]
    new = np.r_[True, np.any(s[1:] != s[:-1], axis=1)]
    inv = np.empty(len(w), dtype=np.uint32)
    inv[order] = (np.cumsum(new) - 1).astype(np.uint32)
    return np.ascontiguousarray(s[new]).view(F), inv


def _cut_parts(mat_sorted, min_parts, empty_parts=0):
    """one part per material run, runs cut further until there are at least min(min_parts, n_tris) parts; `empty_parts` parts of
    no triangles are sprinkled in (they are legal: they tile nothing)"""
    n = len(mat_sorted)
    starts = np.flatnonzero(np.r_[True, mat_sorted[1:] != mat_sorted[:-1]])
    runs = [[int(s), int(e)] for s, e in zip(starts, np.r_[starts[1:], n])]
    want = min(min_parts, n)
    pieces = [[r] for r in runs]                               # per run: list of [s, e)
    while sum(len(p) for p in pieces) < want:
        k = max(range(len(pieces)), key=lambda i: max(e - s for s, e in pieces[i]))
        j = max(range(len(pieces[k])), key=lambda i: pieces[k][i][1] - pieces[k][i][0])
        s, e = pieces[k][j]
        mid = (s + e) // 2
        pieces[k][j:j + 1] = [[s, mid], [mid, e]]
    flat = [se for p in pieces for se in p]
    parts = np.zeros(len(flat), dtype=PART)
    for i, (s, e) in enumerate(flat):
        parts[i] = (s, e - s, mat_sorted[s], 0)
    if empty_parts:
        at = np.linspace(0, len(parts), empty_parts).astype(int)
        ins = np.zeros(empty_parts, dtype=PART)
        for i, a in enumerate(at):
            ins[i] = (parts[a]["first_tri"] if a < len(parts) else n, 0, mat_sorted[0], 0)
        parts = np.insert(parts, at, ins)
    return parts


def mesh_from_triangles(tris, min_parts=1, shared=False, empty_parts=0):
    """Fat triangles -> an indexed mesh.  A part has ONE material, so the triangles are first stable-sorted by material_id; the
    permutation is returned (expand(mesh) == tris[perm]).  Positions, normals and tex coords are de-duplicated by bit pattern into
    three arrays with three index streams; `shared`: re-indexed to unique full vertices with ONE stream instead.
    Returns (dict of from_mesh / expand keyword arguments, perm)."""
    tris = np.ascontiguousarray(tris)
    perm = np.argsort(tris["material_id"], kind="stable")
    t = tris[perm]
    v = t["vertices"].reshape(-1)
    pos = np.ascontiguousarray(v["position"])
    nrm = np.ascontiguousarray(v["normal"])
    tex = np.ascontiguousarray(np.stack([v["tex_coord_x"], v["tex_coord_y"]], axis=1))
    parts = _cut_parts(t["material_id"], min_parts, empty_parts)
    if shared:
        full, idx = _dedup(np.concatenate([pos, nrm, tex], axis=1))
        mesh = dict(positions=np.ascontiguousarray(full[:, 0:3]), normals=np.ascontiguousarray(full[:, 3:6]),
                    tex_coords=np.ascontiguousarray(full[:, 6:8]), indices=idx, normal_indices=None, tex_coord_indices=None, parts=parts)
    else:
        up, ip = _dedup(pos)
        un, i_n = _dedup(nrm)
        ut, i_t = _dedup(tex)
        mesh = dict(positions=up, normals=un, tex_coords=ut, indices=ip, normal_indices=i_n, tex_coord_indices=i_t, parts=parts)
    return mesh, perm
