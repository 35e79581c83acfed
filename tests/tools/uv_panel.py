"""The uv panel: 12 x 8 small quads in front of the camera, every TRIANGLE with one (u, v) at all three of its vertices, drawn from
the edge coordinates of tests/tools/texel_model.py -- so whole patches of the frame look a texture up at a texel boundary, a
negative coordinate, a subnormal, +-2^24, infinity or NaN, through the real kernels (trace, batch, first hit) instead of a probe.

The panel is the inside of half a cylinder with the camera in it, so every quad faces the camera, scattered rays meet other quads
and deeper bounces are textured too.  Its materials carry a base-colour and an emission texture of different, non-square sizes (5x3, 1x1, 7x2, 16x16 as height x
width); a few carry only one of the two.  The emission textures are dark and the sky is open, so paths end."""
import numpy as np

import texel_model as T

NX, NY = 12, 8
TEX_SHAPES = ((5, 3), (1, 1), (7, 2), (16, 16))                                  # (height, width)
# (base-colour texture, emission texture), None = the material's constant
MATERIAL_TEXTURES = ((0, 2), (2, 3), (3, 1), (1, 0), (0, None), (None, 3), (2, None), (None, 0))
CAMERA = ((0.0, 0.0, 0.0), 0.0, 0.0)                                            # looks down -X
SIZE, SPP, DEPTH = (64, 40), 2, 4


def textures(shapes=TEX_SHAPES, seed=5):
    """Every texel of every texture differs from every other in RGB (16-bit codes spread over R and G, the texture's number in B)"""
    rng = np.random.default_rng(seed)
    out = []
    for k, (h, w) in enumerate(shapes):
        # distinct 16-bit codes where the texture has at most 2^16 texels; a larger one takes random codes
        code = (rng.permutation(1 << 16)[: h * w] if h * w <= 1 << 16 else rng.integers(0, 1 << 16, h * w)).astype(np.uint32)
        t = np.zeros((h * w, 4), dtype=np.uint8)
        t[:, 0], t[:, 1], t[:, 2], t[:, 3] = code & 255, code >> 8, 16 * k + 7, rng.integers(0, 256, h * w)
        out.append(t.reshape(h, w, 4))
    return out


def _targets(w, h):
    """(u, v) that reach, on a w x h texture: texel 0; the last texel; NaN; a negative coordinate that stays inside (mixed signs:
    i = -1 with j = 2 where the texture has a third row, else -tiny); a clamped lookup"""
    f, up, dn = np.float32, np.float32(np.inf), np.float32(-np.inf)
    last = (np.nextafter(f(w - 1) / f(w), up), np.nextafter(f(h - 1) / f(h), up))
    mixed = (np.nextafter(f(-1) / f(w), dn), np.nextafter(f(2) / f(h), up)) if h >= 3 and w >= 2 else (f(-1e-45), f(0.0))
    return [(f(0.0), f(0.0)), last, (f(np.nan), f(0.0)), mixed, (f(-1e-45), f(-1e-30)), (np.nextafter(f(-1), f(0)), np.nextafter(f(-1), f(0)))]


def material_textures(n_textures):
    """MATERIAL_TEXTURES folded onto a scene with another number of textures (none: every material keeps its constants)"""
    fold = lambda i: None if i is None or n_textures == 0 else i % n_textures  # noqa: E731
    return tuple((fold(b), fold(e)) for b, e in MATERIAL_TEXTURES)


def uv_assignment(n_tris, material_of, tex_shapes=TEX_SHAPES, seed=9):
    """One (u, v) per triangle.  The first triangles of every material take the targets of its textures; the rest draw u from the
    boundary coordinates of a texture's width and the specials, v from those of its height and the specials."""
    rng = np.random.default_rng(seed)
    uv = np.zeros((n_tris, 2), dtype=np.float32)
    spec = T.special_coords()
    seen, mat_tex = {}, material_textures(len(tex_shapes))
    coords = {d: np.concatenate([T.boundary_coords(d), spec]) for hw in tex_shapes for d in hw}
    for t in range(n_tris):
        m = int(material_of[t])
        ids = [i for i in mat_tex[m] if i is not None]
        if not ids:
            uv[t] = (spec[int(rng.integers(len(spec)))], spec[int(rng.integers(len(spec)))])
            continue
        queue = seen.setdefault(m, [p for i in ids for p in _targets(tex_shapes[i][1], tex_shapes[i][0])])
        if queue:
            uv[t] = queue.pop(0)
            continue
        h, w = tex_shapes[ids[int(rng.integers(len(ids)))]]
        us, vs = coords[w], coords[h]
        uv[t] = (us[int(rng.integers(len(us)))], vs[int(rng.integers(len(vs)))])
    return uv


def panel(tex_shapes=TEX_SHAPES):
    """-> (tris, materials, textures, camera) as rust_ray_tracing_amd.synth.make_scene returns them"""
    from rust_ray_tracing_amd import synth
    axis_x, radius, half_angle, half_y = -1.0, 1.6, np.radians(80.0), 1.7         # half a cylinder round a vertical axis, the camera inside
    th, ys = np.linspace(-half_angle, half_angle, NX + 1), np.linspace(-half_y, half_y, NY + 1)

    def point(i, j):
        return (axis_x - radius * np.cos(th[i]), ys[j], radius * np.sin(th[i]))

    quads, material_of = [], []
    for j in range(NY):
        for i in range(NX):
            m = (i + 3 * j) % len(MATERIAL_TEXTURES)
            p = [np.array(point(i, j)), np.array(point(i + 1, j)), np.array(point(i + 1, j + 1)), np.array(point(i, j + 1))]
            n = np.cross(p[1] - p[0], p[3] - p[0])
            n = n / np.linalg.norm(n)
            if np.dot(n, np.array([axis_x, p[0][1], 0.0]) - p[0]) < 0:         # wound so that the front faces the axis (a back face's
                p, n = [p[0], p[3], p[2], p[1]], -n                            # normal is turned round at the hit: the path would leave)
            quads.append(synth.quad(p[0], p[1], p[2], p[3], n, m))
            material_of += [m, m]
    tris = np.concatenate(quads)
    # a material's triangles in a fixed pseudo-random order, so the targets do not all sit in one corner of the frame
    order = np.random.default_rng(3).permutation(len(tris))
    uv = np.zeros((len(tris), 2), dtype=np.float32)
    uv[order] = uv_assignment(len(tris), np.asarray(material_of)[order], tex_shapes)
    tris["vertices"]["tex_coord_x"] = uv[:, 0:1]
    tris["vertices"]["tex_coord_y"] = uv[:, 1:2]
    mats = []
    for k, (b, e) in enumerate(material_textures(len(tex_shapes))):
        base, emis = (0.3 + 0.05 * k, 0.8 - 0.04 * k, 0.55), (0.02 * k, 0.1, 0.25 - 0.02 * k)
        mats.append(synth.material(base=base, emission=emis, base_tex=synth.NO_TEXTURE if b is None else b,
                                   emission_tex=synth.NO_TEXTURE if e is None else e))
    return tris, mats, textures(tex_shapes), CAMERA


def scene(rrt, tex_shapes=TEX_SHAPES):
    tris, mats, texs, cam = panel(tex_shapes)
    sc = rrt.Scene.from_arrays(tris, mats, texs)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    return sc


def cameras(rrt):
    """the panel's camera and two more, for the 3-view batch"""
    out = []
    for pos, pitch, yaw in (CAMERA, ((0.3, 0.2, -0.4), 6.0, -9.0), ((-0.2, -0.3, 0.5), -8.0, 12.0)):
        c = rrt.Camera(position=pos, pitch=pitch, yaw=yaw)
        c.update_view()
        out.append(c)
    return out


def first_hit_lookups(sc, model_frame):
    """From a features-model frame of the panel (its `material` and `uv` buffers): for every texture, the texel indices the first
    hits look up, and over all lookups the counts of clamped ones, of NaN coordinates and of negative-but-unclamped ones.
    -> ({texture: set of indices}, dict(fetches, clamped, nan, negative_unclamped))"""
    mats = sc.materials_array()
    mat, uv = model_frame["material"].reshape(-1), model_frame["uv"].reshape(-1, 2)
    per_tex = {i: set() for i in range(len(sc.textures))}
    tot = dict(fetches=0, clamped=0, nan=0, negative_unclamped=0)
    for m in range(len(mats)):
        px = np.flatnonzero(mat == m)
        if not len(px):
            continue
        for slot in ("base_color_tex_id", "emission_tex_id"):
            tid = int(mats[m][slot])
            if tid == 0xFFFFFFFF:
                continue
            h, w = sc.textures[tid].shape[:2]
            u, v = uv[px, 0], uv[px, 1]
            idx, clamped, _ = T.lookup_index(u, v, w, h)
            per_tex[tid] |= set(idx.tolist())
            with np.errstate(all="ignore"):
                neg = (u < 0) | (v < 0)
            tot["fetches"] += len(px)
            tot["clamped"] += int(clamped.sum())
            tot["nan"] += int((np.isnan(u) | np.isnan(v)).sum())
            tot["negative_unclamped"] += int((neg & ~clamped).sum())
    return per_tex, tot


def assert_coverage(sc, model_frame):
    """What the panel is for, asserted on a features-model frame of its own camera (never on anything a GPU wrote)"""
    per_tex, tot = first_hit_lookups(sc, model_frame)
    assert 0 < tot["clamped"] < tot["fetches"], tot
    assert tot["nan"] > 0 and tot["negative_unclamped"] > 0, tot
    for tid, seen in per_tex.items():
        h, w = sc.textures[tid].shape[:2]
        assert 0 in seen and h * w - 1 in seen, (tid, sorted(seen))
