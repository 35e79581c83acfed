"""The inputs of the temporal-accumulation tests (tests/test_gpu_temporal.py, tests/test_cpp_host_temporal.py): a small analytic world
-- a back wall with windows onto nothing, a floor and two side walls -- seen through cameras built by hand, so that two cameras see
consistent positions, normals and materials and the taps of the reprojection are reused.  Everything is generated from the size, the
number of views, the camera move and a seed."""
import math

import numpy as np

CAMERA = np.dtype([("look_at", "<f4", (4, 4)), ("position", "<f4", 3), ("_pad", "<f4")])
NONE = 0xFFFFFFFF

# the frames of a sequence, as the move of the camera against the first frame's: (position offset, yaw, pitch in degrees)
SAME, NEAR, FAR = ((0.0, 0.0, 0.0), 0.0, 0.0), ((0.15, 0.05, 0.2), 4.0, 1.5), ((0.8, 0.1, 2.5), -75.0, 3.0)
SEQUENCE = (SAME, SAME, NEAR, FAR)                              # first frame, same camera, translated and yawed, turned far away


# ---- the analytic world --------------------------------------------------------------------------------------------------------
def camera(view, move=SAME):
    """a camera near the origin looking down +z: look_at[c][r] = R[r][c] as mat4.rs:25-44 fills it, the position in column 3"""
    k = view % 7
    pos = np.array([0.1 * k, 0.05 * k, -0.2 * k]) + np.array(move[0])
    yaw, pitch = math.radians(3.0 * k - 6.0 + move[1]), math.radians(1.0 * k + move[2])
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    rot = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    cam = np.zeros((), dtype=CAMERA)
    cam["look_at"][:3, :3] = rot.T
    cam["look_at"][3, :3], cam["look_at"][3, 3] = pos, 1.0
    cam["position"] = pos
    return cam


def view_of_the_world(cam, w, h):
    """what the camera sees, from pixel centres (cpu.rs:31-35,44 without the jitter): position, normal, depth, material [H,W(,3)]"""
    a = cam["look_at"][:3, :3].T.astype(np.float64)
    c = cam["position"].astype(np.float64)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    sx, sy = ((xs / w) * 2 - 1) * (w / h), ((h - ys) / h) * 2 - 1
    d = np.stack([-sx, sy, np.ones_like(sx)], axis=-1) @ a.T
    planes = ((2, 6.0, 1, (0, 0, -1)), (1, -1.5, -1, (0, 1, 0)), (0, 2.5, 1, (-1, 0, 0)), (0, -2.5, -1, (1, 0, 0)))     # axis, offset, side, normal
    with np.errstate(all="ignore"):
        ts = np.stack([np.where(d[..., ax] * side > 1e-9, (off - c[ax]) / d[..., ax], np.inf) for ax, off, side, _ in planes])
    which = ts.argmin(0)
    t = ts.min(0)
    hit = np.isfinite(t) & (t > 0)
    p = c + np.where(hit, t, 0.0)[..., None] * d
    window = (which == 0) & ((np.floor(p[..., 0] * 1.3) + np.floor(p[..., 1] * 1.7)) % 4 == 0)
    hit &= ~window
    normal = np.array([n for _, _, _, n in planes], dtype=np.float64)[which] + 0.04 * np.sin(5.0 * p)
    material = ((np.floor(p[..., 0] * 2) + np.floor(p[..., 1] * 2) + np.floor(p[..., 2] * 2)) % 3).astype(np.uint32)     # the same across a corner: the normal decides there
    position = np.where(hit[..., None], p, 0.0).astype(np.float32)
    dd = position - cam["position"]
    depth = np.where(hit, np.sqrt(((dd * dd).sum(-1)).astype(np.float32)), np.float32(1e30)).astype(np.float32)
    return dict(position=position, normal=np.where(hit[..., None], normal, 0.0).astype(np.float32), depth=depth,
                material=np.where(hit, material, NONE).astype(np.uint32))


_frames = {}


def frame(size, views, move, seed=0):
    """-> (cameras [V], planes {name: [V,H,W(,k)]}): the world through `views` cameras moved by `move`, radiance in [0, 4), albedo in (0, 1]"""
    key = (size, views, move, seed)
    if key not in _frames:
        w, h = size
        cams = np.stack([camera(v, move) for v in range(views)])
        per_view = [view_of_the_world(cams[v], w, h) for v in range(views)]
        planes = {k: np.ascontiguousarray(np.stack([g[k] for g in per_view])) for k in per_view[0]}
        rng = np.random.default_rng(1000 * w + 10 * h + views + 77 * seed + int(1e4 * abs(move[1])))
        planes["hdr"] = (rng.random((views, h, w, 3)) ** 2 * 4.0).astype(np.float32)
        planes["albedo"] = (0.02 + 0.98 * rng.random((views, h, w, 3))).astype(np.float32)
        _frames[key] = (cams, planes)
    return _frames[key]
