"""GPU: the refusals of the Python wrappers that only a device tensor reaches -- the second half of test_wrapper_messages.py, held to
the whole text in the same way.  A non-contiguous device tensor (a transposed view of the right shape) for one float plane of every
operator and for the material plane of upsample and temporal; render_adaptive's counts and out, and temporal's counts and history,
with their own texts; and, behind the same anchor, a tensor of the wrong dtype, device or shape and an array among tensors.

No kernel runs: every call is refused by the wrapper's own checks.  The planes are 2 views of 3 x 4 pixels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V, H, W, SCALE = 2, 3, 4, 2
LEAD, FULL = (V, H, W), (V, H * SCALE, W * SCALE)
CONTIGUOUS = ": expected a contiguous tensor"


def d(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device="cuda:0")


def nc(*shape, dtype=torch.float32):
    """of this shape, its last two dimensions transposed in memory"""
    a = d(*shape[:-2], shape[-1], shape[-2], dtype=dtype).transpose(-1, -2)
    assert tuple(a.shape) == shape and not a.is_contiguous()
    return a


def features(**change):
    return dict(dict(position=d(*LEAD, 3), normal=d(*LEAD, 3), depth=d(*LEAD), material=d(*LEAD, dtype=torch.int32)), **change)


def lo_full(name, lo, full):
    return dict(lo_hdr=d(*LEAD, 3), lo_guides={name: lo}, guides={name: full}, scale=SCALE)


def cases(rrt, r):
    from rust_ray_tracing_amd import _lib as L
    cams = np.zeros(V, dtype=L.CAMERA)
    ids = torch.int32
    points = d(H * W, 4, dtype=ids)
    scene = rrt.Scene()                                                 # never uploaded: handle=1 stands in, and is never used

    def temporal(hdr=None, **kw):
        return lambda: r.temporal(d(*LEAD, 3) if hdr is None else hdr, kw.pop("features", features()), cams, **kw)

    def adaptive(**kw):
        return lambda: r.render_adaptive(scene, handle=1, **kw)

    return [
        (lambda: r.denoise(nc(*LEAD, 3)), "hdr" + CONTIGUOUS),
        (lambda: r.denoise(d(*LEAD, 3), normal=nc(*LEAD, 3)), "normal" + CONTIGUOUS),
        (lambda: r.denoise(d(*LEAD, 3), depth=nc(*LEAD)), "depth" + CONTIGUOUS),
        (lambda: r.denoise(d(*LEAD, 3), normal=d(*LEAD, 3, dtype=torch.float64)), "normal: expected a float32 tensor on hdr's device cuda:0"),
        (lambda: r.denoise(d(*LEAD, 3), albedo=torch.zeros(*LEAD, 3)), "albedo: expected a float32 tensor on hdr's device cuda:0"),
        (lambda: r.denoise(d(*LEAD, 3), depth=d(*LEAD, 1)), "depth: expected shape (2, 3, 4); got (2, 3, 4, 1)"),
        (lambda: r.denoise(d(*LEAD, 3), normal=np.zeros(LEAD + (3,), np.float32)),
         "normal: hdr and the guides must all be numpy arrays or all torch tensors"),
        (lambda: r.denoise_variance(d(*LEAD, 3), albedo=nc(*LEAD, 3)), "albedo" + CONTIGUOUS),
        (lambda: r.denoise_variance(d(*LEAD, 3), nc(*LEAD), d(*LEAD)), "variance" + CONTIGUOUS),
        (lambda: r.denoise_variance(d(*LEAD, 3), d(*LEAD), nc(*LEAD)), "length" + CONTIGUOUS),
        (lambda: r.denoise_variance(d(*LEAD, 3), d(*LEAD), d(*LEAD, dtype=ids)), "length: expected a float32 tensor on hdr's device cuda:0"),
        (lambda: r.denoise_variance(d(*LEAD, 3), nc(H, W), d(*LEAD)), "variance: expected shape (2, 3, 4); got (3, 4)"),
        (lambda: r.upsample(**lo_full("normal", nc(*LEAD, 3), d(*FULL, 3))), "lo_normal" + CONTIGUOUS),
        (lambda: r.upsample(**lo_full("material", d(*LEAD, dtype=ids), nc(*FULL, dtype=ids))), "material" + CONTIGUOUS),
        (lambda: r.upsample(**lo_full("material", d(*LEAD), d(*FULL, dtype=ids))), "lo_material: expected a int32 tensor on lo_hdr's device cuda:0"),
        (lambda: r.upsample(**lo_full("depth", d(*LEAD), d(*FULL, dtype=ids))), "depth: expected a float32 tensor on lo_hdr's device cuda:0"),
        (lambda: r.upsample(**lo_full("material", d(*LEAD, dtype=ids), nc(*LEAD, dtype=ids))), "material: expected shape (2, 6, 8); got (2, 3, 4)"),
        (lambda: r.sample_map(d(*LEAD), hdr=nc(*LEAD, 3)), "hdr" + CONTIGUOUS),
        (lambda: r.sample_map(nc(*LEAD), rounds=2), "variance" + CONTIGUOUS),
        (lambda: r.sample_map(d(*LEAD), hdr=d(*LEAD, 3), albedo=nc(*LEAD, 3), rounds=2), "albedo" + CONTIGUOUS),
        (lambda: r.sample_map(d(*LEAD), hdr=d(*LEAD, 3, dtype=torch.float16)), "hdr: expected a float32 tensor on variance's device cuda:0"),
        (temporal(features=features(position=nc(*LEAD, 3))), "position" + CONTIGUOUS),
        (temporal(features=features(material=nc(*LEAD, dtype=ids))), "material" + CONTIGUOUS),
        (temporal(features=features(material=d(*LEAD))), "material: expected a int32 tensor on hdr's device cuda:0"),
        (temporal(features=features(depth=d(*LEAD, dtype=ids))), "depth: expected a float32 tensor on hdr's device cuda:0"),
        (temporal(features=features(material=nc(H, W, dtype=ids))), "material: expected shape (2, 3, 4); got (3, 4)"),
        (temporal(counts=nc(*LEAD, dtype=ids)), "counts: expected a contiguous int32 tensor on hdr's device cuda:0"),
        (temporal(counts=d(*LEAD)), "counts: expected a contiguous int32 tensor on hdr's device cuda:0"),
        (temporal(counts=nc(H, W, dtype=ids)), "counts: expected shape (2, 3, 4); got (3, 4)"),
        (temporal(history=nc(2, 160, dtype=ids)), "history: expected a contiguous int32 tensor of 320 words on hdr's device cuda:0"),
        (temporal(history_out=d(319, dtype=ids)), "history_out: expected a contiguous int32 tensor of 320 words on hdr's device cuda:0"),
        (adaptive(counts=nc(H, W, dtype=ids)), "counts: expected a contiguous int32 tensor on cuda:0"),
        (adaptive(counts=d(H, W, dtype=ids), out=nc(1, H, W, 3)), "out: expected a contiguous float32 tensor of shape (1, 3, 4, 3) on cuda:0"),
        (adaptive(counts=d(H, W, dtype=ids), out=d(H, W, 3)), "out: expected a contiguous float32 tensor of shape (1, 3, 4, 3) on cuda:0"),
        (lambda: rrt.Scene.lightmap_filter(nc(H, W, 3), points), "radiance" + CONTIGUOUS),
        (lambda: rrt.Scene.lightmap_filter(d(H, W, 3), points, position=nc(H, W, 3)), "position" + CONTIGUOUS),
        (lambda: rrt.Scene.lightmap_filter(d(H, W, 3), points, normal=nc(H * W, 3)), "normal" + CONTIGUOUS),
        (lambda: rrt.Scene.lightmap_filter(d(H, W, 3), points, position=d(H * W, 3), normal=d(H * W, 4)),
         "normal: expected shape (3, 4, 3); got (12, 4)"),
        (lambda: rrt.Scene.lightmap_filter(d(H, W, 3), points, position=d(H, W, 3), normal=d(H, W, 3, dtype=torch.float64)),
         "normal: expected a float32 tensor on radiance's device cuda:0"),
        (lambda: rrt.Scene.lightmap_filter(d(H, W, 3), np.zeros(H * W, dtype=L.SURFACE_POINT)),
         "points: radiance and points must both be numpy arrays or both device tensors"),
        (lambda: rrt.Scene.lightmap_dilate(nc(H, W, 3), points), "radiance" + CONTIGUOUS),
        (lambda: rrt.Scene.lightmap_dilate(d(H, W, 3, dtype=torch.float64), points, want_level=True),
         "radiance: expected a float32 tensor on radiance's device cuda:0"),
    ]


def test_device_tensors_are_refused_with_the_whole_message(rrt):
    r = rrt.Renderer(rrt.RendererOptions(samples=4, output_image_dimensions=(W, H), output_image_path="/dev/null"))
    table = cases(rrt, r)
    for i, (call, text) in enumerate(table):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text, i
    assert len(table) == 42
