"""CPU: the whole text of every ValueError the Python wrappers of the image-space operators raise before they call libmipt --
the Python twin of test_plane_entry_messages.py.  Renderer.denoise, denoise_variance, upsample, sample_map (plain and rounds=),
temporal (counts and history included), render_adaptive's counts, Scene.lightmap_filter and lightmap_dilate.  The model tests
beside this one only look at how a message starts; here every refusal is held to its full wording, and inputs with two faults fix
which of the two is reported.

Nothing is launched: every call is refused by the wrapper's own checks.  The planes are 2 views of 3 x 4 pixels.  What only a
device tensor can reach (the checks behind "expected a ... tensor on hdr's device") is in test_gpu_wrapper_messages.py."""
import numpy as np
import pytest
import torch

V, H, W, SCALE = 2, 3, 4, 2
LEAD, FULL = (V, H, W), (V, H * SCALE, W * SCALE)
ALL = "must all be numpy arrays or all torch tensors"


def f(*shape, dtype=np.float32):
    return np.zeros(shape, dtype=dtype)


def t(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)                              # a host tensor: never the device the wrappers want


HDR, PLANE, IDS = f(*LEAD, 3), f(*LEAD), f(*LEAD, dtype=np.uint32)
GUIDES = " and the guides " + ALL


def features(**change):
    d = dict(position=f(*LEAD, 3), normal=f(*LEAD, 3), depth=f(*LEAD), material=f(*LEAD, dtype=np.uint32))
    d.update(change)
    return {k: v for k, v in d.items() if v is not None}


def lo_full(name, lo, full):
    """upsample's two dicts with one guide in them"""
    return dict(lo_guides={name: lo}, guides={name: full}, scale=SCALE)


DENOISE = [  # Renderer.denoise(hdr, normal, depth, albedo) and, with the same planes, denoise_variance
    (dict(hdr=HDR, normal=t(*LEAD, 3)), "normal: hdr" + GUIDES),
    (dict(hdr=HDR, depth=t(*LEAD)), "depth: hdr" + GUIDES),
    (dict(hdr=HDR, albedo=[[0.0]], normal=t(*LEAD, 3)), "normal: hdr" + GUIDES),
    (dict(hdr=HDR.astype(np.float64)), "hdr: expected float32; got float64"),
    (dict(hdr=HDR, depth=f(*LEAD, dtype=np.int32)), "depth: expected float32; got int32"),
    (dict(hdr=HDR, albedo=f(*LEAD, 3, dtype=np.float16)), "albedo: expected float32; got float16"),
    (dict(hdr=f(W, 3)), "hdr: expected shape [V,H,W,3] or [H,W,3]; got (4, 3)"),
    (dict(hdr=f(*LEAD, 4)), "hdr: expected shape [V,H,W,3] or [H,W,3]; got (2, 3, 4, 4)"),
    (dict(hdr=HDR, depth=f(*LEAD, 3)), "depth: expected shape (2, 3, 4); got (2, 3, 4, 3)"),
    (dict(hdr=HDR, normal=f(V, H, W + 1, 3)), "normal: expected shape (2, 3, 4, 3); got (2, 3, 5, 3)"),
    (dict(hdr=HDR[0], normal=f(*LEAD, 3)), "normal: expected shape (3, 4, 3); got (2, 3, 4, 3)"),
    (dict(hdr=HDR, normal=f(*LEAD, 3, dtype=np.float64), depth=f(H, W)), "normal: expected float32; got float64"),
    (dict(hdr=HDR, normal=f(*LEAD, dtype=np.float64)), "normal: expected float32; got float64"),
    (dict(hdr=t(*LEAD, 3)), "hdr: expected a float32 tensor on hdr's device cpu"),
    (dict(hdr=t(*LEAD, 3, dtype=torch.float64)), "hdr: expected a float32 tensor on hdr's device cpu"),
    (dict(hdr=t(H, W)), "hdr: expected shape [V,H,W,3] or [H,W,3]; got (3, 4)"),
    (dict(hdr=t(*LEAD, 3), normal=f(*LEAD, 3)), "hdr: expected a float32 tensor on hdr's device cpu"),
]
VARIANCE_ALL = "hdr, the guides, variance and length " + ALL
VARIANCE = [  # what denoise_variance adds: variance and length
    (dict(hdr=HDR, variance=t(*LEAD), length=PLANE), "variance: " + VARIANCE_ALL),
    (dict(hdr=HDR, variance=PLANE, length=t(*LEAD)), "length: " + VARIANCE_ALL),
    (dict(hdr=HDR, variance=PLANE.astype(np.float64), length=PLANE), "variance: expected float32; got float64"),
    (dict(hdr=HDR, variance=PLANE, length=IDS), "length: expected float32; got uint32"),
    (dict(hdr=HDR, variance=f(*LEAD, 3), length=PLANE), "variance: expected shape (2, 3, 4); got (2, 3, 4, 3)"),
    (dict(hdr=HDR, variance=PLANE, length=f(V, H, W + 1)), "length: expected shape (2, 3, 4); got (2, 3, 5)"),
    (dict(hdr=HDR[0], variance=PLANE, length=PLANE[0]), "variance: expected shape (3, 4); got (2, 3, 4)"),
    (dict(hdr=HDR, variance=t(*LEAD), depth=t(*LEAD)), "depth: hdr" + GUIDES),                 # the guides are checked first
    (dict(hdr=HDR, variance=f(H, W), length=PLANE.astype(np.float64)), "variance: expected shape (2, 3, 4); got (3, 4)"),
]
LO = f(*LEAD, 3)
UPSAMPLE = [  # Renderer.upsample(lo_hdr, lo_guides, guides, scale)
    (dict(lo_hdr=LO, **lo_full("normal", t(*LEAD, 3), f(*FULL, 3))), "lo_normal: lo_hdr" + GUIDES),
    (dict(lo_hdr=LO, **lo_full("material", f(*LEAD, dtype=np.uint32), t(*FULL, dtype=torch.int32))), "material: lo_hdr" + GUIDES),
    (dict(lo_hdr=LO.astype(np.float64), lo_guides=None, guides=None, scale=SCALE), "lo_hdr: expected float32; got float64"),
    (dict(lo_hdr=LO, **lo_full("depth", f(*LEAD), f(*FULL, dtype=np.float64))), "depth: expected float32; got float64"),
    (dict(lo_hdr=LO, **lo_full("material", f(*LEAD), f(*FULL, dtype=np.uint32))), "lo_material: expected uint32; got float32"),
    (dict(lo_hdr=LO, **lo_full("material", f(*LEAD, dtype=np.uint32), f(*FULL, dtype=np.int32))), "material: expected uint32; got int32"),
    (dict(lo_hdr=f(W, 3), lo_guides=None, guides=None, scale=SCALE), "lo_hdr: expected shape [V,h,w,3] or [h,w,3]; got (4, 3)"),
    (dict(lo_hdr=LO, **lo_full("normal", f(*LEAD, 3), f(*FULL))), "normal: expected shape (2, 6, 8, 3); got (2, 6, 8)"),
    (dict(lo_hdr=LO, **lo_full("depth", f(V, H, W + 1), f(*FULL))), "lo_depth: expected shape (2, 3, 4); got (2, 3, 5)"),
    (dict(lo_hdr=LO, **lo_full("albedo", f(*LEAD, 3), f(*LEAD, 3))), "albedo: expected shape (2, 6, 8, 3); got (2, 3, 4, 3)"),
    (dict(lo_hdr=LO, **lo_full("material", f(*LEAD, dtype=np.uint32), f(*LEAD, dtype=np.uint32))), "material: expected shape (2, 6, 8); got (2, 3, 4)"),
    (dict(lo_hdr=LO, **lo_full("material", f(*LEAD, 1, dtype=np.uint32), f(*FULL, dtype=np.uint32))), "lo_material: expected shape (2, 3, 4); got (2, 3, 4, 1)"),
    (dict(lo_hdr=LO[0], **lo_full("depth", f(H, W), f(*FULL))), "depth: expected shape (6, 8); got (2, 6, 8)"),
    (dict(lo_hdr=t(*LEAD, 3), lo_guides=None, guides=None, scale=SCALE), "lo_hdr: expected a float32 tensor on lo_hdr's device cpu"),
    (dict(lo_hdr=t(W), lo_guides=None, guides=None, scale=SCALE), "lo_hdr: expected shape [V,h,w,3] or [h,w,3]; got (4,)"),
    # what only upsample knows comes before any plane is looked at
    (dict(lo_hdr=LO, lo_guides=None, guides=None, scale=1), "scale: expected an integer 2 ... 8; got 1"),
    (dict(lo_hdr=LO, lo_guides=None, guides=None, scale=True), "scale: expected an integer 2 ... 8; got True"),
    (dict(lo_hdr=LO, lo_guides=[], guides=None, scale=SCALE), "lo_guides: expected a dict with any of normal, depth, albedo, material, or None"),
    (dict(lo_hdr=LO, lo_guides=None, guides=3, scale=SCALE), "guides: expected a dict with any of normal, depth, albedo, material, or None"),
    (dict(lo_hdr=LO, lo_guides={}, guides={"normal": f(*FULL, 3)}, scale=SCALE),
     "lo_normal: normal is given at both resolutions or at neither; only guides holds it"),
    (dict(lo_hdr=LO, lo_guides={"depth": f(*LEAD)}, guides=None, scale=SCALE),
     "depth: depth is given at both resolutions or at neither; only lo_guides holds it"),
    (dict(lo_hdr=LO.astype(np.float64), lo_guides={"material": IDS}, guides={}, scale=SCALE),
     "material: material is given at both resolutions or at neither; only lo_guides holds it"),
]
MAP_ALL = "variance, hdr and albedo " + ALL
SAMPLE_MAP = [  # Renderer.sample_map(variance, hdr, albedo), with and without rounds=
    (dict(variance=PLANE, hdr=t(*LEAD, 3)), "hdr: " + MAP_ALL),
    (dict(variance=PLANE, hdr=HDR, albedo=t(*LEAD, 3)), "albedo: " + MAP_ALL),
    (dict(variance=PLANE.astype(np.float64)), "variance: expected float32; got float64"),
    (dict(variance=PLANE, hdr=HDR, albedo=f(*LEAD, 3, dtype=np.uint8)), "albedo: expected float32; got uint8"),
    (dict(variance=f(W)), "variance: expected shape [V,H,W] or [H,W]; got (4,)"),
    (dict(variance=f(*LEAD, 3)), "variance: expected shape [V,H,W] or [H,W]; got (2, 3, 4, 3)"),
    (dict(variance=PLANE, hdr=PLANE), "hdr: expected shape (2, 3, 4, 3); got (2, 3, 4)"),
    (dict(variance=PLANE, hdr=HDR, albedo=f(*LEAD, 4)), "albedo: expected shape (2, 3, 4, 3); got (2, 3, 4, 4)"),
    (dict(variance=PLANE[0], hdr=HDR), "hdr: expected shape (3, 4, 3); got (2, 3, 4, 3)"),
    (dict(variance=PLANE, albedo=HDR), "albedo: given only with hdr"),
    (dict(variance=f(W), albedo=HDR), "variance: expected shape [V,H,W] or [H,W]; got (4,)"),
    (dict(variance=PLANE, hdr=HDR.astype(np.float64), albedo=f(H, W)), "hdr: expected float32; got float64"),
    (dict(variance=t(*LEAD)), "variance: expected a float32 tensor on variance's device cpu"),
    (dict(variance=t(*LEAD, dtype=torch.int32), hdr=HDR), "variance: expected a float32 tensor on variance's device cpu"),
    (dict(variance=t(W)), "variance: expected shape [V,H,W] or [H,W]; got (4,)"),
]
FEATURES = "hdr and the features " + ALL
HOLD = "features must hold it (render_features with position, normal, depth, material)"
CAMS = "cams"                                                           # replaced by V camera records
TEMPORAL = [  # Renderer.temporal(hdr, features, cameras, history=, counts=, samples_cap=)
    (dict(hdr=HDR, features=features(position=t(*LEAD, 3))), "position: " + FEATURES),
    (dict(hdr=HDR, features=features(material=t(*LEAD, dtype=torch.int32))), "material: " + FEATURES),
    (dict(hdr=HDR, features=features(albedo=t(*LEAD, 3))), "albedo: " + FEATURES),
    (dict(hdr=HDR.astype(np.float64), features=features()), "hdr: expected float32; got float64"),
    (dict(hdr=HDR, features=features(normal=f(*LEAD, 3, dtype=np.float64))), "normal: expected float32; got float64"),
    (dict(hdr=HDR, features=features(material=f(*LEAD, dtype=np.int32))), "material: expected uint32; got int32"),
    (dict(hdr=HDR, features=features(material=f(*LEAD))), "material: expected uint32; got float32"),
    (dict(hdr=f(W, 3), features=features()), "hdr: expected shape [V,H,W,3] or [H,W,3]; got (4, 3)"),
    (dict(hdr=HDR, features=features(depth=f(*LEAD, 1))), "depth: expected shape (2, 3, 4); got (2, 3, 4, 1)"),
    (dict(hdr=HDR, features=features(position=f(V, H + 1, W, 3))), "position: expected shape (2, 3, 4, 3); got (2, 4, 4, 3)"),
    (dict(hdr=HDR, features=features(material=f(V, H, W + 1, dtype=np.uint32))), "material: expected shape (2, 3, 4); got (2, 3, 5)"),
    (dict(hdr=HDR, features=features(material=f(H, W, dtype=np.uint32))), "material: expected shape (2, 3, 4); got (3, 4)"),
    (dict(hdr=HDR, features=features(albedo=f(*LEAD))), "albedo: expected shape (2, 3, 4, 3); got (2, 3, 4)"),
    (dict(hdr=t(*LEAD, 3), features=features()), "hdr: expected a float32 tensor on hdr's device cpu"),
    (dict(hdr=t(H, W), features=features()), "hdr: expected shape [V,H,W,3] or [H,W,3]; got (3, 4)"),
    (dict(hdr=HDR, features=[]), "features: expected a dict with position, normal, depth, material and optionally albedo"),
    (dict(hdr=f(W, 3), features=None), "hdr: expected shape [V,H,W,3] or [H,W,3]; got (4, 3)"),
    (dict(hdr=HDR, features=features(depth=None)), "depth: " + HOLD),
    (dict(hdr=HDR, features={}), "position: " + HOLD),
    (dict(hdr=HDR.astype(np.float64), features={}), "hdr: expected float32; got float64"),
    # a plane is looked at before the next one is missed
    (dict(hdr=HDR, features=features(position=f(*LEAD, 3, dtype=np.float64), normal=None)), "position: expected float32; got float64"),
    (dict(hdr=HDR, features=features(position=None, normal=f(*LEAD, 3, dtype=np.float64))), "position: " + HOLD),
    (dict(hdr=HDR, features=features(), cameras=1), "cameras: expected 2 cameras, one per view; got 1"),
    (dict(hdr=HDR[0], features={k: a[0] for k, a in features().items()}, cameras=V), "cameras: expected 1 cameras, one per view; got 2"),
    (dict(hdr=HDR, features=features(material=f(*LEAD)), cameras=1), "material: expected uint32; got float32"),
    (dict(hdr=HDR, features=features(), samples_cap=4), "samples_cap: given only with counts"),
    (dict(hdr=HDR, features=features(), counts=t(*LEAD, dtype=torch.int32)), "counts: hdr and counts must both be numpy arrays or both torch tensors"),
    (dict(hdr=HDR, features=features(), counts=f(*LEAD, dtype=np.int32)), "counts: expected uint32; got int32"),
    (dict(hdr=HDR, features=features(), counts=PLANE), "counts: expected uint32; got float32"),
    (dict(hdr=HDR, features=features(), counts=f(H, W, dtype=np.uint32)), "counts: expected shape (2, 3, 4); got (3, 4)"),
    (dict(hdr=HDR, features=features(), counts=f(V, H, W + 1, dtype=np.uint32)), "counts: expected shape (2, 3, 4); got (2, 3, 5)"),
    (dict(hdr=HDR, features=features(), counts=f(H, W, dtype=np.int32)), "counts: expected uint32; got int32"),
    (dict(hdr=HDR, features=features(), history=f(5)), "history: expected a uint32 array of 320 words; got float32 of 5"),
    (dict(hdr=HDR, features=features(), history=f(320, dtype=np.int32)), "history: expected a uint32 array of 320 words; got int32 of 320"),
    (dict(hdr=HDR, features=features(), history=f(319, dtype=np.uint32)), "history: expected a uint32 array of 320 words; got uint32 of 319"),
    (dict(hdr=HDR, features=features(), history=f(5), counts=f(H, W, dtype=np.uint32)), "counts: expected shape (2, 3, 4); got (3, 4)"),
]
N_TEXELS = H * W
RAD = f(H, W, 3)
BOTH = "points: radiance and points must both be numpy arrays or both device tensors"
LIGHTMAP = [  # Scene.lightmap_filter(radiance, points, position, normal) and, without the guides, lightmap_dilate
    (dict(radiance=RAD, position=t(H, W, 3)), "position: radiance" + GUIDES),
    (dict(radiance=RAD, position=RAD, normal=t(N_TEXELS, 3)), "normal: radiance" + GUIDES),
    (dict(radiance=RAD.astype(np.float64)), "radiance: expected float32; got float64"),
    (dict(radiance=RAD, normal=f(H, W, 3, dtype=np.float64)), "normal: expected float32; got float64"),
    (dict(radiance=HDR), "radiance: expected shape [H,W,3]; got (2, 3, 4, 3)"),
    (dict(radiance=f(H, W, 4)), "radiance: expected shape [H,W,3]; got (3, 4, 4)"),
    (dict(radiance=t(W)), "radiance: expected shape [H,W,3]; got (4,)"),
    # a guide is [H,W,3] or [H*W,3] -- anything of that many values in threes; both forms pass and the plane after them is refused
    (dict(radiance=RAD, position=f(H, W, 3), normal=f(N_TEXELS, 4)), "normal: expected shape (3, 4, 3); got (12, 4)"),
    (dict(radiance=RAD, position=f(N_TEXELS, 3), normal=f(H, W + 1, 3)), "normal: expected shape (3, 4, 3); got (3, 5, 3)"),
    (dict(radiance=RAD, position=f(H, 3, W)), "position: expected shape (3, 4, 3); got (3, 3, 4)"),
    (dict(radiance=RAD, position=f(N_TEXELS * 3)), "position: expected shape (3, 4, 3); got (36,)"),
    (dict(radiance=RAD, position=f(N_TEXELS + 1, 3)), "position: expected shape (3, 4, 3); got (13, 3)"),
    (dict(radiance=RAD, position=f(N_TEXELS, 3, dtype=np.float64), normal=f(H, W)), "position: expected float32; got float64"),
    # a host tensor as the anchor: the records are a numpy array, and radiance's kind is held against theirs first
    (dict(radiance=t(H, W, 3)), BOTH),
    (dict(radiance=t(H, W, 3, dtype=torch.float64), position=RAD), BOTH),
    (dict(radiance=RAD, points=N_TEXELS - 1), "points: expected 12 records, one per texel; got 11"),
    (dict(radiance=RAD.astype(np.float64), points=N_TEXELS + 1), "points: expected 12 records, one per texel; got 13"),
    (dict(radiance=RAD, points=f(N_TEXELS, 3)),
     "points: expected SURFACE_POINT or HIT records, an (n, 4) array of 32-bit words, an int32 device tensor of shape (n, 4) or the dict "
     "query_closest returns"),
    (dict(radiance=RAD, points=t(N_TEXELS, 4, dtype=torch.int32)), "points: expected a contiguous int32 device tensor of shape (n, 4)"),
]
ADAPTIVE = [  # Renderer.render_adaptive(scene, counts, cameras, out=): its checks of counts are its own
    (dict(counts=f(H, W + 1, dtype=np.uint32)), "counts: expected shape (1, 3, 4); got (3, 5)"),
    (dict(counts=f(H, W, dtype=np.uint32), cameras=V), "counts: expected shape (2, 3, 4); got (3, 4)"),
    (dict(counts=f(1, H, W, dtype=np.uint32), cameras=V), "counts: expected shape (2, 3, 4); got (1, 3, 4)"),
    (dict(counts=t(H, W + 1, dtype=torch.int32)), "counts: expected shape (1, 3, 4); got (3, 5)"),
    (dict(counts=f(H, W, dtype=np.int32)), "counts: expected uint32; got int32"),
    (dict(counts=f(1, H, W)), "counts: expected uint32; got float32"),
    (dict(counts=f(H, W, dtype=np.uint32), out=f(1, H, W, 3)), "out: a tensor to write needs counts as a tensor"),
    (dict(counts=f(H, W, dtype=np.int32), out=t(1, H, W, 3)), "out: a tensor to write needs counts as a tensor"),
    (dict(counts=t(H, W, dtype=torch.int32)), "counts: expected a contiguous int32 tensor on cuda:0"),
    (dict(counts=t(V, H, W), cameras=V), "counts: expected a contiguous int32 tensor on cuda:0"),
    (dict(counts=f(H, W, dtype=np.uint32), cameras=0), "render_adaptive: no cameras"),
    (dict(counts=f(W), cameras=0), "render_adaptive: no cameras"),
]


@pytest.fixture(scope="module")
def renderer(rrt):
    return rrt.Renderer(rrt.RendererOptions(samples=4, output_image_dimensions=(W, H), output_image_path="/dev/null"))


def cameras(rrt, n):
    from rust_ray_tracing_amd import _lib as L
    return [rrt.Camera() for _ in range(n // 2)] + list(np.zeros(n - n // 2, dtype=L.CAMERA))      # both kinds a table is made of


def refused(call, text):
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) == text


@pytest.mark.parametrize("i", range(len(DENOISE)))
def test_denoise(renderer, i):
    kw, text = DENOISE[i]
    refused(lambda: renderer.denoise(**kw), text)
    refused(lambda: renderer.denoise_variance(**kw), text)


@pytest.mark.parametrize("i", range(len(VARIANCE)))
def test_denoise_variance(renderer, i):
    kw, text = VARIANCE[i]
    refused(lambda: renderer.denoise_variance(**kw), text)


@pytest.mark.parametrize("i", range(len(UPSAMPLE)))
def test_upsample(renderer, i):
    kw, text = UPSAMPLE[i]
    refused(lambda: renderer.upsample(**kw), text)


@pytest.mark.parametrize("rounds", [None, 2])
@pytest.mark.parametrize("i", range(len(SAMPLE_MAP)))
def test_sample_map(renderer, i, rounds):
    kw, text = SAMPLE_MAP[i]
    refused(lambda: renderer.sample_map(rounds=rounds, **kw), text)


@pytest.mark.parametrize("i", range(len(TEMPORAL)))
def test_temporal(rrt, renderer, i):
    kw, text = TEMPORAL[i]
    kw = dict(kw, cameras=cameras(rrt, kw.get("cameras", V)))
    refused(lambda: renderer.temporal(**kw), text)


@pytest.mark.parametrize("i", range(len(LIGHTMAP)))
def test_lightmap(rrt, i):
    from rust_ray_tracing_amd import _lib as L
    kw, text = LIGHTMAP[i]
    points = kw.get("points", N_TEXELS)
    kw = dict(kw, points=np.zeros(points, dtype=L.SURFACE_POINT) if isinstance(points, int) else points)
    refused(lambda: rrt.Scene.lightmap_filter(**kw), text)
    if "position" not in kw and "normal" not in kw:
        refused(lambda: rrt.Scene.lightmap_dilate(**kw), text)
        refused(lambda: rrt.Scene.lightmap_dilate(want_level=True, **kw), text)


@pytest.mark.parametrize("i", range(len(ADAPTIVE)))
def test_render_adaptive_counts(rrt, renderer, i):
    """``handle``: any value but None keeps the scene from being uploaded; every case is refused before it is used"""
    kw, text = ADAPTIVE[i]
    n = kw.get("cameras")
    kw = dict(kw, cameras=None if n is None else cameras(rrt, n))
    refused(lambda: renderer.render_adaptive(rrt.Scene(), handle=1, **kw), text)


def test_every_operator_has_its_cases():
    """per operator: an array mixed with a tensor, a wrong dtype, a wrong rank, a wrong extent, a host tensor as the anchor"""
    for table in (DENOISE, VARIANCE, UPSAMPLE, SAMPLE_MAP, TEMPORAL, LIGHTMAP):
        texts = [text for _, text in table]
        assert any(ALL in x for x in texts) and any("; got float64" in x for x in texts) and any("expected shape (" in x for x in texts)
    for table, anchor in ((DENOISE, "hdr"), (UPSAMPLE, "lo_hdr"), (SAMPLE_MAP, "variance"), (TEMPORAL, "hdr")):
        assert f"{anchor}: expected a float32 tensor on {anchor}'s device cpu" in [text for _, text in table]
    for table in (UPSAMPLE, TEMPORAL):
        assert any("expected uint32; got" in text for _, text in table)


def test_another_backend_is_refused(rrt):
    """the one refusal that is not a ValueError: every arm only this build has"""
    r = rrt.Renderer(rrt.RendererOptions(backend=rrt.RendererBackend.CPU, output_image_dimensions=(W, H), output_image_path="/dev/null"))
    text = "backend CPU is not part of this build; use RendererBackend.MI355X"
    calls = [lambda: r.render_buffers(rrt.Scene()), lambda: r.render_buffers_batch(rrt.Scene(), []), lambda: r.render_features(rrt.Scene()),
             lambda: r.render_motion(rrt.Scene()), lambda: r.render_denoised(rrt.Scene()),
             lambda: r.render_adaptive(rrt.Scene(), f(H, W, dtype=np.uint32)), lambda: next(r.render_sequence(rrt.Scene(), []))]
    for call in calls:
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == text
