"""CPU: the numpy model of the count-aware temporal accumulation (tests/tools/temporal_counts_model.py) does what include/mipt.h states
for mipt_temporal_counts: a plane of ones is mipt_temporal byte for byte, a pixel without a sample neither reads hdr nor invents a
history, a tap that no sample has reached is rejected, the length counts samples up to max_history, the blend factor stays at most 1,
and the histories of the two models feed each other.  The kernel is held to this model in tests/test_gpu_temporal_counts.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import temporal_counts_model as TC  # noqa: E402
import temporal_model as T  # noqa: E402
import temporal_world as WD  # noqa: E402
from temporal_world import NEAR, SAME, SEQUENCE  # noqa: E402

F = np.float32
SIZE, VIEWS = (61, 37), 2
W, H = SIZE


def _plain(cams, p, history, albedo=True, **opts):
    return T.step(p["hdr"], p["position"], p["normal"], p["depth"], p["material"], cams, history, p["albedo"] if albedo else None,
                  **dict(T.DEFAULTS, **opts))


def _counted(cams, p, counts, cap, history, albedo=True, **opts):
    return TC.step(p["hdr"], p["position"], p["normal"], p["depth"], p["material"], cams, counts, cap, history,
                   p["albedo"] if albedo else None, **dict(T.DEFAULTS, **opts))


def _same(a, b, what):
    for k in ("out", "length", "variance"):
        assert T.same_bits(a[k], b[k]), (what, k)
    v, h, w = a["length"].shape
    assert T.same_history(a["history"], b["history"], v, h, w), (what, "history")


def _counts(shape, seed, values=(0, 1, 2, 3, 5, 9)):
    rng = np.random.default_rng(seed)
    c = rng.choice(np.array(values, dtype=np.uint32), size=shape)
    c[:, : shape[1] // 3, : shape[2] // 4] = 0                      # a block that is not traced at all
    return np.ascontiguousarray(c, dtype=np.uint32)


@pytest.mark.parametrize("opts", [dict(), dict(alpha_min=0.3, max_history=3.0), dict(alpha_min=1.0, max_history=1.0)], ids=["defaults", "floor", "ones"])
@pytest.mark.parametrize("albedo", [True, False])
def test_a_plane_of_ones_is_the_plain_accumulation(albedo, opts):
    """consequence (a), over temporal_model's own sequence (first frame, same camera, moved, turned away) and whatever the cap"""
    ones = np.ones((VIEWS, H, W), dtype=np.uint32)
    history = None
    reused = 0
    for f, move in enumerate(SEQUENCE):
        cams, p = WD.frame(SIZE, VIEWS, move, seed=f)
        want = _plain(cams, p, history, albedo, **opts)
        for cap in (1, 5, 65535):
            _same(_counted(cams, p, ones, cap, history, albedo, **opts), want, (f, cap))
        _same(_counted(cams, p, np.full_like(ones, 7), 1, history, albedo, **opts), want, (f, "capped to one"))
        reused += int((want["cls"] >= T.REUSED4).sum())
        history = want["history"]
    assert reused > VIEWS * W * H


def test_a_pixel_without_a_sample():
    """n == 0 does not read hdr (a NaN there changes nothing); with a history it is reprojected as it is, without one it holds +0 and a
    length of 0"""
    cams0, p0 = WD.frame(SIZE, VIEWS, SAME)
    first = _counted(cams0, p0, np.full((VIEWS, H, W), 3, dtype=np.uint32), 5, None)
    assert np.all(first["length"] == 3)
    cams, p = WD.frame(SIZE, VIEWS, NEAR, seed=2)
    counts = _counts((VIEWS, H, W), 1)
    want = _counted(cams, p, counts, 5, first["history"])
    poisoned = dict(p, hdr=np.where((counts == 0)[..., None], F(np.nan), p["hdr"]).astype(F))
    got = _counted(cams, poisoned, counts, 5, first["history"])
    _same(got, want, "NaN under the zeros")
    zero = counts == 0
    kept, lost = zero & want["reuse"], zero & ~want["reuse"]
    assert kept.sum() > 50 and lost.sum() > 5 and not np.isnan(got["out"][zero]).any()
    assert np.all(want["length"][lost] == 0) and np.all(want["variance"][lost] == 0)
    assert not want["out"][lost].view(np.uint32).any()              # +0, bit for bit
    _, h0, _, h2 = T.unpack_history(want["history"], VIEWS, H, W)
    assert not h0[lost].view(np.uint32).any() and not h2[lost][:, :2].any()
    # pure reprojection: the length is the gathered one (3 up to the roundings of sl / sw), not one more
    assert np.all(np.abs(want["length"][kept] - 3.0) < 1e-3)
    traced = (counts > 0) & want["reuse"]
    n = np.minimum(counts, 5).astype(F)
    assert np.all(np.abs(want["length"][traced] - (3 + n[traced])) < 1e-3)
    # the first frame: nothing to reproject
    start = _counted(cams, poisoned, counts, 5, None)
    assert np.all(start["length"] == np.minimum(counts, 5)) and not start["out"][zero].view(np.uint32).any()


def test_a_tap_no_sample_has_reached_is_rejected():
    """one of a pixel's four taps has len = 0 (and a NaN colour, which any weight would spread): the other three are renormalised by
    their own sw"""
    cams0, p0 = WD.frame(SIZE, 1, SAME)
    history = _plain(cams0, p0, None)["history"].copy()
    cams, p = WD.frame(SIZE, 1, NEAR, seed=2)
    ones = np.ones((1, H, W), dtype=np.uint32)
    base = _counted(cams, p, ones, 1, history, albedo=False)
    ys, xs = np.nonzero(base["taps"][0] == 4)
    rec, h0, h1, h2 = T.unpack_history(history, 1, H, W)
    _, _, fx, fy, _ = T.project(p["position"][0], rec[0], W, H)
    k = len(ys) // 2
    y, x = int(ys[k]), int(xs[k])
    x0, y0 = int(np.floor(fx[y, x])), int(np.floor(fy[y, x]))
    wx, wy = fx[y, x] - np.floor(fx[y, x]), fy[y, x] - np.floor(fy[y, x])
    assert wx > 0.02 and wy > 0.02
    h0[0, y0, x0] = (np.nan, np.nan, np.nan, 0.0)
    got = _counted(cams, p, ones, 1, history, albedo=False)
    assert got["taps"][0, y, x] == 3 and got["reuse"][0, y, x] and np.isfinite(got["out"][0, y, x]).all()
    ox, oy = F(1.0) - wx, F(1.0) - wy
    sw, s, sl = F(0.0), np.zeros(3, dtype=F), F(0.0)
    for qx, qy, wt in ((x0 + 1, y0, wx * oy), (x0, y0 + 1, ox * wy), (x0 + 1, y0 + 1, wx * wy)):
        sw = sw + wt
        s = s + (wt * h0[0, qy, qx, :3])
        sl = sl + (wt * h0[0, qy, qx, 3])
    cp, lp = s / sw, sl / sw
    ln = lp + F(1.0)
    al = F(1.0) / ln
    cc = p["hdr"][0, y, x]
    assert T.same_bits(got["out"][0, y, x], cp + ((cc - cp) * al)) and got["length"][0, y, x] == ln
    # a NaN length is rejected like a zero
    h0[0, y0, x0, 3] = np.nan
    again = _counted(cams, p, ones, 1, history, albedo=False)
    assert T.same_bits(again["out"][0, y, x], got["out"][0, y, x]) and again["taps"][0, y, x] == 3


def test_the_length_counts_samples_up_to_max_history():
    cams, p = WD.frame(SIZE, VIEWS, SAME)
    history, top = None, 0.0
    for f in range(5):
        counts = _counts((VIEWS, H, W), 10 + f)
        r = _counted(cams, p, counts, 9, history, max_history=6.0)
        assert float(np.nanmax(r["length"])) <= 6.0
        top = max(top, float(r["length"].max()))
        history = r["history"]
    assert top == 6.0


def test_the_blend_factor_stops_at_one():
    """nf = 9 against max_history = 4: nf / ln = 2.25 without the clamp; with it the frame is what alpha_min = 1 gives"""
    cams0, p0 = WD.frame(SIZE, VIEWS, SAME)
    history = _plain(cams0, p0, None)["history"]
    cams, p = WD.frame(SIZE, VIEWS, NEAR, seed=2)
    nine = np.full((VIEWS, H, W), 9, dtype=np.uint32)
    got = _counted(cams, p, nine, 9, history, max_history=4.0)
    want = _counted(cams, p, nine, 9, history, max_history=4.0, alpha_min=1.0)
    _same(got, want, "al = 1")
    assert got["reuse"].sum() > 0.3 * got["reuse"].size and np.all(got["length"][got["reuse"]] == 4.0)
    # al = 1 puts this frame's colour in the history's place, up to the roundings of cp + ((cc - cp) * 1) with cp below 4 / 0.02
    assert np.allclose(got["out"][got["reuse"]], p["hdr"][got["reuse"]], rtol=0.0, atol=1e-4)
    assert not np.allclose(_counted(cams, p, np.ones_like(nine), 9, history, max_history=4.0)["out"][got["reuse"]], p["hdr"][got["reuse"]], atol=1e-2)


def test_the_two_histories_feed_each_other():
    """consequence (b)"""
    cams0, p0 = WD.frame(SIZE, VIEWS, SAME)
    cams, p = WD.frame(SIZE, VIEWS, NEAR, seed=2)
    ones = np.ones((VIEWS, H, W), dtype=np.uint32)
    plain = _plain(cams0, p0, None)["history"]
    counted = _counted(cams0, p0, _counts((VIEWS, H, W), 3, values=(1, 2, 3, 5)), 5, None)["history"]
    _same(_counted(cams, p, ones, 4, plain), _plain(cams, p, plain), "counts after plain")
    a = _plain(cams, p, counted)                                    # a history in samples read by the plain blend: one more
    b = _counted(cams, p, ones, 4, counted)
    v, h, w = a["length"].shape
    # the traced block of zeros in `counted` has len 0: the plain entry takes such a tap, the counting one rejects it -- elsewhere equal
    _, c0, _, _ = T.unpack_history(counted, VIEWS, H, W)
    assert (c0[..., 3] == 0).any()
    full = b["taps"] == 4
    assert full.sum() > 100 and T.same_bits(a["out"][full], b["out"][full]) and T.same_bits(a["length"][full], b["length"][full])


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_a_uniform_plane_on_a_static_camera_counts_k_per_frame(k):
    """identity camera over the plane z = 1, W and H powers of two: every pixel reprojects onto itself with one tap of weight 1"""
    w, h = 8, 4
    cam = np.zeros((), dtype=WD.CAMERA)
    cam["look_at"] = np.eye(4, dtype=F)
    xs, ys = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
    sx = (((xs / F(w)) * 2) - 1) * F(w / h)
    sy = (((F(h) - ys) / F(h)) * 2) - 1
    position = np.stack([-sx, sy, np.ones_like(sx)], axis=-1).astype(F)
    depth = np.sqrt((position ** 2).sum(-1)).astype(F)
    normal = np.zeros((h, w, 3), dtype=F)
    normal[..., 2] = -1.0
    material = np.full((h, w), 3, dtype=np.uint32)
    hdr = (np.random.default_rng(5).random((h, w, 3)) * 3.0).astype(F)
    counts = np.full((h, w), k, dtype=np.uint32)
    history = None
    for f in range(1, 9):
        r = TC.step(hdr, position, normal, depth, material, [cam], counts, 8, history, None, alpha_min=0.0, max_history=11.0)
        assert np.all(r["length"] == min(k * f, 11)), (k, f)
        assert np.array_equal(r["out"].view(np.uint32), hdr.view(np.uint32)) and np.all(r["variance"] == 0)
        history = r["history"]
