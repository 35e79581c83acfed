"""-m gpu: the HIP path, called through the C ABI, against the CPU oracle on the same seeded inputs.
Bar: bit-exact f32 radiance (compared as u32), identical RGBA8, identical traversal counters."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _scene(rrt, kind, **kw):
    from rust_ray_tracing_amd import synth
    tris, mats, texs, cam = synth.make_scene(kind, **kw)
    sc = rrt.Scene.from_arrays(tris, mats, texs)
    sc.set_camera(rrt.Camera(position=cam[0], pitch=cam[1], yaw=cam[2]))
    return sc


CASES = [
    ("cornell", {}, 64, 64, 4, 16),
    ("cornell", {}, 61, 37, 3, 5),                                   # ragged 8x8 tiles
    ("helmet", dict(n_target=4000, tex_size=64), 96, 54, 4, 12),
    ("atrium", dict(n_target=60000, tex_size=64), 128, 72, 2, 16),
    ("dragon", dict(n_target=30000), 80, 48, 2, 64),                 # shipped max depth (main.rs:20)
]


@pytest.mark.parametrize("traversal,margin", [(0, 0.0), (1, 0.0), (1, 0.0078125)])
@pytest.mark.parametrize("kind,kw,w,h,spp,depth", CASES)
def test_hdr_bit_exact(rrt, orc, kind, kw, w, h, spp, depth, traversal, margin):
    sc = _scene(rrt, kind, **kw)
    r = rrt.Renderer.new(rrt.RendererOptions(samples=spp, max_ray_depth=depth, output_image_dimensions=(w, h),
                                             output_image_path="/dev/null", traversal=traversal, cull_margin=margin))
    hdr, rgba, st = r.render_buffers(sc, flags=rrt.FLAG_COUNT)
    ref, ref_rgba, rst = orc.render(sc.tris, sc.bvh_nodes, sc.materials_array(), sc.textures, sc.camera.uniform,
                                    w, h, spp, depth, cull=traversal, cull_margin=margin)
    assert st["pixels"] == w * h
    for k in ("rays", "inner_steps", "tri_tests", "hits", "texel_fetches", "max_stack"):
        assert st[k] == rst[k], k
    assert np.array_equal(hdr.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(rgba, ref_rgba)
    # the stated tolerance of the north star (RMSE <= 1e-4) is met with margin zero
    assert float(np.sqrt(np.mean((hdr.astype(np.float64) - ref) ** 2))) == 0.0


# ---- the product build of the trace kernel (flags = 0: COUNT = false) over whole small frames ------------------------------------------
# launch_trace has {COUNT} x {CULL} x {SHADING 0, 1} x {BATCH} instantiations, and the eight without COUNT are compiled under other
# launch bounds than their counting twins: other machine code.  Each is held to the oracle here over every pixel of a small frame with
# ragged tiles -- single view and a batch of three cameras, both traversals, both shading modes.  The product build fills no counters,
# so none are compared; the scheduling is whatever the library sets.
PRODUCT_CASES = {   # name -> (shading, width, height, samples, depth, camera box)
    "cornell": (0, 61, 37, 3, 5, 0.8),
    "helmet": (0, 96, 54, 4, 12, 4.0),
    "wgsl_pbr": (1, 96, 54, 3, 5, 14.0),
    "wgsl_glass": (1, 96, 54, 3, 16, 6.0),
}
_product_scenes, _product_refs = {}, {}


def _product_scene(rrt, case):
    """The scene and three distinct cameras (the scene's own first), built once per case."""
    if case not in _product_scenes:
        import os
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
        import wgsl_scenes as S
        if case == "cornell":
            sc = _scene(rrt, "cornell")
        elif case == "helmet":
            sc = _scene(rrt, "helmet", n_target=4000, tex_size=64)
        elif case == "wgsl_pbr":
            sc = S.pbr_scene(rrt, n_target=20000, tex_size=16)              # textures in all six slots
        else:
            sc = S.glass_scene(rrt, "dragon", 30000, ior=1.5)
        box = PRODUCT_CASES[case][5]
        own = sc.camera
        pos = np.array(own.position, dtype=np.float64)
        cams = [own,
                rrt.Camera(position=tuple(pos + box * np.array([0.3, 0.1, -0.2])), pitch=own.pitch + 12.0, yaw=own.yaw - 25.0),
                rrt.Camera(position=tuple(pos + box * np.array([-0.25, 0.15, 0.3])), pitch=own.pitch - 9.0, yaw=own.yaw + 40.0)]
        for c in cams[1:]:
            c.update_view()
        _product_scenes[case] = (sc, cams)
    return _product_scenes[case]


def _product_ref(orc, case, view, traversal, margin):
    """The oracle's render of one camera, computed once and shared."""
    key = (case, view, traversal)
    if key not in _product_refs:
        sc, cams = _product_scenes[case]
        shading, w, h, spp, depth, _ = PRODUCT_CASES[case]
        hdr, rgba, _ = orc.render(sc.tris, sc.bvh_nodes, sc.materials_array(), sc.textures, cams[view].uniform, w, h, spp, depth,
                                  cull=traversal, cull_margin=margin, shading=shading)
        _product_refs[key] = (hdr, rgba)
    return _product_refs[key]


def _same_bits(a, b):
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("traversal,margin", [(0, 0.0), (1, 0.0078125)])
@pytest.mark.parametrize("case", list(PRODUCT_CASES))
def test_product_kernels_whole_small_frames(rrt, orc, case, traversal, margin):
    shading, w, h, spp, depth, _ = PRODUCT_CASES[case]
    sc, cams = _product_scene(rrt, case)
    refs = [_product_ref(orc, case, v, traversal, margin) for v in range(3)]
    assert not _same_bits(refs[0][0], refs[1][0]) and not _same_bits(refs[0][0], refs[2][0]) and not _same_bits(refs[1][0], refs[2][0])
    r = rrt.Renderer.new(rrt.RendererOptions(samples=spp, max_ray_depth=depth, output_image_dimensions=(w, h), output_image_path="/dev/null",
                                             traversal=traversal, cull_margin=margin, shading=shading))
    hdr, rgba, _ = r.render_buffers(sc, flags=0)                          # pt_trace_kernel<false, CULL, SHADING>
    assert _same_bits(hdr, refs[0][0]), int(np.sum(hdr.view(np.uint32) != refs[0][0].view(np.uint32)))
    assert np.array_equal(rgba, refs[0][1])
    hdr_c, rgba_c, st = r.render_buffers(sc, flags=rrt.FLAG_COUNT)        # the counting twin: the same bits
    assert _same_bits(hdr_c, hdr) and np.array_equal(rgba_c, rgba) and st["pixels"] == w * h
    bhdr, brgba, _ = r.render_buffers_batch(sc, cams, flags=0)            # pt_trace_batch_kernel<false, CULL, SHADING>
    for v in range(3):
        assert _same_bits(bhdr[v], refs[v][0]), (v, int(np.sum(bhdr[v].view(np.uint32) != refs[v][0].view(np.uint32))))
        assert np.array_equal(brgba[v], refs[v][1]), v
    bhdr_c, brgba_c, st = r.render_buffers_batch(sc, cams, flags=rrt.FLAG_COUNT)
    assert _same_bits(bhdr_c, bhdr) and np.array_equal(brgba_c, brgba) and st["pixels"] == 3 * w * h
