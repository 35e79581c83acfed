"""The uv panel (tests/tools/uv_panel.py) on the CPU: its uv assignment reaches what tests/test_gpu_uv_panel.py needs it to reach, seen
from the oracle / model side, and the texel model agrees with the oracle's renders of it.  No GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))

import features_model as F  # noqa: E402
import uv_panel as P  # noqa: E402


def test_panel_reaches_its_cases_and_model_counts_equal_the_oracles(rrt, orc):
    sc = P.scene(rrt)
    w, h = P.SIZE
    assert len(sc.tris) == 2 * P.NX * P.NY and [t.shape[:2] for t in sc.textures] == list(P.TEX_SHAPES)
    for t in sc.tris:                                                        # one (u, v) per triangle
        x, y = t["vertices"]["tex_coord_x"].view(np.uint32), t["vertices"]["tex_coord_y"].view(np.uint32)
        assert x[0] == x[1] == x[2] and y[0] == y[1] == y[2]
    frame, counters, _ = F.frame(orc, sc, sc.camera.uniform, w, h, 0)
    P.assert_coverage(sc, frame)
    per_tex, tot = P.first_hit_lookups(sc, frame)
    assert tot["fetches"] == counters["texel_fetches"]
    # the oracle's render of the first hits alone (1 sample, depth 1) counts the same fetches and the same clamps as the model
    _, _, st = orc.render(sc.tris, sc.bvh_nodes, sc.materials_array(), sc.textures, sc.camera.uniform, w, h, 1, 1)
    assert st["texel_fetches"] == tot["fetches"] and st["tex_clamped"] == tot["clamped"]
    # and the frame the GPU test renders clamps some lookups and not all, in both seed modes and from all three cameras
    for v, cam in enumerate(P.cameras(rrt)):
        for seed_mode in (0, 1):
            _, _, st = orc.render(sc.tris, sc.bvh_nodes, sc.materials_array(), sc.textures, cam.uniform, w, h, P.SPP, P.DEPTH, seed_mode=seed_mode)
            assert 0 < st["tex_clamped"] < st["texel_fetches"], st
            if v == 0:                                                       # scattered rays meet the panel again: deeper bounces are textured too
                assert st["hits"] > 1.1 * P.SPP * counters["hits"], st
