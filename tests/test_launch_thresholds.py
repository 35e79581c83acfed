"""CPU: tests/tools/launch_thresholds.py keeps what it promises, from its own restatement of the host's rules: MID refills lanes under
leaf_period 1, FULL runs under leaf_period 4 with at most a quarter of the work in flight, FULL_F refills every first-hit lane more
than once -- for every occupancy the clamp allows, on small and large devices -- and the numbers DESIGN section 21 quotes for a
256-CU MI355X are the ones computed here."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import launch_thresholds as LT  # noqa: E402

N_CU = [1, 8, 256, 304]
OCC = list(range(1, LT.BLOCKS_PER_CU_CAP + 1))
FRAMES = [(61, 37), (96, 54), (24, 20)]                       # the views the GPU tests build their launches from


@pytest.mark.parametrize("n_cu", N_CU)
def test_thresholds_cross_what_they_name(n_cu):
    mid, full, full_f = LT.mid(n_cu), LT.full(n_cu), LT.full_f(n_cu)
    for occ in OCC:
        # MID: at most two blocks per CU, so fewer lanes than work items; below the period's threshold for every occupancy
        blocks = LT.trace_grid_blocks(n_cu, occ, mid)
        assert blocks <= 2 * n_cu and blocks * LT.BLOCK_LANES < mid
        assert mid < 4 * n_cu * occ * LT.BLOCK_LANES and LT.trace_leaf_period(n_cu, occ, mid) == 1
        LT.check_mid(n_cu, mid)
        # FULL: period 4, a quarter of the work in flight at most
        assert LT.trace_leaf_period(n_cu, occ, full) == 4 and LT.trace_leaf_period(n_cu, occ, full - LT.RAGGED - 1) == (4 if occ < 8 else 1)
        assert 4 * LT.trace_grid_blocks(n_cu, occ, full) * LT.BLOCK_LANES <= full
        LT.check_full(n_cu, full)
        # FULL_F: more than two items per lane
        assert 2 * LT.first_hit_grid_blocks(n_cu, occ, full_f) * LT.BLOCK_LANES < full_f
        LT.check_full_f(n_cu, full_f)
    # ragged tails: the work is no whole number of blocks, of grids or of lanes in flight
    for t in (full, full_f):
        assert t % LT.BLOCK_LANES == 64 and t % LT.lanes_cap(n_cu) == LT.RAGGED % LT.lanes_cap(n_cu) != 0


@pytest.mark.parametrize("n_cu", [256, 304])
@pytest.mark.parametrize("w,h", FRAMES)
def test_whole_views_stay_on_the_named_side(n_cu, w, h):
    """a launch is a whole number of views: rounding the threshold up to one must not carry MID past period 1 or past two blocks per CU
    (FULL and FULL_F only grow).  The GPU tests make the same three checks on their own device."""
    per = LT.view_work(w, h)
    for target, check in ((LT.mid(n_cu), LT.check_mid), (LT.full(n_cu), LT.check_full), (LT.full_f(n_cu), LT.check_full_f)):
        work = LT.views_for(target, w, h) * per
        assert target <= work < target + per
        check(n_cu, work)
    for occ in OCC:
        work = LT.views_for(LT.mid(n_cu), w, h) * per
        assert LT.trace_leaf_period(n_cu, occ, work) == 1 and LT.trace_grid_blocks(n_cu, occ, work) <= 2 * n_cu
    with pytest.raises(AssertionError):
        LT.check_mid(n_cu, 2 * n_cu * LT.BLOCK_LANES)             # every lane gets one item and none a second
    with pytest.raises(AssertionError):
        LT.check_mid(n_cu, 4 * n_cu * LT.BLOCK_LANES)             # period 4 at occ = 1
    with pytest.raises(AssertionError):
        LT.check_full(n_cu, LT.full(n_cu) - LT.RAGGED - 1)        # period 1 at occ = 8
    with pytest.raises(AssertionError):
        LT.check_full_f(n_cu, 2 * LT.lanes_cap(n_cu))


def test_numbers_quoted_in_the_design_document():
    assert (LT.mid(256), LT.full(256), LT.full_f(256)) == (196608, 2097152 + 4928, 1048576 + 4928) == (196608, 2102080, 1053504)
    assert LT.lanes_cap(256) == 524288 and 2 * 256 * LT.BLOCK_LANES == 131072
    assert LT.view_work(61, 37) == 2560 and LT.view_work(96, 54) == 5376 and LT.view_work(24, 20) == 576
    assert LT.views_for(LT.mid(256), 61, 37) == 77 and LT.views_for(LT.full(256), 61, 37) == 822
    assert LT.views_for(LT.mid(256), 96, 54) == 37 and LT.views_for(LT.full(256), 96, 54) == 392
    assert LT.views_for(LT.mid(256), 24, 20) == 342 and LT.views_for(LT.full(256), 24, 20) == 3650
    assert LT.views_for(LT.full_f(256), 61, 37) == 412
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "DESIGN.md"), encoding="utf-8").read()
    for quoted in ("196 608", "2 102 080", "1 053 504"):
        assert quoted in text, quoted
