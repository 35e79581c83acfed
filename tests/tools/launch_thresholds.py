"""The sizes at which the persistent kernels (pt_trace_batch_kernel, pt_trace_adaptive_kernel, first_hit_kernel and its motion forms)
change their schedule, restated from the host code that sets them.  A launch holds a fixed number of lanes, and each lane takes work
items from a queue until it is dry; the tests that use this module cross the thresholds by the size of their input, computed from the
device at run time, and force nothing.  Edit together with:

* render_launch, csrc/mipt_api.cpp ("Small shards ..." and "Leaf phases ...") and its twin in csrc/mipt_adaptive.cpp: the trace grid is
  n_cu x min(occ, max(2, floor(work / (1.25 n_cu 256)))) blocks of 256 lanes, at most ceil(work / 256) (traversal_grid,
  csrc/mipt_scene.h); leaf_period = 4 iff work >= 4 n_cu occ 256, else 1; work = ceil(w / 8) ceil(h / 8) 64 n_views.
* trace_blocks_per_cu / trace_adaptive_blocks_per_cu, csrc/pt_kernel.hip: occ is the occupancy query's answer clamped to 1 ... 8.
* first_hit_setup, csrc/mipt_features.cpp: the feature and motion grid is n_cu x blocks_per_cu blocks, at most ceil(work / 256);
  first_hit_blocks_per_cu and motion_blocks_per_cu (csrc/first_hit.hip) clamp to 1 ... 8 as well -- checked: the same two lines.
* query_blocks_per_cu (csrc/ray_query.hip), the same clamp: tests/test_gpu_query.py::_launch_capacity is this module's lanes_cap.
* grid_for, csrc/bake.hip: every baking launch but cover_huge_kernel is capped at n_cu x 8 blocks of kT = 256 lanes and walks the rest
  of its input with a grid-stride loop -- not persistent, but the same number: lanes_cap(n_cu) is the most triangles, texels, records,
  points or paths a bake launch holds before a lane takes a second one.  (cover_huge_kernel launches n_cu x 4 blocks: half of it.)

tests/test_launch_thresholds.py (CPU) asserts what the names below promise, from these formulas alone."""

BLOCK_LANES = 256                        # kBlockThreads
BLOCKS_PER_CU_CAP = 8                    # the clamp of every *_blocks_per_cu
RAGGED = 77 * 64                         # 77 tiles: no multiple of a block, of a grid or of any view used


def device_n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def lanes_cap(n_cu):
    """the most lanes any of these launches holds in flight, whatever the occupancy query says"""
    return n_cu * BLOCKS_PER_CU_CAP * BLOCK_LANES


def mid(n_cu):
    """trace work items: the grid is at most 2 n_cu blocks, so lanes refill (1.5 items per lane or more); leaf_period = 1"""
    return 3 * n_cu * BLOCK_LANES


def full(n_cu):
    """trace work items: leaf_period = 4 whatever the occupancy, at most a quarter of the work in flight, a ragged tail"""
    return 4 * lanes_cap(n_cu) + RAGGED


def full_f(n_cu):
    """first-hit work items: more than twice the lanes in flight, so every lane refills more than once; a ragged tail"""
    return 2 * lanes_cap(n_cu) + RAGGED


def view_work(w, h):
    """work items of one view: whole 8x8 tiles, the ragged edge included"""
    return ((w + 7) // 8) * ((h + 7) // 8) * 64


def views_for(target, w, h):
    """the fewest views of w x h whose work reaches `target`"""
    per = view_work(w, h)
    return (target + per - 1) // per


# ---- the host's rules, for the CPU test and for messages ----------------------------------------------------------------------------
def trace_grid_blocks(n_cu, occ, work):
    fit = work // int(1.25 * n_cu * BLOCK_LANES)
    bpc = min(occ, max(2, fit))
    return max(1, min(n_cu * bpc, (work + BLOCK_LANES - 1) // BLOCK_LANES))


def trace_leaf_period(n_cu, occ, work):
    return 4 if work >= 4 * n_cu * occ * BLOCK_LANES else 1


def first_hit_grid_blocks(n_cu, bpc, work):
    return max(1, min(n_cu * bpc, (work + BLOCK_LANES - 1) // BLOCK_LANES))


# ---- what a test asserts of the work it is about to launch, whatever occupancy the library will find -------------------------------
def check_mid(n_cu, work):
    occs = range(1, BLOCKS_PER_CU_CAP + 1)
    assert all(trace_grid_blocks(n_cu, occ, work) * BLOCK_LANES * 3 <= work * 2 for occ in occs), (n_cu, work)   # >= 1.5 items per lane
    assert all(trace_leaf_period(n_cu, occ, work) == 1 for occ in occs), (n_cu, work)


def check_full(n_cu, work):
    occs = range(1, BLOCKS_PER_CU_CAP + 1)
    assert all(trace_leaf_period(n_cu, occ, work) == 4 for occ in occs), (n_cu, work)
    assert all(4 * trace_grid_blocks(n_cu, occ, work) * BLOCK_LANES <= work for occ in occs), (n_cu, work)


def check_full_f(n_cu, work):
    assert all(2 * first_hit_grid_blocks(n_cu, bpc, work) * BLOCK_LANES < work for bpc in range(1, BLOCKS_PER_CU_CAP + 1)), (n_cu, work)
