"""The poisoned tier: the map's consumers on memory that does not start out as zeros.

A fresh process gets zeroed pages from hipMalloc and hipHostMalloc, and every GPU test builds a small map on a fresh handle in a fresh
process: memory the library forgot to initialise reads as 0 there and the answer comes out right.  The poisoned variant of the library
(grid_ndt_amd/_lib.py VARIANTS, -DGNDT_POISON, gndt_handle.hpp) fills every device and pinned host allocation with one byte before it
hands it out.  Two bytes: 0xA5 is 2 779 096 485 as a uint32, which breaks indices, counts and flags, but -2.87e-16 as a float, which a
sum survives; 0x7F is 3.40e38 as a float, 1.38e306 as a double and 2 139 062 143 as an int, and none of the library's sentinels (0xFF
would be kNoRow / kEmptyKey / kNoColumn; 0x00 is the fresh process).

CPU tier: the variant cross-compiles and exports the whole boundary, the product refuses the variant's option and counter, and every
node id of GROUPS below exists.  GPU tier: group x byte, each case ONE fresh child process (tests/poisoned_child.py, GNDT_LIB_VARIANT =
poison) that runs the group's existing tests in-process — their references are theirs — and reports how many bytes it poisoned.  The
children run one at a time, each under its group's time limit.  A child that is killed at its limit, ends by a signal, with status 134
or 139, or reports an illegal memory access stops the tier: every case after it fails at once with "not started" and touches no GPU.

The groups: the build, the geometric consumers, the statistical ones, the flood and what runs on it, and "reach" — the clearance field
and the path walks, whose scratch is cut into regions by the row count on every call and whose flag words and key slots are cleared
only in part (tests/test_gpu_clearance.py, tests/test_gpu_walk.py: the hand-drawn maps and the lattices of up to 1025 rows).

The group "blocked" is the blocked bucket kernel (gndt_blocked.hpp) reached with 131 072-point boxes through the lowered floor
(tests/test_gpu_blocked_small.py): three block shapes, four fuzzed boxes and the layout's lifetime on one handle — Part::raw, the
order arrays, the buckets' ranges, both cursor levels, the extent words of blocked_decide, the re-run after a miss and the one after the
staging rows ran out, on poisoned memory.  Its large-then-small test stays out: a 1.1 M-point build would spend the child's time in
poison_malloc's fills.

The group "stream" is the scripted handle lives of tests/test_gpu_stream_sequences.py: change2DMap, del2DMap, deferred emit,
table and word growth in mid-stream, reserve, crop, clear, merge and the statistics round trip on one handle after the other — the
eight arrays alloc_table does not clear, the order arrays and the staging rows behind every kind of finalisation.

The group "owner" is the owner-partitioned build through its steps on W handles of one device (tests/test_gpu_owner.py: the tiny clouds
with ranks that own nothing, and a 3 000-point hash-owned build on the handles of a 60 000-point locality build).  The threads
communicator and RCCL stay out: poison_malloc synchronises the whole device on every allocation, and several rank threads share it.

hipGraph capture and replay are not in the groups: capture refuses allocation, and tools/fuzz_graph.py owns that ground."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from tests import poison_tier
from tests.poison_tier import ROOT
from tests.poison_tier import env as _env

poison_tier.refuse_under_variant()

REUSE = "tests/test_gpu_scratch_reuse.py::"
CLEARANCE = "tests/test_gpu_clearance.py::"
WALK = "tests/test_gpu_walk.py::"
BLOCKED_SMALL = "tests/test_gpu_blocked_small.py::"
STREAM = "tests/test_gpu_stream_sequences.py::"
OWNER = "tests/test_gpu_owner.py::"
# Existing GPU tests whose maps are hand-drawn or hold at most 60 000 points, that assert no wall-clock bound and record no hipGraph, and
# the large-then-small tests of tests/test_gpu_scratch_reuse.py in the group of their consumer.  The bound on the points keeps a child
# short — poison_malloc fills and synchronises on every allocation, and a build's buffers grow with its cloud — and is no rule about
# the maps: the 121 x 121 lattice of the reuse tests of "reach" has 131 770 points, one column each, builds in well under a second and
# is admitted.  The site, the bridge, the 9216- and 9217-row lattices and the grid-stride cases stay out of "reach".
# measured_s: the whole child (interpreter start to exit) on the MI355X under the regular library; limit_s: three times that, rounded up
# to 10 s (poison_malloc adds a fill and a device synchronisation to every allocation).
GROUPS = {
    "build": dict(measured_s=4.14, limit_s=20, ids=[
        "tests/test_gpu_fuzz.py::test_single_points_and_tiny_clouds",
        "tests/test_gpu_fuzz.py::test_interleaved_nodes_inside_a_wave[abab]",
        "tests/test_gpu_fuzz.py::test_interleaved_nodes_inside_a_wave[runs]",
        "tests/test_gpu_fuzz.py::test_interleaved_nodes_inside_a_wave[abcabc_plus_padding]",
        "tests/test_gpu_fuzz.py::test_random_structured_clouds_every_strategy[0]",
        "tests/test_gpu_fuzz.py::test_random_structured_clouds_every_strategy[1]",
        "tests/test_gpu_fuzz.py::test_random_structured_clouds_every_strategy[2]",
        "tests/test_gpu_fuzz.py::test_random_structured_clouds_every_strategy[3]",
        "tests/test_gpu_parity.py::test_edge_inputs",
    ]),
    "geometry": dict(measured_s=4.42, limit_s=20, ids=[
        REUSE + "test_query[1]",
        REUSE + "test_query[4]",
        REUSE + "test_raster",
        REUSE + "test_clear",
        REUSE + "test_cast[voxel]",
        REUSE + "test_cast[ndt]",
        REUSE + "test_crop",
    ]),
    "statistics": dict(measured_s=5.89, limit_s=20, ids=[
        "tests/test_gpu_score.py::test_scores_equal_the_restatement[uniform_box-1]",
        "tests/test_gpu_score.py::test_scores_equal_the_restatement[uniform_box-2]",
        "tests/test_gpu_score.py::test_scores_equal_the_restatement[uniform_box-5]",
        "tests/test_gpu_score.py::test_scores_equal_the_restatement[uniform_box-0]",
        "tests/test_gpu_score_derivs.py::test_derivs_equal_the_restatement[uniform_box-1]",
        "tests/test_gpu_score_derivs.py::test_derivs_equal_the_restatement[uniform_box-2]",
        "tests/test_gpu_score_derivs.py::test_derivs_equal_the_restatement[uniform_box-5]",
        "tests/test_gpu_score_derivs.py::test_derivs_equal_the_restatement[uniform_box-0]",
        "tests/test_gpu_coarsen.py::test_smallest_shapes",
        "tests/test_gpu_coarsen.py::test_after_remove_crop_and_clear",
        "tests/test_gpu_merge.py::test_smallest_shapes",
        "tests/test_gpu_merge.py::test_a_small_destination_table_grows",
        "tests/test_gpu_merge.py::test_a_general_pose_against_the_restatement",
        REUSE + "test_score",
        REUSE + "test_score_derivs",
        REUSE + "test_score_maps",
        REUSE + "test_coarsen",
        REUSE + "test_merge",
    ]),
    "flood": dict(measured_s=4.57, limit_s=20, ids=[
        "tests/test_gpu_cost.py::test_cost_map_goal_statuses_and_lifetime",
        "tests/test_gpu_plan.py::test_floor_all_1600_starts_in_one_call",
        "tests/test_gpu_plan.py::test_capped_lds_tier_spills_and_gives_the_same_bytes",
        "tests/test_gpu_frontiers.py::test_floor_ring_corners_and_nothing",
        "tests/test_gpu_frontiers.py::test_serpentine_is_one_cluster_in_any_row_order[None]",
        "tests/test_gpu_frontiers.py::test_serpentine_is_one_cluster_in_any_row_order[1]",
        "tests/test_gpu_frontiers.py::test_serpentine_is_one_cluster_in_any_row_order[2]",
        "tests/test_gpu_frontiers.py::test_serpentine_is_one_cluster_in_any_row_order[3]",
        "tests/test_gpu_frontiers.py::test_two_storeys",
        REUSE + "test_cost_flood[1]",
        REUSE + "test_cost_flood[0]",
        REUSE + "test_plan",
        REUSE + "test_frontiers[reached]",
        REUSE + "test_frontiers[slopes]",
    ]),
    "reach": dict(measured_s=6.83, limit_s=30, ids=[
        CLEARANCE + "test_corridor_between_plateaus",
        CLEARANCE + "test_two_storeys_do_not_see_each_other",
        CLEARANCE + "test_a_low_ceiling_is_a_barrier_for_the_robot_it_is_too_low_for",
        CLEARANCE + "test_a_step_through_a_pit_column_taller_than_the_step_mask",
        CLEARANCE + "test_outputs_are_optional_and_nothing_is_written_beyond_the_rows",
        CLEARANCE + "test_lattices_at_the_slot_edges_and_the_limit_of_the_one_workgroup_kernel[1023-64]",
        CLEARANCE + "test_lattices_at_the_slot_edges_and_the_limit_of_the_one_workgroup_kernel[1023-1]",
        CLEARANCE + "test_lattices_at_the_slot_edges_and_the_limit_of_the_one_workgroup_kernel[1024-64]",
        CLEARANCE + "test_lattices_at_the_slot_edges_and_the_limit_of_the_one_workgroup_kernel[1024-1]",
        CLEARANCE + "test_lattices_at_the_slot_edges_and_the_limit_of_the_one_workgroup_kernel[1025-64]",
        CLEARANCE + "test_lattices_at_the_slot_edges_and_the_limit_of_the_one_workgroup_kernel[1025-1]",
        CLEARANCE + "test_max_hops_of_one_the_limit_the_depth_one_less_and_an_odd_one_behind_it",
        WALK + "test_corridor_along_across_and_out_of_the_end",
        WALK + "test_a_step_through_a_pit_column_taller_than_the_step_mask",
        WALK + "test_two_storeys_least_dz_and_a_tie_to_the_smaller_row[low]",
        WALK + "test_two_storeys_least_dz_and_a_tie_to_the_smaller_row[high]",
        WALK + "test_a_low_ceiling_stops_the_walk_only_when_asked",
        WALK + "test_lattice_corners_zero_length_segments_and_the_codecs_edge",
        WALK + "test_wave_and_workgroup_edges_of_K_terminators_and_strides[65-33-4]",
        WALK + "test_wave_and_workgroup_edges_of_K_terminators_and_strides[64-1-3]",
        WALK + "test_hops_and_min_hops_against_a_real_clearance_field",
        WALK + "test_the_default_table_choice_at_its_threshold_to_the_row",
        REUSE + "test_clearance[1]",
        REUSE + "test_clearance[0]",
        REUSE + "test_walk[1]",
        REUSE + "test_walk[0]",
        REUSE + "test_clearance_then_walk_share_nothing",
    ]),
    "blocked": dict(measured_s=5.23, limit_s=20, ids=[
        BLOCKED_SMALL + "test_every_block_shape_small[flat_1-slope]",
        BLOCKED_SMALL + "test_every_block_shape_small[levels_4_at_interval-slope]",
        BLOCKED_SMALL + "test_every_block_shape_small[levels_32_moved_origin-slope]",
        BLOCKED_SMALL + "test_fuzzed_boxes[108]",
        BLOCKED_SMALL + "test_fuzzed_boxes[133]",
        BLOCKED_SMALL + "test_fuzzed_boxes[142]",
        BLOCKED_SMALL + "test_fuzzed_boxes[232]",
        BLOCKED_SMALL + "test_staging_rows_run_out_inside_a_small_blocked_build",
        BLOCKED_SMALL + "test_layout_lifetime_on_one_handle",
    ]),
    "stream": dict(measured_s=6.53, limit_s=20, ids=[
        STREAM + "test_script[small_then_stream]",
        STREAM + "test_script[small_seen_then_tails]",
        STREAM + "test_script[small_seen_each_tail]",
        STREAM + "test_script[deferred_crossings]",
        STREAM + "test_script[growth_and_reserve]",
        STREAM + "test_script[rebuild_between]",
        STREAM + "test_script[to_empty_and_back]",
        STREAM + "test_script[merge_and_stats]",
    ]),
    "owner": dict(measured_s=7.40, limit_s=30, ids=[
        OWNER + "test_owner_build_of_tiny_clouds_with_ranks_that_own_nothing[1-2]",
        OWNER + "test_owner_build_of_tiny_clouds_with_ranks_that_own_nothing[7-4]",
        OWNER + "test_owner_build_of_tiny_clouds_with_ranks_that_own_nothing[300-8]",
        OWNER + "test_owner_build_of_tiny_clouds_with_ranks_that_own_nothing[5000-3]",
        OWNER + "test_a_small_hash_owned_build_on_the_handles_of_a_large_locality_build",
    ]),
}


# ---- CPU tier --------------------------------------------------------------------------------------------------------------------------

def test_variant_cross_compiles_for_gfx950_and_exports_every_declared_symbol(native_lib):
    from grid_ndt_amd import _lib
    path = _lib.build_native(variant="poison")
    assert path == _lib.lib_path("poison") == os.path.join(ROOT, "grid_ndt_amd", "csrc", "libgndt_poison.so") and os.path.exists(path)
    assert path != native_lib._name and _lib.LIB_PATH == native_lib._name       # this process itself runs on the product
    with open(path, "rb") as f:
        assert b"gfx950" in f.read()
    # the rest in a process of its own that runs on the variant: the whole boundary is there (lib() binds it, symbol by symbol), and
    # the option and the counter are the variant's.  No device is touched by either.
    code = """
import ctypes as C
import grid_ndt_amd as g
from grid_ndt_amd import _lib
from tests.test_abi import declared_symbols
L = _lib.lib()
assert L._name == _lib.LIB_PATH == _lib.lib_path("poison")
syms = declared_symbols()
assert "gndt_debug_poisoned_bytes" in syms
raw = C.CDLL(L._name)
missing = [s for s in syms if not hasattr(raw, s)]
assert not missing, missing
T = g.TwoDmap
for value, ok in ((0x7F, True), (0, True), (255, True), (0xA5, True), (256, False), (-1, False), (1.5, False), (float("nan"), False)):
    try:
        T.set_debug_option(T.DEBUG_POISON_BYTE, value)
        assert ok, value
    except g.GndtError as e:
        assert not ok and e.code == 1, value
assert T.poisoned_bytes() == (0, 0)
h = C.c_uint64(9)
assert L.gndt_debug_poisoned_bytes(None, C.byref(h)) == 1 and h.value == 9
print("variant ok")
"""
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=_env("poison"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("variant ok"), (r.stdout[-1000:], r.stderr[-2000:])


def test_the_product_refuses_the_poison_byte_and_the_counter(native_lib):
    import grid_ndt_amd as g
    T = g.TwoDmap
    assert T.DEBUG_POISON_BYTE == 7
    for value in (0xA5, 0x7F, 0):
        with pytest.raises(g.GndtError) as e:
            T.set_debug_option(T.DEBUG_POISON_BYTE, value)
        assert e.value.code == 1          # GNDT_ERR_INVALID
    with pytest.raises(g.GndtError) as e:
        T.poisoned_bytes()
    assert e.value.code == 1
    d, h = C.c_uint64(7), C.c_uint64(9)
    assert native_lib.gndt_debug_poisoned_bytes(C.byref(d), C.byref(h)) == 1 and (d.value, h.value) == (7, 9)


def test_the_variant_is_chosen_by_the_environment_in_python_only():
    """GNDT_LIB_VARIANT is read by grid_ndt_amd/_lib.py: unset or empty the product, "poison" the variant, anything else refused"""
    code = "from grid_ndt_amd import _lib; print(_lib.VARIANT, _lib.LIB_PATH)"
    for value, want in ((None, "None " + os.path.join(ROOT, "grid_ndt_amd", "csrc", "libgndt.so")),
                        ("", "None " + os.path.join(ROOT, "grid_ndt_amd", "csrc", "libgndt.so")),
                        ("poison", "poison " + os.path.join(ROOT, "grid_ndt_amd", "csrc", "libgndt_poison.so"))):
        env = _env()
        if value is not None:
            env["GNDT_LIB_VARIANT"] = value
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr[-500:])
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=_env("poisson"), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "GNDT_LIB_VARIANT" in r.stderr


def test_every_node_id_of_the_groups_is_collected():
    poison_tier.ids_collected([i for grp in GROUPS.values() for i in grp["ids"]])


def test_the_limits_are_three_times_the_measured_times():
    for grp in GROUPS.values():
        poison_tier.limit_follows_rule(grp["measured_s"], grp["limit_s"])


# ---- GPU tier --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("byte", poison_tier.BYTES, ids=poison_tier.BYTE_IDS)
@pytest.mark.parametrize("group", list(GROUPS))
def test_group_under_poison(group, byte):
    poison_tier.run_group(group, GROUPS[group]["ids"], GROUPS[group]["limit_s"], byte)
