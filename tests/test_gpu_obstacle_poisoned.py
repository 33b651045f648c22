"""The poisoned tier for the obstacle field: thirteen of tests/test_gpu_obstacle.py in ONE fresh child process per fill byte
(tests/poisoned_child.py, GNDT_LIB_VARIANT = poison: every device and pinned host allocation filled with the byte before it is handed
out), for the two bytes of tests/test_gpu_poisoned.py.  What it is after: the per-row marks (column stamps, worklist places, cover words)
are set to "never" once, when they are allocated, and stamped from then on; the worklist, the steps, the keys, the prefix sums and the
header are cut out of one scratch area on every call and written by the passes themselves, the second key array by round 1.  A word that
a pass reads before anything wrote it is 0 in a fresh process and the byte here — 0xA5A5A5A5 as a column stamp is "listed by a call far
in the future".  The group holds the reuse and the edge cases because they are the ones that read the per-row marks of earlier calls.
The children run one at a time, each under the time limit below; a child that is killed at its limit, ends by a signal, with status 134
or 139, or reports an illegal memory access stops the tier: the case after it fails at once with "not started" and touches no GPU."""
import pytest

from tests import poison_tier

poison_tier.refuse_under_variant()

OBS = "tests/test_gpu_obstacle.py::"
# measured_s: the whole child (interpreter start to exit) on the MI355X under the regular library; limit_s: three times that, rounded
# up to 10 s (poison_malloc adds a fill and a device synchronisation to every allocation).
GROUP = dict(measured_s=4.68, limit_s=20, ids=[
    OBS + "test_one_box_two_overlapping_boxes_and_the_inflation",
    OBS + "test_boxes_astride_the_seams_off_the_map_void_and_none",
    OBS + "test_the_count_on_the_device_and_both_strides_on_real_cluster_records",
    OBS + "test_the_budget_to_the_column",
    OBS + "test_rows_in_reach_and_window_columns_at_the_wave_and_workgroup_edges[63]",
    OBS + "test_rows_in_reach_and_window_columns_at_the_wave_and_workgroup_edges[257]",
    OBS + "test_deep_fields_a_base_in_place_and_the_pits_tall_column",
    OBS + "test_max_hops_of_one_and_of_1024_on_the_41_by_25_lattice[1024]",
    OBS + "test_base_merge_out_of_place_and_in_place_and_every_combination_of_null_outputs",
    OBS + "test_repeat_calls_streams_and_a_small_call_after_a_large_one",
    OBS + "test_first_builder_of_the_index_and_after_an_update_a_crop_and_a_clear",
    OBS + "test_segment_then_field_then_walk_and_shortcut_on_one_stream",
    OBS + "test_python_interface_numpy_torch_and_index_boxes",
])


def test_every_node_id_is_collected_and_the_limit_is_three_times_the_measured_time():
    assert len(GROUP["ids"]) == 13
    poison_tier.ids_collected(GROUP["ids"])
    poison_tier.limit_follows_rule(GROUP["measured_s"], GROUP["limit_s"])


@pytest.mark.gpu
@pytest.mark.parametrize("byte", poison_tier.BYTES, ids=poison_tier.BYTE_IDS)
def test_obstacle_field_under_poison(byte):
    poison_tier.run_group("the obstacle field", GROUP["ids"], GROUP["limit_s"], byte)
