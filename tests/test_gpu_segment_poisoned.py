"""The poisoned tier for scan segmentation: a handful of tests/test_gpu_segment.py in ONE fresh child process per fill byte
(tests/poisoned_child.py, GNDT_LIB_VARIANT = poison: every device and pinned host allocation filled with the byte before it is handed
out), for the two bytes of tests/test_gpu_poisoned.py.  What it is after: the call's cell table, the union-find's parents and the
roots' tallies are cut out of one scratch area on every call, cleared by three fills and otherwise written by the passes themselves; a
word that a pass reads before anything wrote it is 0 in a fresh process and the byte here.  The children run one at a time, each under
the time limit below; a child that is killed at its limit, ends by a signal, with status 134 or 139, or reports an illegal memory
access stops the tier: the case after it fails at once with "not started" and touches no GPU."""
import pytest

from tests import poison_tier

poison_tier.refuse_under_variant()

SEG = "tests/test_gpu_segment.py::"
# hand-drawn scans on the 16 x 16 floor, the count edges of every pass, the list's cut, every combination of null outputs and a small
# call after a large one on the same handle.  measured_s: the whole child (interpreter start to exit) on the MI355X under the regular
# library; limit_s: three times that, rounded up to 10 s (poison_malloc adds a fill and a device synchronisation to every allocation).
GROUP = dict(measured_s=4.17, limit_s=20, ids=[
    SEG + "test_one_box_is_one_cluster_with_known_cells_and_bounds",
    SEG + "test_corner_contact_links_under_26_and_not_under_6_and_a_gap_never",
    SEG + "test_the_three_keyed_classes_and_the_points_without_a_key",
    SEG + "test_serpentine_of_3000_cells_is_one_cluster[1]",
    SEG + "test_the_filters_change_exactly_what_the_restatement_says",
    SEG + "test_point_counts_at_the_wave_and_workgroup_edges[257]",
    SEG + "test_4096_points_in_one_cell_and_in_4096_cells",
    SEG + "test_cluster_counts_astride_the_list_tile[1025]",
    SEG + "test_a_short_list_is_cut_and_nothing_is_written_beyond",
    SEG + "test_every_combination_of_null_outputs_and_runs_of_equal_cells",
    SEG + "test_repeat_calls_streams_and_a_small_call_after_a_large_one",
])


def test_every_node_id_is_collected_and_the_limit_is_three_times_the_measured_time():
    poison_tier.ids_collected(GROUP["ids"])
    poison_tier.limit_follows_rule(GROUP["measured_s"], GROUP["limit_s"])


@pytest.mark.gpu
@pytest.mark.parametrize("byte", poison_tier.BYTES, ids=poison_tier.BYTE_IDS)
def test_segmentation_under_poison(byte):
    poison_tier.run_group("segmentation", GROUP["ids"], GROUP["limit_s"], byte)
