"""The poisoned tier for the route field: twelve of tests/test_gpu_route_field.py in ONE fresh child process per fill byte
(tests/poisoned_child.py, GNDT_LIB_VARIANT = poison: every device and pinned host allocation filled with the byte before it is handed
out), for the two bytes of tests/test_gpu_poisoned.py.  What it is after: the first steps, the rest of the steps, the keys, the weights,
the "more" bits and the sweeps' flag words are cut out of one scratch area on every call; every one of them is written by a pass of the
call before a later pass reads it (the flag words by a memset) — a word that a pass reads before anything wrote it is 0 in a fresh
process and the byte here: 0xA5A5A5A5 as a flag word is "the sweep before changed something" for ever, as a key a cost no walk has,
as a weight a slope that costs -2.9e-16 to enter.  The host entry points' staging and the descent's records are in the group too.
The children run one at a time, each under the time limit below; a child that is killed at its limit, ends by a signal, with status 134
or 139, or reports an illegal memory access stops the tier: the case after it fails at once with "not started" and touches no GPU."""
import pytest

from tests import poison_tier

poison_tier.refuse_under_variant()

RF = "tests/test_gpu_route_field.py::"
# measured_s: the whole child (interpreter start to exit) on the MI355X under the regular library; limit_s: three times that, rounded
# up to 10 s (poison_malloc adds a fill and a device synchronisation to every allocation).
GROUP = dict(measured_s=8.85, limit_s=30, ids=[
    RF + "test_a_box_in_the_corridor_the_way_round_no_way_round_and_the_way_out",
    RF + "test_two_storeys_a_goal_on_the_bridge",
    RF + "test_lattices_at_the_slot_edges_and_the_limit_of_the_one_workgroup_kernel[1025]",
    RF + "test_lattices_at_the_slot_edges_and_the_limit_of_the_one_workgroup_kernel[20448]",
    RF + "test_lattices_at_the_slot_edges_and_the_limit_of_the_one_workgroup_kernel[20449]",
    RF + "test_descend_at_the_wavefront_and_grid_edges_of_K[65]",
    RF + "test_descend_a_short_cap_the_step_guard_to_the_step_and_a_corrupted_next",
    RF + "test_routes_go_straight_into_shortcut_routes",
    RF + "test_repeat_calls_a_side_stream_and_a_larger_call_first",
    RF + "test_first_builder_of_the_index_after_a_crop_and_after_an_update",
    RF + "test_outputs_are_optional_no_goals_and_out_of_sweeps",
    RF + "test_python_interface_rows_points_numpy_torch_and_streams",
])


def test_every_node_id_is_collected_and_the_limit_is_three_times_the_measured_time():
    assert len(GROUP["ids"]) == 12
    poison_tier.ids_collected(GROUP["ids"])
    poison_tier.limit_follows_rule(GROUP["measured_s"], GROUP["limit_s"])


@pytest.mark.gpu
@pytest.mark.parametrize("byte", poison_tier.BYTES, ids=poison_tier.BYTE_IDS)
def test_route_field_under_poison(byte):
    poison_tier.run_group("the route field", GROUP["ids"], GROUP["limit_s"], byte)
