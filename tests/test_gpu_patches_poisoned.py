"""The poisoned tier for surface patches: a handful of tests/test_gpu_patches.py in ONE fresh child process per fill byte
(tests/poisoned_child.py, GNDT_LIB_VARIANT = poison: every device and pinned host allocation filled with the byte before it is handed
out), for the two bytes of tests/test_gpu_poisoned.py.  What it is after: the union-find's parents and member counts, the listed
patches' ten fp64 sums and the tile counts live in a scratch area of the handle that nothing clears, and the host-pointer entry point's
labels, records and counts come back from a staging area that nothing clears either — a parent, a sum or a record field that a kernel
leaves unwritten is 0 in a fresh process and the byte here (0x7F: 1.38e306 as a double, which no plane survives), and the restatement
has neither.  The children run one at a time, each under the time limit below; a child that is killed at its limit, ends by a signal,
with status 134 or 139, or reports an illegal memory access stops the tier: the case after it fails at once with "not started" and
touches no GPU."""
import pytest

from tests import poison_tier

poison_tier.refuse_under_variant()

PATCHES = "tests/test_gpu_patches.py::"
# the hand scene through both entry points with labels on and off and counts only (one build path), the checkerboard's truncated lists
# and min_size through both, the storeys' planes, the boxed U, and the calls after a larger call.  measured_s: the whole child
# (interpreter start to exit) on the MI355X under the regular library; limit_s: three times that, rounded up to 10 s (poison_malloc
# adds a fill and a device synchronisation to every allocation).
GROUP = dict(measured_s=4.22, limit_s=20, ids=[
    PATCHES + "test_the_hand_scene_on_three_build_paths_through_both_entry_points[atomic]",
    PATCHES + "test_a_checkerboard_of_two_tilts_is_every_node_under_6_and_two_patches_under_26",
    PATCHES + "test_two_storeys_stay_two_patches_and_the_stair_is_inclined",
    PATCHES + "test_a_box_cuts_a_patch_in_two",
    PATCHES + "test_a_call_after_a_larger_call_and_as_the_first_builder_of_the_column_index",
])


def test_every_node_id_is_collected_and_the_limit_is_three_times_the_measured_time():
    poison_tier.ids_collected(GROUP["ids"])
    poison_tier.limit_follows_rule(GROUP["measured_s"], GROUP["limit_s"])


@pytest.mark.gpu
@pytest.mark.parametrize("byte", poison_tier.BYTES, ids=poison_tier.BYTE_IDS)
def test_patches_under_poison(byte):
    poison_tier.run_group("surface patches", GROUP["ids"], GROUP["limit_s"], byte)
