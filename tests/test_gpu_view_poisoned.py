"""The poisoned tier for view gain: a handful of tests/test_gpu_view.py in ONE fresh child process per fill byte
(tests/poisoned_child.py, GNDT_LIB_VARIANT = poison: every device and pinned host allocation filled with the byte before it is handed
out), for the two bytes of tests/test_gpu_poisoned.py.  What it is after: the host-pointer entry point's records, rows and ranges come
back from a staging area of the handle that nothing clears — a field of a record, or a ray's row or range, that the kernel leaves
unwritten is 0 in a fresh process and the byte here, and the restatement has neither.  (The kernel's own sets live in LDS, which no
allocation poisons: tests/test_gpu_view.py dirties it itself.)  The children run one at a time, each under the time limit below; a
child that is killed at its limit, ends by a signal, with status 134 or 139, or reports an illegal memory access stops the tier: the
case after it fails at once with "not started" and touches no GPU."""
import pytest

from tests import poison_tier

poison_tier.refuse_under_variant()

VIEW = "tests/test_gpu_view.py::"
# the hand case and the windows at the LDS edges through both entry points, the host path's records on a built map, every combination
# of null per-ray outputs, and the poses that skip every ray.  measured_s: the whole child (interpreter start to exit) on the MI355X
# under the regular library; limit_s: three times that, rounded up to 10 s (poison_malloc adds a fill and a device synchronisation
# to every allocation).
GROUP = dict(measured_s=5.32, limit_s=20, ids=[
    VIEW + "test_the_hand_case_through_both_entry_points[False]",
    VIEW + "test_the_hand_case_through_both_entry_points[True]",
    VIEW + "test_window_edges[0.8-2]",
    VIEW + "test_window_edges[253.0-254]",
    VIEW + "test_window_edges[402.0-403]",
    VIEW + "test_the_cast_parameters_equal_the_restatement",
    VIEW + "test_per_ray_outputs_are_the_casts_bit_for_bit",
    VIEW + "test_capture_is_refused_and_the_empty_batches",
])


def test_every_node_id_is_collected_and_the_limit_is_three_times_the_measured_time():
    poison_tier.ids_collected(GROUP["ids"])
    poison_tier.limit_follows_rule(GROUP["measured_s"], GROUP["limit_s"])


@pytest.mark.gpu
@pytest.mark.parametrize("byte", poison_tier.BYTES, ids=poison_tier.BYTE_IDS)
def test_view_gain_under_poison(byte):
    poison_tier.run_group("view gain", GROUP["ids"], GROUP["limit_s"], byte)
