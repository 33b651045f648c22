"""The poisoned tier for the route field: twelve of tests/test_gpu_route_field.py in ONE fresh child process per fill byte
(tests/poisoned_child.py, GNDT_LIB_VARIANT = poison: every device and pinned host allocation filled with the byte before it is handed
out), for the two bytes of tests/test_gpu_poisoned.py.  What it is after: the first steps, the rest of the steps, the keys, the weights,
the "more" bits and the sweeps' flag words are cut out of one scratch area on every call; every one of them is written by a pass of the
call before a later pass reads it (the flag words by a memset) — a word that a pass reads before anything wrote it is 0 in a fresh
process and the byte here: 0xA5A5A5A5 as a flag word is "the sweep before changed something" for ever, as a key a cost no walk has,
as a weight a slope that costs -2.9e-16 to enter.  The host entry points' staging and the descent's records are in the group too.
The children run one at a time, each under the time limit below; a child that is killed at its limit, ends by a signal, with status 134
or 139, or reports an illegal memory access stops the tier: the case after it fails at once with "not started" and touches no GPU."""
import json
import subprocess
import sys

import pytest

from tests.test_gpu_poisoned import BYTES, ROOT, _abnormal, _env

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
    ids = GROUP["ids"]
    assert len(ids) == len(set(ids)) == 12
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + ids, cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=300)
    found = {line.strip() for line in r.stdout.splitlines() if "::" in line}
    assert r.returncode == 0 and found == set(ids), (sorted(set(ids) - found), r.stdout[-2000:], r.stderr[-2000:])
    assert GROUP["measured_s"] > 0 and GROUP["limit_s"] == -(-3 * GROUP["measured_s"] // 10) * 10


_stopped = []        # why the tier stopped: a child ended abnormally


@pytest.mark.gpu
@pytest.mark.parametrize("byte", BYTES, ids=["0xA5", "0x7F"])
def test_route_field_under_poison(byte):
    from grid_ndt_amd import _lib
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}", pytrace=False)
    _lib.build_native(variant="poison")          # (__graft_entry__.build() has built it: nothing compiles inside the child's limit)
    cmd = [sys.executable, "-m", "tests.poisoned_child", hex(byte)] + GROUP["ids"]
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=_env("poison"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=GROUP["limit_s"])
        returncode, output = r.returncode, r.stdout
    except subprocess.TimeoutExpired as e:
        out = e.stdout or ""
        returncode, output = None, out.decode(errors="replace") if isinstance(out, bytes) else out
    print(output[-6000:])
    why = _abnormal(returncode, output)
    if why:
        _stopped.append(f"the child under {byte:#x} {why}")
        pytest.fail(_stopped[0] + "\n" + output[-3000:], pytrace=False)
    lines = [line for line in output.splitlines() if line.startswith('{"poisoned_child"')]
    assert returncode == 0 and len(lines) == 1, (returncode, output[-3000:])
    rep = json.loads(lines[0])
    assert rep["exit"] == 0 and rep["byte"] == byte
    assert rep["device_bytes"] > 0 and rep["host_bytes"] > 0, rep
    assert rep["lib"] == _lib.lib_path("poison")
