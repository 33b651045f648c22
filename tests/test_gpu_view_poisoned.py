"""The poisoned tier for view gain: a handful of tests/test_gpu_view.py in ONE fresh child process per fill byte
(tests/poisoned_child.py, GNDT_LIB_VARIANT = poison: every device and pinned host allocation filled with the byte before it is handed
out), for the two bytes of tests/test_gpu_poisoned.py.  What it is after: the host-pointer entry point's records, rows and ranges come
back from a staging area of the handle that nothing clears — a field of a record, or a ray's row or range, that the kernel leaves
unwritten is 0 in a fresh process and the byte here, and the restatement has neither.  (The kernel's own sets live in LDS, which no
allocation poisons: tests/test_gpu_view.py dirties it itself.)  The children run one at a time, each under the time limit below; a
child that is killed at its limit, ends by a signal, with status 134 or 139, or reports an illegal memory access stops the tier: the
case after it fails at once with "not started" and touches no GPU."""
import json
import subprocess
import sys

import pytest

from tests.test_gpu_poisoned import BYTES, ROOT, _abnormal, _env

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
    ids = GROUP["ids"]
    assert len(ids) == len(set(ids))
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + ids, cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=300)
    found = {line.strip() for line in r.stdout.splitlines() if "::" in line}
    assert r.returncode == 0 and found == set(ids), (sorted(set(ids) - found), r.stdout[-2000:], r.stderr[-2000:])
    assert GROUP["measured_s"] > 0 and GROUP["limit_s"] == -(-3 * GROUP["measured_s"] // 10) * 10


_stopped = []        # why the tier stopped: a child ended abnormally


@pytest.mark.gpu
@pytest.mark.parametrize("byte", BYTES, ids=["0xA5", "0x7F"])
def test_view_gain_under_poison(byte):
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
