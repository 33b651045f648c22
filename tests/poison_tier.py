"""The poisoned tier's one runner and one latch (tests/test_gpu_poisoned.py describes the variant, the bytes and the groups).

A group is dict(measured_s, limit_s, ids): existing GPU tests that run in ONE fresh child process per fill byte (tests/poisoned_child.py,
GNDT_LIB_VARIANT = poison).  measured_s is the whole child (interpreter start to exit) on the MI355X under the regular library, limit_s
three times that rounded up to 10 s (poison_malloc adds a fill and a device synchronisation to every allocation).  The children run one
at a time, each under its group's limit.  A child that is killed at its limit, ends by a signal, with status 134 or 139, or reports an
illegal memory access stops the tier for the rest of the session, in every file that uses it: each later case fails at once with "not
started" and touches no GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES = (0xA5, 0x7F)
BYTE_IDS = ["0xA5", "0x7F"]
UNDER_VARIANT = bool(os.environ.get("GNDT_LIB_VARIANT"))
REFUSAL = "this process runs on a variant of the library itself (a child of the tier): no children of its own"
# for a tier test in a file whose other tests the children themselves run
refused_under_variant = pytest.mark.skipif(UNDER_VARIANT, reason=REFUSAL)

stopped = []        # the one latch — why the tier stopped: a child ended abnormally


def refuse_under_variant():
    """for a module that holds nothing but a tier: skipped as a whole in a process that runs on a variant"""
    if UNDER_VARIANT:
        pytest.skip(REFUSAL, allow_module_level=True)


def env(variant=None):
    env = dict(os.environ)
    env.pop("GNDT_LIB_VARIANT", None)
    if variant:
        env["GNDT_LIB_VARIANT"] = variant
    return env


def abnormal(returncode, output):
    if returncode is None:
        return "killed at its time limit"
    if returncode < 0:
        return f"ended by signal {-returncode}"
    if returncode in (134, 139):
        return f"ended with status {returncode}"
    if "illegal memory access" in output:
        return "reported an illegal memory access"
    return None


def ids_collected(ids):
    """every node id exists, once, and the ids name nothing else"""
    assert len(ids) == len(set(ids))
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + list(ids), cwd=ROOT, env=env(),
                       capture_output=True, text=True, timeout=300)
    found = {line.strip() for line in r.stdout.splitlines() if "::" in line}
    missing = [i for i in ids if i not in found]
    assert r.returncode == 0 and not missing, (missing, r.stdout[-2000:], r.stderr[-2000:])
    assert len(found) == len(ids), sorted(found - set(ids))


def limit_follows_rule(measured_s, limit_s):
    assert measured_s > 0 and limit_s == -(-3 * measured_s // 10) * 10, (measured_s, limit_s)


def run_group(label, ids, limit_s, byte):
    """one child on the poisoned variant under the fill byte; an abnormal end latches"""
    from grid_ndt_amd import _lib
    if stopped:
        pytest.fail(f"not started: {stopped[0]}", pytrace=False)
    _lib.build_native(variant="poison")          # (the build has made it: nothing compiles inside the child's limit)
    cmd = [sys.executable, "-m", "tests.poisoned_child", hex(byte)] + list(ids)
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=env("poison"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit_s)
        returncode, output = r.returncode, r.stdout
    except subprocess.TimeoutExpired as e:
        out = e.stdout or ""
        returncode, output = None, out.decode(errors="replace") if isinstance(out, bytes) else out
    print(output[-6000:])
    why = abnormal(returncode, output)
    if why:
        stopped.append(f"the child of {label} under {byte:#x} {why}")
        pytest.fail(stopped[0] + "\n" + output[-3000:], pytrace=False)
    lines = [line for line in output.splitlines() if line.startswith('{"poisoned_child"')]
    assert returncode == 0 and len(lines) == 1, (returncode, output[-3000:])
    rep = json.loads(lines[0])
    assert rep["exit"] == 0 and rep["byte"] == byte
    assert rep["device_bytes"] > 0 and rep["host_bytes"] > 0, rep
    assert rep["lib"] == _lib.lib_path("poison")
