"""CPU tier: the poisoned tier's runner (tests/poison_tier.py) without a child and without a GPU — what counts as an abnormal end, the
limit rule on the numbers of every group that uses the tier, and the one latch: set, it keeps run_group from starting anything; an
abnormal end sets it and names the group."""
import subprocess

import pytest

from tests import poison_tier

if poison_tier.UNDER_VARIANT:
    pytest.skip(poison_tier.REFUSAL, allow_module_level=True)          # (the modules below refuse to be imported there)

from tests import test_gpu_blocked_columns, test_gpu_footprint, test_gpu_obstacle_poisoned, test_gpu_poisoned      # noqa: E402
from tests import test_gpu_route_field_poisoned, test_gpu_segment_poisoned, test_gpu_shortcut, test_gpu_view_poisoned      # noqa: E402


def test_abnormal_ends():
    assert poison_tier.abnormal(None, "") == "killed at its time limit"
    assert poison_tier.abnormal(-11, "") == "ended by signal 11"
    assert poison_tier.abnormal(134, "") == "ended with status 134"
    assert poison_tier.abnormal(139, "") == "ended with status 139"
    assert poison_tier.abnormal(0, "HIP error: an illegal memory access was encountered") == "reported an illegal memory access"
    assert poison_tier.abnormal(0, "7 passed") is None
    assert poison_tier.abnormal(1, "1 failed, 6 passed") is None


def test_the_limit_rule_on_the_numbers_of_every_group():
    for measured_s, limit_s in ((0.01, 10), (3.33, 10), (3.34, 20), (10.0, 30), (10.01, 40)):
        poison_tier.limit_follows_rule(measured_s, limit_s)
    for measured_s, limit_s in ((0, 10), (-1.0, 10), (4.0, 10), (4.0, 30), (3.0, 9)):
        with pytest.raises(AssertionError):
            poison_tier.limit_follows_rule(measured_s, limit_s)
    groups = list(test_gpu_poisoned.GROUPS.values()) + [mod.GROUP for mod in (
        test_gpu_obstacle_poisoned, test_gpu_route_field_poisoned, test_gpu_segment_poisoned, test_gpu_view_poisoned, test_gpu_footprint,
        test_gpu_shortcut, test_gpu_blocked_columns)]
    assert len(groups) == len(test_gpu_poisoned.GROUPS) + 7
    for grp in groups:
        poison_tier.limit_follows_rule(grp["measured_s"], grp["limit_s"])
        assert grp["ids"] and len(grp["ids"]) == len(set(grp["ids"]))


class _Ended:
    def __init__(self, returncode, stdout):
        self.returncode, self.stdout = returncode, stdout


@pytest.fixture
def latch(monkeypatch):
    """the latch as it was, whatever the test does to it; the variant counts as built; every subprocess.run is recorded"""
    from grid_ndt_amd import _lib
    before = list(poison_tier.stopped)
    del poison_tier.stopped[:]
    monkeypatch.setattr(_lib, "build_native", lambda **kw: _lib.lib_path("poison"))
    yield poison_tier.stopped
    poison_tier.stopped[:] = before


def test_a_set_latch_starts_nothing(latch, monkeypatch):
    calls = []
    monkeypatch.setattr(subprocess, "run", lambda *a, **kw: calls.append(a))
    latch.append("the child of build under 0xa5 ended by signal 11")
    with pytest.raises(pytest.fail.Exception, match="not started: the child of build under 0xa5 ended by signal 11"):
        poison_tier.run_group("the footprints", ["tests/test_gpu_footprint.py::test_row_caps_around_support"], 20, 0x7F)
    assert not calls and len(latch) == 1


@pytest.mark.parametrize("returncode, output, why", [(139, "", "ended with status 139"), (-6, "", "ended by signal 6"),
                                                       (1, "an illegal memory access was encountered", "reported an illegal memory access")],
                         ids=["status_139", "signal_6", "illegal_access"])
def test_an_abnormal_end_sets_the_latch_and_names_the_group(latch, monkeypatch, returncode, output, why):
    calls = []

    def run(cmd, **kw):
        calls.append((cmd, kw))
        return _Ended(returncode, output)
    monkeypatch.setattr(subprocess, "run", run)
    with pytest.raises(pytest.fail.Exception, match=why):
        poison_tier.run_group("the column table", ["tests/some.py::test"], 20, 0xA5)
    assert latch == [f"the child of the column table under 0xa5 {why}"]
    assert len(calls) == 1 and calls[0][0][1:4] == ["-m", "tests.poisoned_child", "0xa5"] and calls[0][1]["timeout"] == 20
    assert calls[0][1]["env"]["GNDT_LIB_VARIANT"] == "poison"
    with pytest.raises(pytest.fail.Exception, match="not started"):          # and the next group, in whichever file, starts nothing
        poison_tier.run_group("view gain", ["tests/other.py::test"], 20, 0x7F)
    assert len(calls) == 1


def test_a_child_killed_at_its_limit_sets_the_latch(latch, monkeypatch):
    def run(cmd, **kw):
        raise subprocess.TimeoutExpired(cmd, kw["timeout"], output=b"half a line")
    monkeypatch.setattr(subprocess, "run", run)
    with pytest.raises(pytest.fail.Exception, match="killed at its time limit"):
        poison_tier.run_group("segmentation", ["tests/some.py::test"], 20, 0x7F)
    assert latch == ["the child of segmentation under 0x7f killed at its time limit"]


def test_a_failing_child_fails_its_case_and_leaves_the_latch(latch, monkeypatch):
    monkeypatch.setattr(subprocess, "run", lambda cmd, **kw: _Ended(1, "1 failed\n"))
    with pytest.raises(AssertionError):
        poison_tier.run_group("the route field", ["tests/some.py::test"], 30, 0xA5)
    assert latch == []
