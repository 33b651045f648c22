"""CPU tier: the two guards of the host shims' plumbing (tests/host_emulation.py).  The ShimMap a map crosses the C boundary in is
declared twice — tests/shim_map.hpp and its ctypes mirror — and load_shim refuses a shim whose layout is not the mirror's; a shim is
compiled again when any header it may include, directly or not, is newer than its binary."""
import ctypes as C
import os

import pytest

from tests import host_emulation as he


def test_a_mirror_that_drifts_from_the_header_fails_at_load():
    L = he.consumer_shim()                      # (loaded: the real mirror has passed)
    assert hasattr(L, "shim_map_layout")
    he.check_shim_map(L)
    fields = list(he.ShimMap._fields_)
    at = {name: i for i, (name, _) in enumerate(fields)}

    def mirror(changed):
        return type("Drifted", (C.Structure,), {"_fields_": changed})

    # two pointers swapped: every offset and the size stay, the names do not
    swapped = list(fields)
    swapped[at["mean"]], swapped[at["normal"]] = swapped[at["normal"]], swapped[at["mean"]]
    # a field of another width: the names stay, and so does every offset (padding takes up the difference); its size does not
    wider = list(fields)
    wider[at["n"]] = ("n", C.c_uint32)
    # a field left out
    shorter = [f for f in fields if f[0] != "cov"]
    for changed in (swapped, wider, shorter):
        with pytest.raises(AssertionError, match="ShimMap"):
            he.check_shim_map(L, mirror(changed))


def test_a_header_included_only_through_another_rebuilds_the_shim(tmp_path, monkeypatch):
    """a source tree of two headers, the shim naming only the outer one: the rule lists no includes, it takes every *.hpp of the tree"""
    csrc = tmp_path / "csrc"
    csrc.mkdir()
    (csrc / "gndt_cost.hpp").write_text("#pragma once\nconstexpr int kInner = 41;\n")
    (csrc / "gndt_clearance.hpp").write_text('#pragma once\n#include "gndt_cost.hpp"\nconstexpr int kOuter = kInner + 1;\n')
    src = tmp_path / "tiny_shim.cpp"
    src.write_text('#include "gndt_clearance.hpp"\nextern "C" int tiny() { return kOuter; }\n')
    so = str(tmp_path / "_tiny_shim.so")
    monkeypatch.setattr(he, "_CSRC", str(csrc))
    load = lambda: he.load_shim(str(src), so, {"tiny": ([], C.c_int)})
    assert load().tiny() == 42
    built = os.stat(so).st_mtime_ns
    load()
    assert os.stat(so).st_mtime_ns == built                     # nothing newer: the binary stays
    os.utime(so, ns=(built - 10 ** 10, built - 10 ** 10))       # the binary ten seconds older than it is, then the inner header touched
    old = os.stat(so).st_mtime_ns
    for f in (src, csrc / "gndt_clearance.hpp"):
        os.utime(f, ns=(old - 10 ** 9, old - 10 ** 9))
    os.utime(csrc / "gndt_cost.hpp", ns=(old + 10 ** 9, old + 10 ** 9))
    load()
    assert os.stat(so).st_mtime_ns > old + 10 ** 9              # compiled again
