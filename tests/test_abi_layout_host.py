"""The binding's layouts against include/gndt.h, as the host C compiler lays them out.

A C program that includes the header prints sizeof and every field's offsetof for each ctypes.Structure of grid_ndt_amd/_lib.py (the C
typedef is gndt_ plus the snake-cased class name, but for NAMES) and for each record dtype of _lib.RECORDS; the output is compared with
ctypes.sizeof / the ctypes field offsets and with the dtypes' itemsize / field offsets.  Then record_views, which derives a device
tensor's columns from those dtypes, is held against the numpy fields on random bytes.  Host code only."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from grid_ndt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"CommSelftest": "gndt_comm_selftest_report"}     # the one class not named after its typedef


def _structs():
    return sorted((n, v) for n, v in vars(_lib).items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure)


def _c_name(cls_name):
    return NAMES.get(cls_name) or "gndt_" + re.sub(r"(?<!^)(?=[A-Z])", "_", cls_name).lower()


@pytest.fixture(scope="module")
def c_layouts(tmp_path_factory):
    """{label: [sizeof, offsetof of every field in order]} from the compiled program"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler")
    items = [("ctypes:" + n, _c_name(n), [f[0] for f in v._fields_]) for n, v in _structs()]
    items += [("dtype:" + c, c, list(dt.names)) for c, dt in _lib.RECORDS.items()]
    src = ["#include <stddef.h>", "#include <stdio.h>", '#include "gndt.h"', "int main(void) {"]
    for label, ctype, fields in items:
        src.append(f'    printf("{label} %zu", sizeof({ctype}));')
        src += [f'    printf(" %zu", offsetof({ctype}, {f}));' for f in fields]
        src.append('    printf("\\n");')
    src += ["    return 0;", "}"]
    d = tmp_path_factory.mktemp("abi")
    (d / "layout.c").write_text("\n".join(src) + "\n")
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(d / "layout.c"), "-o", str(d / "layout")], check=True)
    out = subprocess.run([str(d / "layout")], check=True, capture_output=True, text=True).stdout
    return {w[0]: [int(x) for x in w[1:]] for w in (line.split() for line in out.splitlines())}


def test_every_ctypes_structure_matches_the_header(c_layouts):
    structs = _structs()
    assert len(structs) >= 31
    for name, cls in structs:
        want = [C.sizeof(cls)] + [getattr(cls, f[0]).offset for f in cls._fields_]
        assert c_layouts["ctypes:" + name] == want, f"{name} against {_c_name(name)}: C says {c_layouts['ctypes:' + name]}, ctypes {want}"


def test_every_record_dtype_matches_the_header(c_layouts):
    assert set(_lib.RECORDS) == {"gndt_route_info", "gndt_walk_info", "gndt_shortcut_info", "gndt_footprint_info", "gndt_view_info",
                                 "gndt_pose_score", "gndt_pose_derivs", "gndt_frontier", "gndt_scan_cluster"}
    for cname, dt in _lib.RECORDS.items():
        want = [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
        assert c_layouts["dtype:" + cname] == want, f"{cname}: C says {c_layouts['dtype:' + cname]}, the dtype {want}"
        assert dt.itemsize % 4 == 0


def test_the_one_record_with_a_ctypes_mirror_agrees_with_its_dtype():
    dt, cls = _lib.RECORDS["gndt_pose_derivs"], _lib.PoseDerivs
    assert [f[0] for f in cls._fields_] == list(dt.names) and C.sizeof(cls) == dt.itemsize
    mirrored = {_c_name(n) for n, _ in _structs()} & set(_lib.RECORDS)
    assert mirrored == {"gndt_pose_derivs"}      # (a record is described once: by its dtype)


@pytest.mark.parametrize("cname, wide", [(c, False) for c in sorted(_lib.RECORDS)] + [("gndt_pose_score", True), ("gndt_pose_derivs", True)])
@pytest.mark.parametrize("K", (0, 1, 5))
def test_record_views_are_the_dtype_fields(cname, K, wide):
    """the device decode against the host's, on the same bytes: every field, every width, a swapped half or column shows (wide:
    a record of 8-byte fields handed over as the int64 tensor the binding makes for it)"""
    assert _lib.record_is_wide(_lib.RECORDS[cname]) == (cname in ("gndt_pose_score", "gndt_pose_derivs"))
    import torch
    dt = _lib.RECORDS[cname]
    rng = np.random.default_rng(len(cname) + K)
    raw = rng.integers(0, 256, (K, dt.itemsize), dtype=np.uint8)
    host = raw.view(dt).reshape(K)
    dev = _lib.record_views(torch.from_numpy(raw.view(np.int64 if wide else np.int32).copy()), dt)
    assert list(dev) == [n for n in dt.names if n != "reserved"]
    for name, t in dev.items():
        field = host[name]
        got = t.numpy()
        assert got.shape == field.shape, name
        assert got.dtype.itemsize == max(field.dtype.itemsize, 4) and (got.dtype.kind == "f") == (field.dtype.kind == "f"), name
        if field.dtype.itemsize == 2:
            assert (got == field.astype(np.int32)).all(), name
        else:
            assert (np.ascontiguousarray(got).view(np.uint8) == np.ascontiguousarray(field).view(np.uint8)).all(), name
