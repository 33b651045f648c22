"""The child of tests/test_gpu_poisoned.py: `python -m tests.poisoned_child <byte> <node id> ...` with GNDT_LIB_VARIANT=poison in its
environment runs the given tests in this process on the poisoned variant of the library (grid_ndt_amd/_lib.py VARIANTS: every
device and pinned host allocation filled with <byte> before it is handed out) and prints one JSON line: pytest's exit code, the bytes
poisoned on the device and on the host, and the path of the library that was loaded.  Exits with pytest's code."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv):
    import pytest
    import grid_ndt_amd as g
    from grid_ndt_amd import _lib
    byte, ids = int(argv[0], 0), argv[1:]
    _lib.lib()
    assert _lib.VARIANT == "poison" and _lib.LIB_PATH == _lib.lib_path("poison") and _lib.lib()._name == _lib.LIB_PATH, _lib.LIB_PATH
    g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_POISON_BYTE, byte)
    code = int(pytest.main(["-x", "-q", "-p", "no:cacheprovider", "--rootdir", ROOT] + [os.path.join(ROOT, i) for i in ids]))
    device_bytes, host_bytes = g.TwoDmap.poisoned_bytes()
    sys.stdout.flush()
    print(json.dumps({"poisoned_child": True, "exit": code, "byte": byte, "device_bytes": device_bytes, "host_bytes": host_bytes,
                      "lib": _lib.LIB_PATH}), flush=True)
    return code


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
