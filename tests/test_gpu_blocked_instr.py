"""k_bucket_blocked with its wave scans by DPP (full_wave_scan_add, gndt_blocked.hpp): the scan helper on the device against numpy, and
blocked builds of clouds aimed at the kernel's key -> slot -> rank -> walk steps — points within 2 ulp of cell and block borders,
weighted records (64 and 512 identical points in one record), a record outside its block, a record beyond the key range.  Whatever
the instructions, the map is the oracle's by parity.compare's strict gates.  The clouds' CPU-tier twins (no GPU mark) hold the
fixtures: the oracle alone passes the gates on them and the layout rule still gives the scene's block."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import blocked_scenes as bs
from tests import parity
from tests.gpu_kit import dev, handle

SCENE = "levels_4_at_interval"
BLOCKED = 7             # GNDT_STRATEGY_PARTITION_BLOCKED
ERR_KEY_RANGE = 4
EDGE_POINTS = 4096
_HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the clouds ----
def _ulp_steps(v, steps):
    """v moved by steps[i] float32 ulps (-2 .. 2)"""
    v = v.astype(np.float32).copy()
    for k in (1, 2):
        v = np.where(steps >= k, np.nextafter(v, np.float32(np.inf)), v)
        v = np.where(steps <= -k, np.nextafter(v, np.float32(-np.inf)), v)
    return v


@functools.lru_cache(maxsize=None)
def _cloud(kind):
    """The scene's cloud with, `borders`: its last 4 096 points within +-2 ulp of cell borders (all three axes, both sides of the
    origin and the origin's own border) and of the block borders inside the box (x every 16 cells, y every 8; the box is one block
    high); `weighted`: identical points where level 1 of the partition (k_part2_level1: tiles of 4 096 points, wave w of a tile holds points
    512 j + 64 w + lane, j = 0 .. 7) folds them — a run of 512 from a multiple of 4 096 (strip j = 0 of all eight waves: eight records
    of weight 64), a run of 64 from a multiple of 64 (one record of weight 64) and all eight strips of one wave (one record of
    weight 512) —, in three blocks.  _folded_records restates the rule."""
    s = bs.SCENES[SCENE]
    c = bs.cloud(SCENE).copy()
    if kind == "borders":
        rng = np.random.default_rng(0xB0DE)
        n = EDGE_POINTS
        lo, hi = np.float64(s["lo"]), np.float64(s["hi"])
        pts = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
        lens = (s["grid_len"], s["grid_len"], s["z_len"])
        axis = np.arange(n) % 3
        steps = rng.integers(-2, 3, n)
        for a in range(3):
            sel = np.flatnonzero(axis == a)
            kmax = int(round(hi[a] / lens[a])) - 1                   # cell borders strictly inside the box: |k| <= kmax
            k = rng.integers(-kmax, kmax + 1, sel.size)
            if a < 2:                                                # every other one on a block border: the box starts on one
                ext = s["block"][a]
                first = int(round(lo[a] / lens[a]))
                m = rng.integers(1, (2 * -first) // ext, sel.size)
                k[::2] = first + ext * m[::2]
            k[:3] = (-1, 0, 1)
            pts[sel, a] = _ulp_steps((k * np.float64(lens[a])).astype(np.float32), steps[sel])
        assert (pts >= np.float32(lo)).all() and (pts <= np.float32(hi)).all()
        c[-n:] = pts
    elif kind == "weighted":
        c[1 + 4096 * 100:1 + 4096 * 100 + 512] = np.float32([3.3, -7.1, 0.05])        # (body index = cloud index - 1)
        c[1 + 64 * 9001:1 + 64 * 9001 + 64] = np.float32([-21.3, 30.2, -0.1])
        strips = 1 + 4096 * 200 + 64 * 3 + (512 * np.arange(8)[:, None] + np.arange(64)[None, :]).reshape(-1)      # wave 3 of tile 200
        c[strips] = np.float32([30.7, 12.4, 0.1])
    else:
        raise KeyError(kind)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _ref(kind, demand):
    return parity.ref_from_cloud(_cloud(kind), bs.params(SCENE, demand), mode=2)


def _folded_records(cloud):
    """(records of weight 64, records of weight 512) that level 1 of the two-level partition makes of the cloud's body
    (gndt_partition.hpp, k_part2_level1): in every whole tile of 4 096 points a wave whose 512 points are bit-identical sends one
    record of weight 512, otherwise each of its strips of 64 bit-identical points one of weight 64."""
    body = np.ascontiguousarray(cloud[1:]).view(np.uint32)
    tiles = body.shape[0] // 4096
    t = body[:tiles * 4096].reshape(tiles, 8, 8, 64, 3)                    # tile, strip j, wave, lane
    strip_same = (t == t[:, :, :, :1]).all((3, 4))                          # (tile, j, wave)
    wave_same = strip_same.all(1) & (t[:, :, :, 0] == t[:, :1, :, 0]).all((1, 3))
    w512 = int(wave_same.sum())
    w64 = int(strip_same.sum()) - 8 * w512
    tail = body[tiles * 4096:]                                              # (the last, partial tile: strips only)
    for s in range(0, tail.shape[0] - 63, 64):
        w64 += int((tail[s:s + 64] == tail[s]).all())
    return w64, w512


# ---- CPU tier: the fixtures ----
@pytest.mark.parametrize("kind", ["borders", "weighted"])
def test_fixture_cloud_keeps_the_scenes_block_and_the_oracle_alone_passes(kind):
    want = bs.SCENES[SCENE]
    for demand in ("slope", "true"):
        ref = _ref(kind, demand)
        lay = bs.plan(ref, bs.POINTS)
        assert lay["state"] == 1 and (1 << lay["shx"], 1 << lay["shy"], 1 << lay["shz"]) == want["block"], lay
        assert (lay["nx"], lay["ny"]) == want["blocks"], lay
        rep = parity.compare(bs.perfect_build(ref), ref, demand)
        assert rep["ok"], (demand, rep["fail"])
    if kind == "borders":
        tail = _cloud(kind)[-EDGE_POINTS:]
        lens = np.float32([want["grid_len"], want["grid_len"], want["z_len"]])
        near = np.abs(tail / lens - np.round(tail / lens)) < 1e-4
        assert near.any(1).all() and (tail[near.any(1)] > 0).any() and (tail < 0).any()
    else:
        ref = _ref(kind, "slope")
        big = np.sort(ref["count"])[-3:]
        assert big[0] >= 64 and big[1] >= 512 and int(big[2]) * 4 < bs.POINTS // 242, big      # far below a quarter of a block's points
        # what reaches the bucket kernel: nine records of weight 64, one of weight 512 (and none in the other clouds)
        assert _folded_records(_cloud(kind)) == (9, 1) and _folded_records(bs.cloud(SCENE)) == (0, 0)


# ---- GPU tier ----
def _blocked_builds(kind, demand):
    """Three builds on a fresh handle: the layout after the first is the rule's on the oracle's map, builds 2 and 3 are blocked, not
    re-run, and the oracle's map.  -> the handle."""
    P = bs.params(SCENE, demand)
    cloud, ref = _cloud(kind), _ref(kind, demand)
    m = handle(P, min_points=P["min_points"])
    m.setCloudFirst(cloud[0])
    t = dev(cloud[1:], copy=True)
    for k in range(3):
        m.create2DMap(demand, t)
        if k == 0:
            m.sync()
            assert m.block_layout() == bs.plan(ref, bs.POINTS), (m.block_layout(), bs.plan(ref, bs.POINTS))
            continue
        out = m.export()
        assert m.last_strategy() == BLOCKED and m.retry_count() == 0, (k, m.STRATEGY_NAMES[m.last_strategy()], m.retry_count())
        rep = parity.compare(out, ref, demand, min_points=P["min_points"])
        assert rep["ok"], (kind, demand, k, rep["fail"])
    assert m.block_layout() == bs.plan(ref, bs.POINTS)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("demand", ["slope", "true"])
def test_points_on_cell_and_block_borders(demand):
    _blocked_builds("borders", demand)


@pytest.mark.gpu
@pytest.mark.parametrize("demand", ["slope", "true"])
def test_weighted_records_reach_the_walk(demand):
    """Level 1 of the partition folds a strip of 64 identical points into one record of weight 64 and a wave's eight identical strips
    into one of weight 512 (the index word's flags): 1 088 points of the cloud reach the blocked build as ten records (the CPU-tier
    twin counts them by the kernel's rule; the library exposes no count of its own), and its walk adds them with their weights —
    a walk that took them as single points would leave the three nodes 63, 504 and 511 points short, which the parity gate on the
    counts catches."""
    m = _blocked_builds("weighted", demand)
    out = m.export()
    assert np.sort(out["count"])[-3:].tolist() == np.sort(_ref("weighted", demand)["count"])[-3:].tolist()


@pytest.mark.gpu
def test_record_outside_its_block_and_record_beyond_the_key_range():
    import grid_ndt_amd as g
    P = bs.params(SCENE)
    m = _blocked_builds("borders", "slope")
    cloud = _cloud("borders")
    t = dev(cloud[1:], copy=True)
    # |nz| = 2.5 M > 2^21 - 1: found by the bucket kernel; the handle keeps its box
    bad = cloud.copy()
    bad[-1, 2] = np.float32(2.0e5)
    with pytest.raises(g.GndtError) as e:
        m.create2DMap("slope", dev(bad[1:], copy=True))
        m.sync()
    assert e.value.code == ERR_KEY_RANGE, str(e.value)
    m.create2DMap("slope", t)
    out = m.export()
    assert m.last_strategy() == BLOCKED, m.STRATEGY_NAMES[m.last_strategy()]
    rep = parity.compare(out, _ref("borders", "slope"), "slope")
    assert rep["ok"], rep["fail"]
    # one level above the box (the box is one block high): not its block's -> the build is run again with hashed buckets
    out_of_box = cloud.copy()
    out_of_box[-1] = np.float32([1.1, 1.1, 0.2])
    before = m.retry_count()
    m.create2DMap("slope", dev(out_of_box[1:], copy=True))
    out = m.export()
    assert m.last_strategy() != BLOCKED and m.retry_count() > before, (m.STRATEGY_NAMES[m.last_strategy()], m.retry_count())
    rep = parity.compare(out, parity.ref_from_cloud(out_of_box, P, mode=2), "slope")
    assert rep["ok"], rep["fail"]


# ---- the scan helper ----
_SCAN_SO = os.path.join(_HERE, "_wave_scan_shim.so")


def _scan_shim():
    """tests/wave_scan_shim.hip built like the device maths shim (tests/host_emulation.build_device_shim): libgndt's flags, linked
    against the HIP runtime the process shares with torch"""
    from grid_ndt_amd import _lib
    _lib.lib()
    src = os.path.join(_HERE, "wave_scan_shim.hip")
    dep = [src] + [os.path.join(_lib._CSRC, h) for h in _lib.HEADERS if not os.path.isabs(h)]
    if not os.path.exists(_SCAN_SO) or os.path.getmtime(_SCAN_SO) < max(os.path.getmtime(d) for d in dep):
        obj = os.path.splitext(_SCAN_SO)[0] + ".o"
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + _lib.HIPCC_FLAGS
                              + ["-I", os.path.join(os.path.dirname(_HERE), "include"), "-I", _lib._CSRC, "-o", obj, src])
        libdir = _lib._hip_runtime_dir()
        tmp = _SCAN_SO + ".tmp.so"
        subprocess.check_call(["g++", "-shared", "-o", tmp, obj, "-L", libdir, "-l:libamdhip64.so", "-Wl,-rpath," + libdir,
                               "-Wl,--no-undefined", "-lpthread", "-ldl"])
        os.replace(tmp, _SCAN_SO)
    L = C.CDLL(_SCAN_SO)
    L.wshim_scan.restype = C.c_int
    L.wshim_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    return L


def test_scan_shim_cross_compiles():
    """CPU tier: the shim builds for gfx950 with the library's flags (keeps the GPU tier's case from rotting)."""
    assert os.path.exists(_scan_shim()._name)


@pytest.mark.gpu
def test_full_wave_scan_add_against_numpy():
    import torch
    L = _scan_shim()
    rng = np.random.default_rng(3)
    waves = [rng.integers(0, 4096, (8, 64)), np.zeros((1, 64), np.int64), np.full((1, 64), 0xFFFF, np.int64)]
    for lane in (0, 15, 16, 31, 32, 63):
        w = np.zeros((1, 64), np.int64)
        w[0, lane] = 7 + lane
        waves.append(w)
    x = np.concatenate(waves).astype(np.uint32)
    d_in = torch.from_numpy(x.view(np.int32).reshape(-1)).cuda()
    d_out = torch.full_like(d_in, -1)
    d_tot = torch.full((x.shape[0],), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream()
    assert L.wshim_scan(d_in.data_ptr(), d_out.data_ptr(), d_tot.data_ptr(), x.shape[0], stream.cuda_stream) == 0
    stream.synchronize()
    want = np.cumsum(x.astype(np.int64), 1)
    np.testing.assert_array_equal(d_out.cpu().numpy().view(np.uint32).reshape(x.shape), want.astype(np.uint32))
    np.testing.assert_array_equal(d_tot.cpu().numpy().view(np.uint32), want[:, -1].astype(np.uint32))
