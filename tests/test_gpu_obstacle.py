"""GPU tier: the obstacle field (gndt_obstacle_field_device / gndt_obstacle_field, TwoDmap.obstacle_field / index_boxes).  Every map is
built on the device; hops, obstacle and counts are compared for equality with the restatement (tests/obstacle_ref.py) on the handle's own
export, through both entry points.  Hand cases on a 16 x 16 floor across the origin, the device-side box count, both strides (72 on real
gndt_scan_cluster records), the budget, lattices with exact row and column counts at the kernels' edges, the base merge, every
combination of NULL outputs, every refused argument, repeat calls on two streams, a small call after a large one, the call after an
update, a crop and a clear, and the chain segment_scan -> obstacle_field -> walk_paths / shortcut_routes on one stream.  No tolerance
anywhere: the one step that is not IEEE arithmetic is the gates' acosf, and every map keeps its angle decisions more than 1e-3 degrees
from the threshold.  Every test asserts that it is not vacuous: covered > 0, some finite hops > 0, some BEYOND."""
import ctypes as C

import numpy as np
import pytest

from tests import clearance_ref as cr
from tests import frontier_ref as fr
from tests import obstacle_ref as ob
from tests.gpu_kit import Padded, PaddedCall, at, build, dev, robot_arg
from tests.gpu_kit import tails_untouched as untouched

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
ATOMIC = 1
SENTINEL = 0x5A5A5A5A
PAD = 5                      # sentinel entries behind num_nodes
_scenes = {}


def _tgc():
    import tests.test_gpu_clearance as tgc
    return tgc


def raw(m, boxes, inflate=0, max_hops=8, levels_above=0, levels_below=0, max_columns=0, base=None, in_place=False, n_boxes_dev=None,
        stride=24, robot=None, outs=("hops", "obstacle"), stream=None, host=False, reserved=(0, 0), counts=True, n_boxes=None, params=True,
        misalign=0):
    """The C entry points, every output num_nodes + PAD entries of sentinel.  -> (rc, dict(hops, obstacle: the outputs asked for, cut to
    num_nodes; counts; tails: what lies behind num_nodes))"""
    from grid_ndt_amd._lib import ObstacleParams
    n = int(m.sync()[0])
    prm = ObstacleParams(inflate, max_hops, levels_above, levels_below, max_columns, (C.c_uint32 * 2)(*reserved))
    boxes = None if boxes is None else np.ascontiguousarray(boxes, np.int32).reshape(-1, 6)
    nb = (0 if boxes is None else len(boxes)) if n_boxes is None else n_boxes
    recs = np.full((max(nb, 1), stride // 4 if stride >= 24 and stride % 4 == 0 else 6), SENTINEL, np.int32)
    off = (recs.shape[1] - 6) // 2                        # the six words somewhere inside a wider record
    if boxes is not None:
        recs[:len(boxes), off:off + 6] = boxes
    buf = {k: Padded(n, back=PAD, fill=SENTINEL) for k in outs}
    bs = None
    if base is not None:
        base = np.ascontiguousarray(base).view(np.uint32)
        bs = Padded(len(base), back=PAD, fill=SENTINEL)
        bs.body[:] = base
        if in_place:
            buf["hops"].a[:] = bs.a
    cnt = Padded(8, fill=SENTINEL)
    # (the host entry point has no count on the device)
    nbd = [] if host else [None if n_boxes_dev is None else np.array([n_boxes_dev], np.uint32)]
    rc = PaddedCall(host, stream, wait_for_current=True)(
        m._L.gndt_obstacle_field, m._L.gndt_obstacle_field_device, m._h, robot_arg(robot, cr.ROBOT),
        None if boxes is None else at(recs, 4 * off + misalign), nb, stride, *nbd, C.byref(prm) if params else None,
        buf["hops"] if in_place else bs, buf.get("hops"), buf.get("obstacle"), cnt if counts else None)
    if bs is not None:
        assert bs.body.tobytes() == base.tobytes() and bs.untouched()          # the base is read, never written
    out = {k: p.body for k, p in buf.items()}
    out.update(counts=cnt.a, tails={k: p.tail for k, p in buf.items()})
    return rc, out


REF_KEYS = ("inflate", "max_hops", "levels_above", "levels_below", "max_columns", "base", "n_boxes_dev")


def check(m, f, cells, boxes, what="", entries=(False, True), vacuous_ok=False, **kw):
    """both entry points against the restatement -> (the device call's answer, the restatement)"""
    want = ob.field(f, cells, boxes, **{k: v for k, v in kw.items() if k in REF_KEYS})
    first = None
    for host in entries:
        if host and "n_boxes_dev" in kw:
            continue                                       # (the host entry point has no count on the device)
        rc, got = raw(m, boxes, host=host, **kw)
        assert rc == 0, (what, host, m._L.gndt_last_error(m._h))
        assert np.array_equal(got["counts"], want["counts"]), (what, host, got["counts"], want["counts"])
        for k in kw.get("outs", ("hops", "obstacle")):
            assert np.array_equal(got[k], want[k]), (what, host, k, np.flatnonzero(got[k] != want[k])[:8], got[k][:8], want[k][:8])
        assert untouched(got), (what, host)
        first = first or got
    if not vacuous_ok:
        h = want["own_hops"]
        assert want["counts"][0] > 0 and ((h > 0) & (h != ob.BEYOND)).any() and (h == ob.BEYOND).any(), (what, want["counts"])
    return first, want


def floor():
    """a 16 x 16 floor across the origin on both axes: columns -8 .. -1, 1 .. 8, all slopes on level 1 -> (m, restatement, export)"""
    return _tgc().drawn("obstacle floor", lambda: fr.cells_cloud([(ix, iy) for ix in range(-8, 8) for iy in range(-8, 8)]))


def corridor():
    return _tgc().drawn("corridor", cr.corridor_cloud, cr.CORRIDOR_P)


# ---- hand cases on the 16 x 16 floor --------------------------------------------------------------------------------------------------

def test_one_box_two_overlapping_boxes_and_the_inflation():
    m, f, cells = floor()
    assert cells["num_nodes"] == 256 and ((cells["flags"] & 2) != 0).all() and set(cells["sz"].tolist()) == {1}
    got, want = check(m, f, cells, [[3, 4, 5, 5, 1, 1]], "one box", max_hops=3)
    assert tuple(got["counts"]) == (2, 2 + 6 + 10 + 14, 3, 1, 1, 8 * 7, 0, 0)
    assert (got["hops"][(cells["sx"] == 3) & (cells["sy"] == 5)] == 0).all() and (got["hops"][(cells["sx"] == 1) & (cells["sy"] == 5)] == 2).all()
    # the overlap belongs to the smaller index, and so does every slope the same steps from both
    two = [[2, 4, 2, 4, 1, 1], [4, 6, 4, 6, 1, 1]]
    got, want = check(m, f, cells, two, "two boxes", max_hops=2)
    at = lambda x, y: int(got["obstacle"][(cells["sx"] == x) & (cells["sy"] == y)][0])
    assert at(4, 4) == 0 and at(3, 3) == 0 and at(6, 6) == 1 and at(5, 4) == 1 and at(4, 6) == 1 and got["counts"][4] == 2
    got2, _ = check(m, f, cells, two[::-1], "two boxes, swapped", max_hops=2)
    assert int(got2["obstacle"][(cells["sx"] == 4) & (cells["sy"] == 4)][0]) == 0 and np.array_equal(got2["hops"], got["hops"])
    for inflate, covered, reach in ((0, 1, 25), (1, 9, 49), (3, 49, 110)):             # (the last window is cut by the floor's edge)
        got, _ = check(m, f, cells, [[-4, -4, 3, 3, 1, 1]], ("inflate", inflate), inflate=inflate, max_hops=2)
        assert got["counts"][0] == covered and got["counts"][5] == reach


def test_boxes_astride_the_seams_off_the_map_void_and_none():
    m, f, cells = floor()
    # across index 0 on x, on y and on z: -1 and 1 are neighbours
    got, _ = check(m, f, cells, [[-1, 1, 4, 4, 1, 1]], "seam x", max_hops=2)
    assert got["counts"][0] == 2 and got["counts"][5] == 6 * 5
    got, _ = check(m, f, cells, [[-3, -3, -1, 1, 1, 1]], "seam y", max_hops=2)
    assert got["counts"][0] == 2 and got["counts"][5] == 5 * 6
    got, _ = check(m, f, cells, [[2, 2, 2, 2, -1, 1]], "seam z", max_hops=2)
    assert got["counts"][0] == 1
    # the body's levels decide by one level
    for box, kw, covered in (([2, 2, 2, 2, -2, -1], dict(levels_below=0), 0), ([2, 2, 2, 2, -2, -1], dict(levels_below=1), 1),
                             ([2, 2, 2, 2, 3, 5], dict(levels_above=1), 0), ([2, 2, 2, 2, 3, 5], dict(levels_above=2), 1)):
        got, _ = check(m, f, cells, [box], ("levels", box, kw), max_hops=2, vacuous_ok=not covered, **kw)
        assert got["counts"][0] == covered and got["counts"][5] == 25
    # wholly off the map, every box void, no box at all: the base or BEYOND, NO_ROW, counts zero but B
    for boxes, B in (([[40, 44, 40, 41, 1, 1]], 1), ([[3, 2, 1, 1, 1, 1], [1, 1, 5, 4, 1, 1], [1, 1, 1, 1, 2, 1]], 3), (np.zeros((0, 6), np.int32), 0)):
        got, want = check(m, f, cells, boxes, ("nothing", B), max_hops=2, vacuous_ok=True)
        assert tuple(got["counts"]) == (0, 0, 0, B, 0, 0, 0, 0) and (got["hops"] == ob.BEYOND).all() and (got["obstacle"] == ob.NO_ROW).all()
    rc, got = raw(m, None, n_boxes=0)
    assert rc == 0 and tuple(got["counts"]) == (0,) * 8 and (got["hops"] == ob.BEYOND).all() and untouched(got)


def test_the_count_on_the_device_and_both_strides_on_real_cluster_records():
    import grid_ndt_amd as g
    import torch
    m, f, cells = floor()
    boxes = [[2, 2, 2, 2, 1, 1], [-5, -4, 6, 6, 1, 1], [7, 7, -7, -7, 1, 1], [-8, -8, -8, -8, 1, 1]]
    for nd in (0, 2, 4, 9, 0xFFFFFFFF):
        got, want = check(m, f, cells, boxes, ("n_boxes_dev", nd), max_hops=2, n_boxes_dev=nd, vacuous_ok=nd == 0)
        assert got["counts"][3] == min(nd, 4) and got["counts"][4] == min(nd, 4)
    check(m, f, cells, boxes, "stride 72", max_hops=2, stride=72)
    # gndt_scan_cluster records as segmentation writes them, read where they lie, cut by its counts[0]
    recs = np.zeros(6, g.TwoDmap.SEG_DTYPE)
    assert recs.itemsize == 72 and recs.dtype.fields["sx_min"][1] == 16
    for k, b in enumerate(boxes):
        recs[k] = (k, 1, 0, 1) + tuple(b) + (0, 0, 0, 0.0, 0.0)
    recs[4:] = (0xFFFFFFFF,) * 4 + (1, 1, 1, 1, 1, 1) + (-1, -1, -1, np.nan, np.nan)         # behind the count: never read
    d = torch.from_numpy(recs.view(np.int32).reshape(6, 18)).cuda()
    wide = d.view(torch.int64)
    seg = {"label": d[:, 0], "sx_min": d[:, 4], "counts": torch.tensor([4, 0, 0, 4], dtype=torch.int32, device="cuda"), "sum_x": wide[:, 5]}
    out = m.obstacle_field(seg, max_hops=2, levels_above=0)
    want = ob.field(f, cells, boxes, max_hops=2)
    assert np.array_equal(out["hops"].cpu().numpy().view(np.uint32), want["hops"]) and np.array_equal(out["counts"].cpu().numpy().view(np.uint32), want["counts"])
    assert np.array_equal(out["obstacle"].cpu().numpy().view(np.uint32), want["obstacle"]) and want["counts"][0] == 5


def test_the_budget_to_the_column():
    m, f, cells = floor()
    boxes = [[2, 2, 2, 2, 1, 1], [9, 8, 1, 1, 1, 1], [-5, -4, 6, 6, 1, 1], [7, 7, -7, -7, 1, 1], [-8, -8, -8, -8, 1, 1]]
    W = ob.budget(ob.resolve(boxes), 1, 2)[4]
    assert list(W) == [49, 49, 105, 154, 203]
    for cols, admitted in ((203, 4), (202, 3), (154, 3), (153, 2), (105, 2), (104, 1), (49, 1), (48, 0)):
        got, want = check(m, f, cells, boxes, ("budget", cols), inflate=1, max_hops=2, max_columns=cols, vacuous_ok=admitted == 0)
        assert got["counts"][6] == 4 - admitted and got["counts"][4] == admitted and got["counts"][3] == 5
        assert not want["admitted"][int(np.flatnonzero(want["dropped"]).min()):].any() if admitted < 4 else True     # once dropped, all later
    # the whole plane is one box of 131 070^2 columns: dropped by the default budget, and the box behind it with it
    got, _ = check(m, f, cells, [[-65535, 65535, -65535, 65535, 1, 1], [2, 2, 2, 2, 1, 1]], "the plane", max_hops=2, vacuous_ok=True)
    assert got["counts"][6] == 2 and got["counts"][0] == 0


# ---- kernel edges: lattices with exact row counts (tests/clearance_ref.LATTICES) -----------------------------------------------------------

@pytest.mark.parametrize("rows", [63, 64, 65, 255, 256, 257])
def test_rows_in_reach_and_window_columns_at_the_wave_and_workgroup_edges(rows):
    """k_obstacle_steps / k_obstacle_round: four lanes a worklist row, `live = t < 4 * len` around the quad exchange; k_obstacle_mark: one
    lane a window column.  On the 32 x 32 lattice a box's window of max_hops = 1 is the box grown by one column: 7 x 9, 8 x 8, 5 x 13,
    15 x 17 and 16 x 16 columns and rows; 257 is the 16 x 16 window and one row more, the corner column of a box that lies off the map."""
    m, f, cells = _tgc().lattice(1024)
    w, h = {63: (7, 9), 64: (8, 8), 65: (5, 13), 255: (15, 17), 256: (16, 16), 257: (16, 16)}[rows]
    boxes = [[9, 9 + w - 3, 9, 9 + h - 3, 1, 1]] + ([[-1, -1, -1, -1, 1, 1]] if rows == 257 else [])
    got, want = check(m, f, cells, boxes, ("rows in reach", rows), max_hops=1)
    assert got["counts"][5] == rows and int(want["w"][0]) == w * h and got["counts"][0] == (w - 2) * (h - 2)
    if rows == 257:
        assert int(want["w"][1]) == 9 and got["counts"][4] == 1


def test_deep_fields_a_base_in_place_and_the_pits_tall_column():
    """40 rounds over a worklist of the whole 32 x 32 lattice, a base merged in place there, and on the device the walk that steps onto
    row 36 of the pit's column, behind its neighbours' step masks"""
    m, f, cells = floor()
    for boxes, kw in (([[3, 4, 5, 5, 1, 1]], dict(max_hops=3)), ([[2, 4, 2, 4, 1, 1], [4, 6, 4, 6, 1, 1]], dict(max_hops=2, inflate=1)),
                      ([[-1, 1, 4, 4, 1, 1], [9, 8, 1, 1, 1, 1]], dict(max_hops=5, outs=("hops",)))):
        check(m, f, cells, boxes, ("floor", kw), **kw)
    m, f, cells = _tgc().lattice(1024)
    got, want = check(m, f, cells, [[20, 20, 20, 20, 1, 1]], "1024 rows, 40 hops", max_hops=40, vacuous_ok=True)
    assert got["counts"][5] == 1024 and got["counts"][2] >= 30
    base = f.clearance(cr.BLOCKED, 32)["hops"]
    check(m, f, cells, [[20, 20, 20, 20, 1, 1], [5, 6, 28, 28, 1, 1]], "1024 rows, a base", max_hops=7, base=base, in_place=True, vacuous_ok=True)
    m, f, cells = _tgc().drawn("pit", cr.pit_cloud)
    z = int(cells["sz"][np.flatnonzero(cells["sx"] == 7)[0]])
    got, _ = check(m, f, cells, [[7, 7, 1, 1, z, z]], "through the pit's tall column", max_hops=8)
    assert got["counts"][2] == 6


def test_a_window_over_the_whole_large_lattice_and_the_second_grid_stride_trip():
    """one box over all 363 x 363 columns: every row of the map is in the worklist, 4 x 131 769 quads are more than one trip of 2048
    workgroups, and the finish's 512 workgroups go 697 rows into their second"""
    m, f, cells = _tgc().lattice(131769)
    n = int(cells["num_nodes"])
    assert 4 * n > 2048 * 256 and n > 512 * 256
    got, want = check(m, f, cells, [[100, 110, 120, 121, 1, 1], [1, 363, 1, 363, 9, 9]], "whole lattice", max_hops=8, entries=(False,))
    assert got["counts"][5] == n and got["counts"][0] == 22 and got["counts"][4] == 1 and got["counts"][2] == 8
    tail = got["hops"][512 * 256:]
    assert (tail == ob.BEYOND).any() and (got["hops"][:512 * 256] != ob.BEYOND).any()


def test_4096_one_cell_boxes_beside_one_zone_of_300_by_300():
    """the marking's balance: the zone's 304^2 window columns and the 4096 x 25 of the small boxes are one run of items; the zone comes
    last, so the bisection's every depth is used"""
    m, f, cells = _tgc().lattice(131769)
    small = [[1 + 5 * (k % 64), 1 + 5 * (k % 64), 1 + 5 * (k // 64), 1 + 5 * (k // 64), 1, 1] for k in range(4096)]
    boxes = small + [[40, 339, 30, 329, 1, 1]]
    got, want = check(m, f, cells, boxes, "balance", max_hops=2, entries=(False,))
    assert got["counts"][3] == 4097 and got["counts"][4] == 4011 and got["counts"][6] == 0 and int(want["W"][-1]) == 4096 * 25 + 304 * 304
    assert (got["obstacle"] == 4096).any() and (got["obstacle"] == 4095).any() and (got["obstacle"] == 0).any()


@pytest.mark.parametrize("max_hops", [1, 1024])
def test_max_hops_of_one_and_of_1024_on_the_41_by_25_lattice(max_hops):
    """1024 hops: a window of 2049^2 columns for one cell, 1025 flag words, rounds that stop when the field is through"""
    m, f, cells = _tgc().lattice("41x25")
    got, want = check(m, f, cells, [[3, 3, 3, 3, 1, 1]], ("max_hops", max_hops), max_hops=max_hops, vacuous_ok=max_hops == 1024)
    assert got["counts"][0] == 1 and got["counts"][2] == (1 if max_hops == 1 else int(want["raw_hops"].max()))
    assert got["counts"][5] == (9 if max_hops == 1 else 1025) and int(want["w"][0]) == (9 if max_hops == 1 else 2049 ** 2)
    if max_hops == 1024:
        assert got["counts"][2] == 60 and got["counts"][1] == 1003           # (no step leads onto the wall's 22 tops)


# ---- outputs ----------------------------------------------------------------------------------------------------------------------------

def test_base_merge_out_of_place_and_in_place_and_every_combination_of_null_outputs():
    m, f, cells = corridor()
    base = f.clearance(cr.BLOCKED, 32)["hops"]
    z = int(cells["sz"][(cells["sx"] == 4) & (cells["sy"] == 6)][0])
    boxes = [[4, 4, 6, 6, z, z]]
    plain, want0 = check(m, f, cells, boxes, "no base", max_hops=4)
    for in_place in (False, True):
        got, want = check(m, f, cells, boxes, ("base", in_place), max_hops=4, base=base, in_place=in_place)
        assert np.array_equal(got["hops"], np.minimum(base, plain["hops"])) and np.array_equal(got["obstacle"], plain["obstacle"])
        assert (got["hops"] < plain["hops"]).any() and (got["hops"] < base).any() and np.array_equal(got["counts"], plain["counts"])
    for outs in (("hops",), ("obstacle",)):
        for b in (None, base):
            got, _ = check(m, f, cells, boxes, ("outs", outs, b is not None), max_hops=4, outs=outs, base=b)
            assert set(got["tails"]) == set(outs)


def test_refused_arguments():
    m, f, cells = floor()
    box = [[2, 2, 2, 2, 1, 1]]
    err = lambda: m._L.gndt_last_error(m._h).decode()
    for kw, text in ((dict(params=False), "null params"), (dict(counts=False), "null counts"), (dict(outs=()), "both NULL"),
                     (dict(stride=20), "box_stride_bytes"), (dict(stride=26), "box_stride_bytes"), (dict(misalign=2), "aligned to 4"),
                     (dict(n_boxes=(1 << 20) + 1), "n_boxes > 2^20"), (dict(inflate=1025), "inflate > 1024"), (dict(max_hops=1025), "max_hops > 1024"),
                     (dict(max_columns=(1 << 28) + 1), "max_columns > 2^28"), (dict(reserved=(0, 1)), "reserved"), (dict(reserved=(7, 0)), "reserved")):
        for host in (False, True):
            rc, got = raw(m, box, host=host, **kw)
            assert rc == ERR_INVALID and text in err() and untouched(got), (kw, host, rc, err())
            assert all((got[k] == SENTINEL).all() for k in kw.get("outs", ("hops", "obstacle"))) and (got["counts"] == SENTINEL).all()
    # a device pointer that is not aligned to 4 bytes: each of the five in turn
    import torch
    from grid_ndt_amd._lib import ObstacleParams
    d_box, buf = dev(box, np.int32), torch.zeros(300, dtype=torch.int32, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    good = dict(n_boxes_dev=p(buf, 1184), base=p(buf, 0), hops=p(buf, 0), obstacle=p(buf, 4 * 260 - 4 * 256 + 0), counts=p(buf, 1152))
    prm2 = ObstacleParams(0, 2, 0, 0, 0)
    for bad in ("n_boxes_dev", "base", "hops", "obstacle", "counts"):
        a = dict(good)
        a[bad] = C.c_void_p(a[bad].value + 2)
        rc = m._L.gndt_obstacle_field_device(m._h, None, p(d_box), 1, 24, a["n_boxes_dev"], C.byref(prm2), a["base"], a["hops"], a["obstacle"],
                                             a["counts"], None)
        assert rc == ERR_INVALID and "aligned to 4 bytes" in err(), (bad, rc, err())
    torch.cuda.synchronize()
    assert not buf.any()
    for host in (False, True):
        rc, _ = raw(m, None, n_boxes=3, host=host)
        assert rc == ERR_INVALID and "null boxes" in err()
    from grid_ndt_amd._lib import ObstacleParams
    prm = ObstacleParams(0, 2, 0, 0, 0)
    assert m._L.gndt_obstacle_field(None, None, None, 0, 24, C.byref(prm), None, None, None, None) == ERR_INVALID
    assert m._L.gndt_obstacle_field_device(None, None, None, 0, 24, None, C.byref(prm), None, None, None, None, None) == ERR_INVALID
    # the limits themselves are taken
    for kw in (dict(inflate=1024, max_hops=1), dict(max_columns=1 << 28), dict(n_boxes_dev=7)):
        rc, got = raw(m, box, **kw)
        assert rc == 0 and got["counts"][0] >= 1, kw
    # no finished build; a stream under capture
    import grid_ndt_amd as g
    import torch
    e = g.TwoDmap(0.5, 0.25)
    e.setCloudFirst((0, 0, 0))
    with pytest.raises(g.GndtError) as ex:
        e.obstacle_field(np.int32(box), host=True)
    assert ex.value.code == ERR_INVALID
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    outs = [torch.zeros(256, dtype=torch.int32, device="cuda") for _ in range(2)] + [torch.zeros(8, dtype=torch.int32, device="cuda")]
    d_box = dev(box, np.int32)
    torch.cuda.synchronize()
    with g.graph_capture(graph, stream=s):
        rc = m._L.gndt_obstacle_field_device(m._h, None, C.c_void_p(d_box.data_ptr()), 1, 24, None, C.byref(prm), None, C.c_void_p(outs[0].data_ptr()),
                                             C.c_void_p(outs[1].data_ptr()), C.c_void_p(outs[2].data_ptr()), C.c_void_p(s.cuda_stream))
        outs[2].add_(1)
    assert rc == ERR_INVALID and "hipGraph" in err()
    graph.replay()
    torch.cuda.synchronize()
    check(m, f, cells, box, "after the refusals", max_hops=2)


# ---- the handle's life ----------------------------------------------------------------------------------------------------------------

def test_repeat_calls_streams_and_a_small_call_after_a_large_one():
    """the marks are stamped, not cleared: the same call again, a call on another stream, and a small call behind one that had every row
    of the map in its worklist all find the earlier calls' stamps, slots and cover words in place"""
    import torch
    m = build(cr.lattice(14641, fr.P), fr.P)
    cells = m.export()
    f = cr.Field(cells)
    assert cells["num_nodes"] == 14641
    small = [[30, 31, 40, 40, 1, 1], [90, 90, 90, 95, 1, 1]]
    first, want = check(m, f, cells, small, "first call on the handle", max_hops=5)          # (also the builder of the column index)
    s = torch.cuda.Stream()
    for stream in (None, s, None, s):
        rc, got = raw(m, small, max_hops=5, stream=stream)
        assert rc == 0 and all(got[k].tobytes() == first[k].tobytes() for k in ("hops", "obstacle", "counts")), stream
    large, _ = check(m, f, cells, [[1, 121, 1, 121, 1, 1], [30, 31, 40, 40, 1, 1]], "large", max_hops=16, vacuous_ok=True, entries=(False,))
    assert large["counts"][5] == 14641 and large["counts"][0] == 14505           # (the walls' tops stand on another level)
    for host in (False, True):
        rc, got = raw(m, small, max_hops=5, host=host)
        assert rc == 0 and untouched(got) and all(got[k].tobytes() == first[k].tobytes() for k in ("hops", "obstacle", "counts")), host
    assert 0 < first["counts"][5] < 14641 // 8


def test_first_builder_of_the_index_and_after_an_update_a_crop_and_a_clear():
    cloud = fr.cells_cloud([(ix, iy) for ix in range(-12, 12) for iy in range(-10, 10)])
    m = build(cloud, fr.P, ATOMIC)
    boxes = [[-2, 2, -1, 1, 1, 1], [9, 9, 9, 9, 1, 1]]

    def fresh(what):
        cells = m.export()
        f = cr.Field(cells)
        assert f.angle_margin_deg > 1e-3, what
        got, _ = check(m, f, cells, boxes, what, max_hops=3, inflate=1)
        return int(cells["num_nodes"]), got

    n0, before = fresh("first call: the column index is this call's")
    more = fr.cells_cloud([(ix, iy) for ix in range(12, 15) for iy in range(-10, 10)])[1:]
    m.change2DMap("slope", dev(more[:, :3]))
    n1, _ = fresh("update")
    m.crop_box((-9, 1000, -1000, 1000), "keep_inside")
    n2, _ = fresh("crop")
    ends = np.float32([[ix * fr.GL + 0.25, 2 * fr.GL + 0.25, -3.0] for ix in range(4, 8)])
    st = m.clear_rays((3.0, 1.25, 4.0), dev(ends))
    n3, after = fresh("clear")
    assert n1 == n0 + 60 and n2 < n1 and st["cleared"] > 0 and n3 == n2 - st["cleared"]
    assert after["counts"][0] > 0
    # everything cropped away: both entry points answer alike, the boxes counted, no slope covered, nothing else written
    m.crop_box((1000, 1010, 1, 2), "keep_inside")
    assert m.sync()[0] == 0
    empty = [raw(m, boxes, host=host, max_hops=3, inflate=1) for host in (False, True)]
    for rc, got in empty:
        assert rc == 0 and untouched(got) and got["counts"][3] == len(boxes) and not got["counts"][:3].any()
    assert empty[0][1]["counts"].tobytes() == empty[1][1]["counts"].tobytes()


# ---- the chain ------------------------------------------------------------------------------------------------------------------------

def test_segment_then_field_then_walk_and_shortcut_on_one_stream():
    """a pallet dropped in the corridor: segment_scan finds it, obstacle_field reads its records and their count where they lie, and the
    walks that were DONE are TOO_CLOSE at the restatement's row — all enqueued on one stream, no result read in between"""
    import torch
    import tests.test_gpu_shortcut as tgs
    from tests import shortcut_ref as sr
    from tests import walk_ref as wr
    m, s, cells = tgs.drawn("obstacle corridor", cr.corridor_cloud, cr.CORRIDOR_P)
    f = s.w.f
    z = int(cells["sz"][(cells["sx"] == 2) & (cells["sy"] == 7)][0])
    assert cells["num_nodes"] == 156 and z == 1
    rng = np.random.default_rng(5)
    # the frame: the corridor as mapped, and a box of points in cell (1, 6) = column (2, 7), levels 2 and 3
    pallet = np.float32(rng.uniform((0.01 + 0.55, 0.01 + 3.05, 0.30), (0.01 + 0.95, 0.01 + 3.45, 0.74), (400, 3)))
    frame = np.concatenate([cr.corridor_cloud()[1:], pallet]).astype(np.float32)
    paths = np.concatenate([_tgc_path((0.76, 0.3), (0.76, 5.7)), _tgc_path((2.76, 0.3), (2.76, 5.7))])       # along columns 2 and 6
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    d_frame, d_paths = dev(frame), dev(paths)
    stream.wait_stream(torch.cuda.current_stream())
    seg = m.segment_scan(d_frame, max_clusters=8, stream=stream)
    field1 = m.obstacle_field(seg, max_hops=8, levels_above=2, obstacle=True, stream=stream)
    free = m.walk_paths(d_paths, stream=stream)
    near = m.walk_paths(d_paths, hops=field1, min_hops=1, stream=stream)
    wide = m.walk_paths(d_paths, hops=field1, min_hops=2, stream=stream)
    stream.synchronize()
    n_seg = int(seg["counts"][0].item())
    assert n_seg == 1
    box = [[int(seg[k][0].item()) for k in ("sx_min", "sx_max", "sy_min", "sy_max", "sz_min", "sz_max")]]
    assert box == [[2, 2, 7, 7, 2, 3]]
    want = ob.field(f, cells, box, max_hops=8, levels_above=2)
    assert np.array_equal(field1["hops"].cpu().numpy().view(np.uint32), want["hops"]) and np.array_equal(field1["counts"].cpu().numpy().view(np.uint32), want["counts"])
    assert np.array_equal(field1["obstacle"].cpu().numpy().view(np.uint32), want["obstacle"]) and want["counts"][0] == 1 and (want["hops"] == ob.BEYOND).any()
    np_ = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
    free, near, wide = np_(free), np_(near), np_(wide)
    assert free["status"].tolist() == [wr.DONE, wr.DONE]
    w = wr.Walker(cells, cr.corridor_cloud()[0], 0.5, 0.25, field=f)
    for got, min_hops in ((near, 1), (wide, 2)):
        info, _, _ = w.walk(paths, hops=want["hops"], min_hops=min_hops, row_cap=0)
        for k in ("status", "steps", "end_row", "hops_min"):
            assert np.array_equal(got[k].view(np.uint32), info[k].view(np.uint32)), (min_hops, k, got[k], info[k])
        # the near path ends on the first slope closer than min_hops to the pallet's column (the slope that fails the check has been
        # entered); the path on the far side of the corridor passes
        assert got["status"].tolist() == [wr.TOO_CLOSE, wr.DONE]
        assert int(cells["sy"][got["end_row"][0]]) == 8 - min_hops and int(cells["sx"][got["end_row"][0]]) == 2
        assert want["hops"][got["end_row"][0]] == min_hops - 1 and got["hops_min"].tolist() == [min_hops - 1, 4]
    # the shortcutter drops the middle of a route that runs up column 2 without the field, and keeps waypoints with it
    route = tgs.route(cells, *tgs.legs((1, 0), (1, 2), (3, 2), (3, 10), (1, 10), (1, 11)))
    rows, lengths = tgs.pack([route])
    without = tgs.check(m, s, rows, lengths, "no field", caps=False)
    with_field = tgs.check(m, s, rows, lengths, "with the field", caps=False, hops=want["hops"], min_hops=2)
    # ... and the same from the field as it lies on the device
    d_rows, d_len = dev(rows.view(np.int32), np.int32), dev(lengths, np.int32)
    stream.wait_stream(torch.cuda.current_stream())
    got = m.shortcut_routes(d_rows, lengths=d_len, hops=field1, min_hops=2, stream=stream)
    stream.synchronize()
    k = int(with_field[0]["waypoints"][0])
    assert int(got["waypoints"][0]) == k and got["waypoint_rows"][0, :k].cpu().tolist() == with_field[1][0, :k].tolist()
    assert int(got["status"][0]) == sr.OK and int(got["hops_min"][0]) == int(with_field[0]["hops_min"][0]) >= 2
    assert without[0]["waypoints"][0] == 2 and with_field[0]["waypoints"][0] > 2 and with_field[0]["status"][0] == sr.OK


def _tgc_path(*xy):
    import tests.test_gpu_walk as tgw
    return tgw.path(*xy)


def test_python_interface_numpy_torch_and_index_boxes():
    import torch
    m, f, cells = floor()
    o = fr.ORIGIN
    lo = np.float32([[o[0] + 0.6, o[1] + 0.6, o[2]], [o[0] - 1.4, o[1] + 2.1, o[2] + 0.01]])
    hi = np.float32([[o[0] + 1.4, o[1] + 0.9, o[2] + 0.2], [o[0] - 0.1, o[1] + 2.4, o[2] + 0.3]])
    boxes = m.index_boxes(lo, hi)
    assert boxes.tolist() == [[2, 3, 2, 2, -1, 1], [-3, -1, 5, 5, 1, 2]]
    want = ob.field(f, cells, boxes, inflate=1, max_hops=3, levels_above=2)
    base = m.clearance(max_hops=32)
    for b in (boxes, torch.from_numpy(boxes).cuda()):
        for host in (False, True):
            out = m.obstacle_field(b, inflate=1, max_hops=3, host=host)            # levels_above: ceil(2 * 0.25 / 0.25) = 2
            np_ = lambda v: (v.cpu().numpy() if hasattr(v, "cpu") else v).view(np.uint32)
            assert isinstance(out["hops"], np.ndarray) == (host or isinstance(b, np.ndarray))
            assert np.array_equal(np_(out["hops"]), want["hops"]) and np.array_equal(np_(out["obstacle"]), want["obstacle"])
            assert np.array_equal(np_(out["counts"]), want["counts"]) and out["hops"].dtype in (np.int32, torch.int32)
            merged = m.obstacle_field(b, inflate=1, max_hops=3, base=base, obstacle=False, host=host)
            assert "obstacle" not in merged and np.array_equal(np_(merged["hops"]), np.minimum(np_(base["hops"]), want["hops"]))
    assert want["counts"][0] == 4 * 3 + 5 * 3
