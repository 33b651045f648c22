"""GPU tier: frontier extraction (gndt_frontiers_device / gndt_frontiers, TwoDmap.frontiers / frontier_points).  Every map is built on
the device; every label, record and count is compared for equality with the restatement (tests/frontier_ref.py) on the handle's own
export, and under REACHED with the device's own cost_export.  Hand-drawn maps whose answer is known beforehand — the floor's ring and
corners, a serpentine of one cluster over many workgroups in shuffled row orders, the origin's seam, diagonals, two storeys — then the
site and the bridge, truncation behind a sentinel, min_size, boxes, repeat calls and streams, crop and update, the round trip into the
planner, and every refused argument.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import frontier_ref as fr
from tests import plan_ref as pr
from tests.gpu_kit import Padded, PaddedCall, build, dev, to_np

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
ATOMIC = 1
SENTINEL = 0x5A5A5A5A
PAD = 3                      # sentinel records on either side of the list
FIELDS = ("sx", "sy", "sz", "count", "first_idx", "mean", "cov", "rough", "normal", "flags")
_scenes = {}


def cfg(candidates=fr.SLOPES, open_rule=fr.OPEN_COLUMN, level_reach=1, min_open=1, link_dz=1):
    return dict(candidates=candidates, open_rule=open_rule, level_reach=level_reach, min_open=min_open, link_dz=link_dz)


def raw(m, c, box=None, min_size=1, cap=None, labels=True, stream=None, host=False, reserved=(0, 0), counts=True, clusters=True):
    """The C entry points.  cap None: as many records as the map has rows.  -> (rc, dict(label, clusters [min(counts[0], cap)],
    counts, buf: the whole record buffer with PAD sentinel records on either side))"""
    from grid_ndt_amd._lib import CropBox, FrontierParams
    n = int(m.sync()[0])
    cap = n if cap is None else cap
    prm = FrontierParams(c["candidates"], c["open_rule"], c["level_reach"], c["min_open"], c["link_dz"], min_size, (C.c_uint32 * 2)(*reserved))
    buf, lab, cnt = Padded(cap, words=16, front=PAD, back=PAD, fill=SENTINEL), Padded(max(n, 1), fill=SENTINEL), Padded(4, fill=SENTINEL)
    rc = PaddedCall(host, stream)(m._L.gndt_frontiers, m._L.gndt_frontiers_device, m._h, None if box is None else C.byref(CropBox(*box)),
                                  C.byref(prm), lab if labels else None, buf if cap and clusters else None, cap, cnt if counts else None)
    k = min(int(cnt.a[0]), cap) if rc == 0 else 0
    return rc, dict(label=lab.a[:n], clusters=buf.a.view(fr.RECORD)[PAD:PAD + k], counts=cnt.a, buf=buf.a)


def untouched(buf, written):
    """the sentinel records before the list and everything behind its `written` records"""
    return Padded.over(buf, words=16, front=PAD, fill=SENTINEL).untouched(written)


def check(m, ref_map, c, cost=None, box=None, min_size=1, what="", **kw):
    """one call against the restatement -> (the call's answer, the restatement)"""
    rc, got = raw(m, c, box=box, min_size=min_size, **kw)
    assert rc == 0, (what, m._L.gndt_last_error(m._h))
    ref = ref_map.frontiers(box=box, h_bits=None if cost is None else cost["h"].view(np.uint32), state=None if cost is None else cost["state"], **c)
    recs, counts = fr.listed(ref, min_size)
    assert np.array_equal(got["counts"], counts), (what, got["counts"], counts)
    if kw.get("labels", True):
        assert np.array_equal(got["label"], ref["label"]), what
    cap = kw.get("cap")
    want = recs if cap is None else recs[:cap]
    assert fr.same_records(got["clusters"], want), (what, fr.diff_records(got["clusters"], want))
    assert untouched(got["buf"], len(want)), what
    return got, ref


def drawn(name, cells, seed=None):
    """a map drawn from a cell list -> (m, ref_map, export)"""
    key = (name, seed)
    if key not in _scenes:
        m = build(fr.cells_cloud(cells, seed), fr.P)
        cells_out = m.export()
        _scenes[key] = (m, fr.Map(cells_out), cells_out)
    return _scenes[key]


def flooded(name):
    """-> (m, ref_map, export, cost_export) of the floor, the drivable site or the bridge, flooded as tests/test_gpu_plan.py floods them"""
    if name not in _scenes:
        if name == "floor":
            cloud, P, goal, robot = pr.floor_cloud(), pr.FLOOR_P, pr.FLOOR_GOAL, pr.FLOOR_ROBOT
        elif name == "site":
            cloud, P, goal, robot = scenes.drivable_site(), scenes.COST_PARAMS, scenes.DRIVABLE_GOAL, dict(radius=0.25)
        else:
            cloud, P, goal, robot = scenes.bridge_ground(), scenes.BRIDGE_PARAMS, pr.BRIDGE_GOALS["deck"], None
        m = build(cloud, P)
        assert m.computeCost(goal, robot)["rc"] == 0
        cells = m.export()
        _scenes[name] = (m, fr.Map(cells), cells, m.cost_export())
    return _scenes[name]


# ---- maps whose answer is known beforehand -------------------------------------------------------------------------------------------

def test_floor_ring_corners_and_nothing():
    m, ref_map, cells, cost = flooded("floor")
    N = pr.FLOOR_N
    got, ref = check(m, ref_map, cfg(fr.REACHED), cost, what="ring")
    rim = (np.abs(cells["sx"] - (N + 1) / 2) == (N - 1) / 2) | (np.abs(cells["sy"] - (N + 1) / 2) == (N - 1) / 2)
    assert (cost["state"][rim] == 1).all()
    rec = got["clusters"]
    assert len(rec) == 1 and int(rec["size"][0]) == 4 * N - 4 == int(rim.sum()) and tuple(got["counts"]) == (1, 4 * N - 4, 1, 0)
    assert np.array_equal(got["label"] != fr.NO_ROW, rim) and int(rec["label"][0]) == int(np.flatnonzero(rim)[0])
    assert (int(rec["sx_min"][0]), int(rec["sx_max"][0]), int(rec["sy_min"][0]), int(rec["sy_max"][0])) == (1, N, 1, N)
    assert int(rec["open_sides"][0]) == 4 * N        # a side each, two at the corners
    # the ring's best row is the rim's cheapest slope of the device's own cost map
    h_rim = np.where(rim, cost["h"], np.float32(np.inf))
    best = int(rec["best_row"][0])
    assert h_rim[best] == h_rim.min() and best == int(np.flatnonzero(h_rim == h_rim.min())[0])
    assert rec["best_h"].view(np.uint32)[0] == cost["h"].view(np.uint32)[best]
    # two open sides: the four corners, each on its own
    got, _ = check(m, ref_map, cfg(fr.REACHED, min_open=2), cost, what="corners")
    assert tuple(got["counts"]) == (4, 4, 4, 0) and (got["clusters"]["size"] == 1).all() and (got["clusters"]["open_sides"] == 2).all()
    # three: none, and the list is not touched
    got, _ = check(m, ref_map, cfg(fr.REACHED, min_open=3), cost, what="none")
    assert tuple(got["counts"]) == (0, 0, 0, 0) and (got["label"] == fr.NO_ROW).all()


@pytest.mark.parametrize("seed", [None, 1, 2, 3])
def test_serpentine_is_one_cluster_in_any_row_order(seed):
    cells = fr.serpentine()
    assert len(cells) == 2177
    m, ref_map, out = drawn("serpentine", cells, seed)
    got, _ = check(m, ref_map, cfg(), what=("serpentine", seed))
    assert tuple(got["counts"]) == (1, 2177, 1, 0) and int(got["clusters"]["size"][0]) == 2177 and (got["label"] == 0).all()
    assert int(got["clusters"]["sum_px"][0]) == 0 and int(got["clusters"]["sum_py"][0]) == 0       # centred on the origin


def test_serpentine_without_connectors_is_33_lines():
    m, ref_map, out = drawn("lines", fr.serpentine(connectors=False), 4)
    got, _ = check(m, ref_map, cfg(), what="lines")
    assert tuple(got["counts"]) == (33, 33 * 65, 33, 0) and (got["clusters"]["size"] == 65).all()
    assert (got["clusters"]["sy_min"] == got["clusters"]["sy_max"]).all()


def test_columns_minus_one_and_one_are_adjacent():
    m, ref_map, out = drawn("origin", [(ix, iy) for ix in range(-3, 3) for iy in range(-3, 3)])
    assert sorted(set(out["sx"].tolist())) == [-3, -2, -1, 1, 2, 3]
    got, _ = check(m, ref_map, cfg(), what="origin")
    rec = got["clusters"]
    assert tuple(got["counts"]) == (1, 20, 1, 0) and int(rec["size"][0]) == 20
    assert (int(rec["sx_min"][0]), int(rec["sx_max"][0]), int(rec["sy_min"][0]), int(rec["sy_max"][0])) == (-3, 3, -3, 3)
    assert int(rec["sum_px"][0]) == int(rec["sum_py"][0]) == -10          # lin: -3 .. 2


def test_diagonal_steps_link_and_a_step_of_two_columns_does_not():
    m, ref_map, _ = drawn("stairs", [(k, k) for k in range(-5, 6)], 7)
    got, _ = check(m, ref_map, cfg(), what="stairs")
    assert tuple(got["counts"]) == (1, 11, 1, 0) and int(got["clusters"]["open_sides"][0]) == 44
    m, ref_map, _ = drawn("broken_stairs", [(k, k) for k in range(-5, 1)] + [(k + 1, k) for k in range(1, 6)], 7)
    got, _ = check(m, ref_map, cfg(), what="broken stairs")
    assert tuple(got["counts"]) == (2, 11, 2, 0) and sorted(got["clusters"]["size"].tolist()) == [5, 6]


def test_two_storeys():
    up = fr.Z_FLOOR + 4 * fr.ZL
    floor = [(ix, iy) for ix in range(-4, 4) for iy in range(-4, 4)]
    # two equal floors over the same columns, and a lone column with both levels
    cells = [(ix, iy, fr.Z_FLOOR) for ix, iy in floor] + [(ix, iy, up) for ix, iy in floor] + [(20, 20, fr.Z_FLOOR), (20, 20, up)]
    m, ref_map, out = drawn("storeys", cells, 11)
    assert len(set(out["sz"].tolist())) == 2 and abs(fr.lin(int(out["sz"].max())) - fr.lin(int(out["sz"].min()))) == 4
    got, _ = check(m, ref_map, cfg(link_dz=1), what="storeys apart")
    assert tuple(got["counts"]) == (4, 58, 4, 0) and sorted(got["clusters"]["size"].tolist()) == [1, 1, 28, 28]
    for dz in (3, 4, 8):
        got, _ = check(m, ref_map, cfg(link_dz=dz), what=("storeys", dz))
        # joined through neighbouring columns from 4 levels on; the lone column's two slopes never
        assert sorted(got["clusters"]["size"].tolist()) == ([1, 1, 28, 28] if dz < 4 else [1, 1, 56])
    # a deck over a larger ground: under OPEN_COLUMN the deck has no frontier, under OPEN_LEVEL its edge is one
    ground = [(ix, iy, fr.Z_FLOOR) for ix in range(-5, 5) for iy in range(-5, 5)]
    deck = [(ix, iy, up) for ix in range(-3, 3) for iy in range(-3, 3)]
    m, ref_map, out = drawn("deck", ground + deck, 12)
    top = out["sz"] == out["sz"].max()
    got, _ = check(m, ref_map, cfg(fr.SLOPES, fr.OPEN_COLUMN), what="deck, column")
    assert tuple(got["counts"]) == (1, 36, 1, 0) and (got["label"][top] == fr.NO_ROW).all()
    got, _ = check(m, ref_map, cfg(fr.SLOPES, fr.OPEN_LEVEL, 1), what="deck, level")
    assert tuple(got["counts"]) == (2, 56, 2, 0) and int((got["label"][top] != fr.NO_ROW).sum()) == 20
    got, _ = check(m, ref_map, cfg(fr.SLOPES, fr.OPEN_LEVEL, 4), what="deck, level 4")
    assert tuple(got["counts"]) == (1, 36, 1, 0)


# ---- the site and the bridge -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["site", "bridge"])
def test_both_modes_and_rules_are_the_restatement(name):
    m, ref_map, cells, cost = flooded(name)
    some = 0
    for cand in (fr.REACHED, fr.SLOPES):
        for rule, reach in ((fr.OPEN_COLUMN, 1), (fr.OPEN_LEVEL, 0), (fr.OPEN_LEVEL, 1), (fr.OPEN_LEVEL, 3)):
            got, _ = check(m, ref_map, cfg(cand, rule, reach), cost, what=(name, cand, rule, reach))
            some += int(got["counts"][1])
    for mo, dz in ((2, 0), (3, 2), (4, 1), (0, 2)):
        check(m, ref_map, cfg(fr.REACHED, fr.OPEN_LEVEL, 1, mo, dz), cost, what=(name, mo, dz))
    assert some > 100


def test_a_short_list_is_cut_and_nothing_is_written_beyond():
    m, ref_map, cells, cost = flooded("site")
    c = cfg(fr.SLOPES, fr.OPEN_LEVEL, 1)
    full, _ = check(m, ref_map, c, what="full")
    n = int(full["counts"][0])
    assert n >= 4
    for cap in (1, 2, n - 1, n, n + 5):
        for host in (False, True):
            check(m, ref_map, c, cap=cap, host=host, what=("cap", cap, host))
    # count only
    rc, got = raw(m, c, cap=0)
    assert rc == 0 and np.array_equal(got["counts"], full["counts"]) and untouched(got["buf"], 0)


def test_min_size_no_labels_and_boxes():
    m, ref_map, cells, cost = flooded("site")
    c = cfg(fr.REACHED, fr.OPEN_LEVEL, 1)
    full, ref = check(m, ref_map, c, cost, what="full")
    sizes = ref["clusters"]["size"]
    assert len(set(sizes.tolist())) > 1
    for ms in (0, 2, int(np.median(sizes)) + 1, int(sizes.max()), int(sizes.max()) + 1):
        got, _ = check(m, ref_map, c, cost, min_size=ms, what=("min_size", ms))
        assert np.array_equal(got["label"], full["label"]) and got["counts"][2] == full["counts"][2]
    check(m, ref_map, c, cost, labels=False, what="no labels")
    # boxes on the floor: a strip through the ring's middle leaves two pieces; a box outside the map nothing
    m, ref_map, cells, cost = flooded("floor")
    got, _ = check(m, ref_map, cfg(fr.REACHED), cost, box=(10, 20, -5, 100), what="strip")
    assert tuple(got["counts"]) == (2, 22, 2, 0) and (got["clusters"]["size"] == 11).all()
    got, _ = check(m, ref_map, cfg(fr.REACHED), cost, box=(pr.FLOOR_N + 10, pr.FLOOR_N + 20, 1, 5), what="outside")
    assert tuple(got["counts"]) == (0, 0, 0, 0)
    got, _ = check(m, ref_map, cfg(fr.SLOPES), box=(0, 1, 0, 1), what="one column")
    assert tuple(got["counts"]) == (1, 1, 1, 0)


def test_repeat_calls_and_a_second_stream_give_the_same_bytes_and_change_nothing():
    import torch
    m, ref_map, cells, cost = flooded("site")
    c = cfg(fr.REACHED, fr.OPEN_LEVEL, 1)
    first, _ = check(m, ref_map, c, cost, what="first")
    s = torch.cuda.Stream()
    for stream in (None, s, None, s):
        rc, got = raw(m, c, stream=stream)
        assert rc == 0
        for k in ("label", "clusters", "counts", "buf"):
            assert got[k].tobytes() == first[k].tobytes(), (k, stream)
    # an answer of another shape in between (the scratch and the list are reused)
    check(m, ref_map, cfg(fr.SLOPES, min_open=2), what="between")
    rc, got = raw(m, c, host=True)
    assert rc == 0 and got["clusters"].tobytes() == first["clusters"].tobytes() and got["label"].tobytes() == first["label"].tobytes()
    after, cost_after = m.export(), m.cost_export()
    for k in FIELDS:
        assert np.asarray(after[k]).tobytes() == np.asarray(cells[k]).tobytes(), k
    assert cost_after["h"].tobytes() == cost["h"].tobytes() and cost_after["state"].tobytes() == cost["state"].tobytes()


def test_after_a_crop_and_after_an_update():
    import grid_ndt_amd as g
    site = scenes.drivable_site(200_000)
    m = build(site, scenes.COST_PARAMS, ATOMIC)
    assert m.computeCost(scenes.DRIVABLE_GOAL)["rc"] == 0
    check(m, fr.Map(m.export()), cfg(fr.REACHED), m.cost_export(), what="before")

    def stale_then_flooded(what):
        cells = m.export()
        ref_map = fr.Map(cells)
        for host in (False, True):
            rc, _ = raw(m, cfg(fr.REACHED), host=host)
            assert rc == ERR_INVALID, what                               # the cost map is the old map's
        with pytest.raises(g.GndtError) as e:
            m.frontiers()
        assert e.value.code == ERR_INVALID
        got, _ = check(m, ref_map, cfg(fr.SLOPES, fr.OPEN_LEVEL, 1), what=what)
        assert got["counts"][1] > 0
        assert m.computeCost(scenes.DRIVABLE_GOAL)["rc"] == 0
        got, _ = check(m, ref_map, cfg(fr.REACHED), m.cost_export(), what=(what, "flooded"))
        assert got["counts"][1] > 0

    x0, x1 = int(m.export()["sx"].min()), int(m.export()["sx"].max())
    m.crop_box((x0 + 5, x1 - 5, -1000, 1000), "keep_inside")
    stale_then_flooded("crop")
    m.change2DMap("slope", dev(site[1:1000, :3] + np.float32([0.0, 0.0, 0.02])))
    stale_then_flooded("update")
    # everything cropped away: four zero counts, nothing else written
    m.crop_box((x1 + 50, x1 + 60, 1, 2), "keep_inside")
    assert m.sync()[0] == 0
    for host in (False, True):
        rc, got = raw(m, cfg(fr.SLOPES), cap=4, host=host)
        assert rc == 0 and tuple(got["counts"]) == (0, 0, 0, 0) and untouched(got["buf"], 0)


# ---- the Python interface and the round trip into the planner ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["floor", "site"])
def test_best_rows_are_starts_the_planner_finds_routes_from(name):
    m, ref_map, cells, cost = flooded(name)
    for host in (False, True):
        f = m.frontiers(labels=True, host=host)                          # reached, column: the defaults
        ref = ref_map.frontiers(fr.REACHED, h_bits=cost["h"].view(np.uint32), state=cost["state"])
        K = len(ref["clusters"])
        assert K >= 1 and tuple(to_np(f["counts"]).tolist()) == (K, ref["rows"], K, 0)
        for k in fr.RECORD.names[:-1]:
            assert to_np(f[k]).tobytes() == ref["clusters"][k].tobytes(), (k, host)
        assert np.array_equal(to_np(f["labels"]).view(np.uint32), ref["label"])
        pts = m.frontier_points(f, "best")
        assert pts.shape == (K, 3) and (hasattr(pts, "cpu") != host)
        rows, info = m.plan_routes(pts, start_mode="nearest_slope", route_cap=8, host=host)
        assert (to_np(info["status"]) == 0).all(), to_np(info["status"])      # GNDT_ROUTE_FOUND
        assert np.array_equal(to_np(info["start_row"]), to_np(f["best_row"]))
        assert np.array_equal(to_np(info["h_start"]).view(np.uint32), to_np(f["best_h"]).view(np.uint32))
        # the centroid: origin + (sum / size + 0.5) * cell, from the records
        cen = to_np(m.frontier_points(f, "centroid"))
        o, rec = np.asarray(m.cloudFirst, np.float64), ref["clusters"]
        want = np.stack([o[0] + (rec["sum_px"] / rec["size"] + 0.5) * m.gridLen, o[1] + (rec["sum_py"] / rec["size"] + 0.5) * m.gridLen,
                         o[2] + (rec["sum_pz"] / rec["size"] + 0.5) * m.zLen], 1).astype(np.float32)
        assert np.array_equal(cen, want)


def test_python_list_capacity_and_options():
    m, ref_map, cells, cost = flooded("site")
    ref = ref_map.frontiers(fr.SLOPES, fr.OPEN_LEVEL, 3, 2, 2)
    recs, counts = fr.listed(ref, 2)
    assert len(recs) >= 3
    box = None
    for host in (False, True):
        f = m.frontiers("slopes", "level", level_reach=3, min_open=2, link_dz=2, min_size=2, box=box, host=host)
        assert "labels" not in f and np.array_equal(to_np(f["counts"]).view(np.uint32), counts)
        assert to_np(f["label"]).view(np.uint32).tolist() == recs["label"].tolist() and to_np(f["size"]).tolist() == recs["size"].tolist()
        f = m.frontiers("slopes", "level", level_reach=3, min_open=2, link_dz=2, min_size=2, max_clusters=2, host=host)
        assert to_np(f["label"]).view(np.uint32).tolist() == recs["label"][:2].tolist() and int(to_np(f["counts"])[0]) == len(recs)
        f = m.frontiers("slopes", "level", level_reach=3, min_open=2, link_dz=2, min_size=2, max_clusters=len(recs) + 2, host=host)
        # room to spare: the host list is cut to what was found; the device list keeps its capacity, size 0 behind the clusters,
        # and such an entry is no point
        assert to_np(f["size"]).tolist() == recs["size"].tolist() + ([] if host else [0, 0])
        for which in ("best", "centroid"):
            pts = to_np(m.frontier_points(f, which))
            assert pts.shape == (len(recs) + (0 if host else 2), 3)
            assert np.isfinite(pts[:len(recs)]).all() and np.isnan(pts[len(recs):]).all()


def test_python_call_on_another_stream_sizes_its_list_on_that_stream():
    """max_clusters=None reads the count-only call's answer back: on the stream it was enqueued on, not on torch's current one"""
    import torch
    m, ref_map, cells, cost = flooded("site")
    ref = ref_map.frontiers(fr.REACHED, fr.OPEN_LEVEL, 1, h_bits=cost["h"].view(np.uint32), state=cost["state"])
    recs, counts = fr.listed(ref)
    assert len(recs) > 10
    for _ in range(3):
        s = torch.cuda.Stream()
        f = m.frontiers("reached", "level", level_reach=1, labels=True, stream=s)
        s.synchronize()
        assert np.array_equal(to_np(f["counts"]).view(np.uint32), counts)
        for k in fr.RECORD.names[:-1]:
            assert to_np(f[k]).tobytes() == recs[k].tobytes(), k
        assert np.array_equal(to_np(f["labels"]).view(np.uint32), ref["label"])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_refused_arguments():
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd._lib import FrontierParams
    m, ref_map, cells, cost = flooded("floor")
    ok = cfg(fr.REACHED)
    for host in (False, True):
        assert raw(m, ok, host=host)[0] == 0
        for bad in (dict(candidates=2), dict(candidates=-1), dict(open_rule=2), dict(open_rule=-1), dict(min_open=5)):
            assert raw(m, dict(ok, **bad), host=host)[0] == ERR_INVALID, bad
        assert raw(m, dict(ok, min_open=4), host=host)[0] == 0
        assert raw(m, ok, reserved=(1, 0), host=host)[0] == ERR_INVALID
        assert raw(m, ok, reserved=(0, 7), host=host)[0] == ERR_INVALID
        for box in ((3, 2, 1, 1), (1, 1, 3, 2), (-65536, 1, 1, 2), (1, 2, 1, 65536), (0, 0, 1, 2), (1, 2, 0, 0)):
            assert raw(m, ok, box=box, host=host)[0] == ERR_INVALID, box
        # the codec's whole range is the whole map (the raster's pixel limit does not apply)
        whole, full = raw(m, ok, host=host), raw(m, ok, box=(-65535, 65535, -65535, 65535), host=host)
        assert full[0] == 0 and full[1]["buf"].tobytes() == whole[1]["buf"].tobytes() and np.array_equal(full[1]["counts"], whole[1]["counts"])
        assert raw(m, ok, clusters=False, host=host)[0] == ERR_INVALID          # NULL clusters with cluster_cap > 0
        assert raw(m, ok, counts=False, host=host)[0] == ERR_INVALID            # NULL counts
    prm = FrontierParams(fr.SLOPES, 0, 1, 1, 1, 1)
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    recs = torch.zeros(32, dtype=torch.int32, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    assert m._L.gndt_frontiers_device(m._h, None, C.byref(prm), None, p(recs), 0, p(cnt), None) == ERR_INVALID      # clusters with cluster_cap 0
    assert m._L.gndt_frontiers_device(m._h, None, C.byref(prm), None, p(recs, 4), 1, p(cnt), None) == ERR_INVALID   # not aligned as the struct is
    assert m._L.gndt_frontiers_device(m._h, None, C.byref(prm), None, p(recs, 8), 1, p(cnt), None) == 0             # 8 bytes are enough
    torch.cuda.synchronize()
    assert int(recs[2]) == 0 and int(recs[3]) == 4 * pr.FLOOR_N - 4 and int(recs[0]) == 0 and int(recs[18]) == 0     # the ring, and only it
    assert m._L.gndt_frontiers_device(m._h, None, None, None, None, 0, p(cnt), None) == ERR_INVALID                 # NULL params
    assert m._L.gndt_frontiers_device(None, None, C.byref(prm), None, None, 0, p(cnt), None) == ERR_INVALID
    assert m._L.gndt_frontiers(None, None, C.byref(prm), None, None, 0, None) == ERR_INVALID
    # REACHED without a cost map, and no finished build
    e = build(fr.cells_cloud([(0, 0), (1, 0)]), fr.P)
    assert raw(e, cfg(fr.REACHED))[0] == ERR_INVALID and raw(e, cfg(fr.SLOPES))[0] == 0
    e = g.TwoDmap(0.5, 0.25)
    e.setCloudFirst((0.0, 0.0, 0.0))
    with pytest.raises(g.GndtError) as err:
        e.frontiers("slopes")
    assert err.value.code == ERR_INVALID
    # a capturing stream: refused, and the capture goes on
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    with g.graph_capture(graph, stream=s):
        rc = m._L.gndt_frontiers_device(m._h, None, C.byref(prm), None, None, 0, p(cnt), C.c_void_p(s.cuda_stream))
        x.add_(1.0)
    assert rc == ERR_INVALID
    graph.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    check(m, ref_map, ok, cost, what="after the refused capture")
