"""GPU tier: scan segmentation (gndt_segment_scan_device / gndt_segment_scan, TwoDmap.segment_scan / cluster_boxes).  Every map is built
on the device; every class, label, record and count is compared for equality with the restatement (tests/segment_ref.py) on the
handle's own export.  Hand-drawn scans over a 16 x 16 floor whose answer is known beforehand — one box, boxes that touch at a corner,
boxes a cell apart, the seams at index 0 on all three axes, the three keyed classes and the points without a key — point orders, a
serpentine over many workgroups, the filters, the count edges of every pass, agreement with gndt_score_poses' own d2 on the drivable
site, and the interface.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import edge_shapes as es
from tests import frontier_ref as fr
from tests import query_ref as qr
from tests import score_ref as sr
from tests import segment_ref as gr
from tests.gpu_kit import Padded, PaddedCall, build, dev, to_np

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
ATOMIC = 1
SENTINEL = 0x5A5A5A5A
PAD = 3                      # sentinel records on either side of the list
WORDS = 18                   # 32-bit words of a record
FIELDS = ("sx", "sy", "sz", "count", "first_idx", "mean", "cov", "rough", "normal", "flags")
_scenes = {}


def raw(m, pts, pose=None, stride=12, cap=None, host=False, stream=None, want_class=True, want_label=True, clusters=True, counts=True,
        reserved=(0, 0), nbh=7, min_count=0, cov_rel=0.0, cov_floor=0.0, novel_d2=0.0, classes=0, min_points=0, connectivity=0,
        min_cluster_points=0, min_cluster_cells=0):
    """The C entry points.  cap None: as many records as the scan has points.  -> (rc, dict(point_class, point_label, clusters
    [min(counts[0], cap)], counts, buf: the whole record buffer with PAD sentinel records on either side))"""
    from grid_ndt_amd._lib import SegmentParams
    pts = np.ascontiguousarray(np.asarray(pts, np.float32)[:, :3])
    n = len(pts)
    if stride == 16:
        pts = np.ascontiguousarray(np.concatenate([pts, np.full((n, 1), 7.0, np.float32)], 1))
    cap = n if cap is None else cap
    prm = SegmentParams(nbh, min_count, cov_rel, cov_floor, novel_d2, classes, min_points, connectivity, min_cluster_points, min_cluster_cells,
                        (C.c_uint32 * 2)(*reserved))
    T = None if pose is None else np.ascontiguousarray(sr.as_poses(pose)[0], np.float64).reshape(12)
    buf, cnt = Padded(cap, words=WORDS, front=PAD, back=PAD, fill=SENTINEL), Padded(4, fill=SENTINEL)
    cls, lab = Padded(max(n, 1), np.uint8, fill=0x5A), Padded(max(n, 1), fill=SENTINEL)
    rc = PaddedCall(host, stream)(m._L.gndt_segment_scan, m._L.gndt_segment_scan_device, m._h, pts, n, stride, T, C.byref(prm),
                                  cls if want_class else None, lab if want_label else None, buf if cap and clusters else None, cap,
                                  cnt if counts else None)
    k = min(int(cnt.a[0]), cap) if rc == 0 else 0
    return rc, dict(point_class=cls.a[:n], point_label=lab.a[:n], clusters=buf.a.view(gr.RECORD)[PAD:PAD + k], counts=cnt.a, buf=buf.a)


def untouched(buf, written):
    """the sentinel records before the list and everything behind its `written` records"""
    return Padded.over(buf, words=WORDS, front=PAD, fill=SENTINEL).untouched(written)


REF_KEYS = ("pose", "nbh", "novel_d2", "classes", "min_points", "connectivity", "min_count", "cov_rel", "cov_floor")


def want(m, cells, pts, **kw):
    return gr.segment(cells, np.float32(m.cloudFirst), m.gridLen, m.zLen, pts, **{k: v for k, v in kw.items() if k in REF_KEYS})


def check(m, cells, pts, what="", ref=None, **kw):
    """one call against the restatement -> (the call's answer, the restatement)"""
    rc, got = raw(m, pts, **kw)
    assert rc == 0, (what, m._L.gndt_last_error(m._h))
    ref = want(m, cells, pts, **kw) if ref is None else ref
    recs, counts = gr.listed(ref, kw.get("min_cluster_points", 0), kw.get("min_cluster_cells", 0))
    assert np.array_equal(got["counts"], counts), (what, got["counts"], counts)
    if kw.get("want_class", True):
        assert np.array_equal(got["point_class"], ref["point_class"]), (what, np.flatnonzero(got["point_class"] != ref["point_class"])[:10])
    else:
        assert (got["point_class"] == 0x5A).all(), what
    if kw.get("want_label", True):
        assert np.array_equal(got["point_label"], ref["point_label"]), (what, np.flatnonzero(got["point_label"] != ref["point_label"])[:10])
    else:
        assert (got["point_label"] == SENTINEL).all(), what
    cap = kw.get("cap")
    listed = recs if cap is None else recs[:cap]
    assert gr.same_records(got["clusters"], listed), (what, gr.diff_records(got["clusters"], listed))
    assert untouched(got["buf"], len(listed)), what
    return got, ref


def floor():
    """the one-storey floor of 16 x 16 columns across the origin, nine points a node -> (m, export, cloud)"""
    if "floor" not in _scenes:
        cloud = fr.cells_cloud(gr.floor_cells())
        m = build(cloud, fr.P)
        _scenes["floor"] = (m, m.export(), cloud)
    return _scenes["floor"]


def site():
    if "site" not in _scenes:
        cloud = scenes.drivable_site()
        m = build(cloud, scenes.COST_PARAMS)
        _scenes["site"] = (m, m.export(), cloud)
    return _scenes["site"]


def site_scan(cloud, seed=3):
    """every 20th point of the site, some of them lifted off the ground, and boxes that were not there when the map was made"""
    rng = np.random.default_rng(seed)
    lifted = cloud[7::160, :3] + np.float32([0, 0, 0.12])
    boxes = [rng.uniform(lo, hi, size=(k, 3)) for lo, hi, k in (((-5, -5, 0.8), (-3.6, -4.2, 2.4), 1500), ((2, 3, 1.0), (2.9, 3.4, 1.6), 600),
                                                                 ((-0.4, -0.4, 0.9), (0.4, 0.4, 1.5), 800), ((20, -20, 1), (21.5, -19, 2), 400))]
    return np.concatenate([cloud[1::20, :3], lifted] + boxes).astype(np.float32)


def one(got):
    assert len(got["clusters"]) == 1
    return got["clusters"][0]


# ---- hand-drawn: the linking rules ---------------------------------------------------------------------------------------------------

def test_one_box_is_one_cluster_with_known_cells_and_bounds():
    m, cells, cloud = floor()
    box = gr.box_cells((2, 4), (-5, -4), (3, 6))                       # 3 x 2 x 4 cells, three points each, levels well above the floor
    got, ref = check(m, cells, gr.cell_points(box, per=3), what="box")
    r = one(got)
    assert (r["label"], r["cells"], r["off_surface"], r["unmapped"]) == (0, 24, 0, 72)
    assert (r["sx_min"], r["sx_max"], r["sy_min"], r["sy_max"], r["sz_min"], r["sz_max"]) == (3, 5, -5, -4, 4, 7)
    assert list(got["counts"]) == [1, 72, 24, 1] and (got["point_label"] == 0).all() and (got["point_class"] == gr.UNMAPPED).all()


def test_corner_contact_links_under_26_and_not_under_6_and_a_gap_never():
    m, cells, cloud = floor()
    a, b = gr.box_cells((0, 1), (0, 1), (3, 4)), gr.box_cells((2, 3), (2, 3), (5, 6))      # b's corner cell touches a's at a corner only
    pts = gr.cell_points(a + b, per=2)
    got, _ = check(m, cells, pts, what="corner, 26")
    assert one(got)["cells"] == 16 and list(got["counts"]) == [1, 32, 16, 1]
    for conn in (26, 0):
        assert check(m, cells, pts, connectivity=conn)[0]["buf"].tobytes() == got["buf"].tobytes()
    got, _ = check(m, cells, pts, what="corner, 6", connectivity=6)
    assert list(got["clusters"]["cells"]) == [8, 8] and list(got["clusters"]["label"]) == [0, 16] and list(got["counts"]) == [2, 32, 16, 2]
    # an edge contact (two axes differ) is no link under 6 either; a face contact is one under both
    edge = gr.cell_points(gr.box_cells((0, 0), (0, 0), (3, 3)) + gr.box_cells((1, 1), (1, 1), (3, 3)), per=1)
    assert list(check(m, cells, edge, connectivity=6)[0]["counts"]) == [2, 2, 2, 2] and list(check(m, cells, edge)[0]["counts"]) == [1, 2, 2, 1]
    face = gr.cell_points(gr.box_cells((0, 1), (0, 0), (3, 3)), per=1)
    assert list(check(m, cells, face, connectivity=6)[0]["counts"]) == [1, 2, 2, 1]
    apart = gr.cell_points(gr.box_cells((0, 1), (0, 1), (3, 4)) + gr.box_cells((3, 4), (0, 1), (3, 4)), per=2)          # column 2 stays empty
    for conn in (26, 6):
        got, _ = check(m, cells, apart, what=("apart", conn), connectivity=conn)
        assert list(got["clusters"]["cells"]) == [8, 8] and list(got["counts"]) == [2, 32, 16, 2]


# ---- hand-drawn: seams and classes ---------------------------------------------------------------------------------------------------

def test_boxes_astride_the_seams_at_index_zero():
    m, cells, cloud = floor()
    for axis, box in enumerate((gr.box_cells((-1, 0), (3, 3), (4, 4)), gr.box_cells((3, 3), (-1, 0), (4, 4)), gr.box_cells((12, 12), (3, 3), (-1, 0)))):
        for conn in (26, 6):
            got, _ = check(m, cells, gr.cell_points(box, per=2), what=("seam", axis, conn), connectivity=conn)
            r = one(got)
            lo, hi = (r["sx_min"], r["sy_min"], r["sz_min"])[axis], (r["sx_max"], r["sy_max"], r["sz_max"])[axis]
            assert (lo, hi) == (-1, 1) and r["cells"] == 2                       # -1 and 1 are neighbours: there is no index 0
    # diagonal across all three seams at once
    diag = gr.cell_points([(-1, -1, -1), (0, 0, 0)], per=1)
    got, _ = check(m, cells, diag, what="diagonal")
    assert list(got["counts"]) == [1, 2, 2, 1] and (one(got)["sx_min"], one(got)["sy_max"], one(got)["sz_min"], one(got)["sz_max"]) == (-1, 1, -1, 1)
    assert list(check(m, cells, diag, connectivity=6)[0]["counts"]) == [2, 2, 2, 2]


def test_the_three_keyed_classes_and_the_points_without_a_key():
    m, cells, cloud = floor()
    on = gr.floor_scan(cloud)
    off = gr.off_plane(cloud)
    beside = gr.cell_points(gr.box_cells((9, 10), (0, 3), (0, 0)), per=2)               # at the floor's height, where the map has no column
    g, o = np.float32(fr.GL), fr.ORIGIN
    odd = np.float32([[np.nan, 0, 0], [0, 0, np.inf], [o[0] + 65536.5 * g, 0, 0], [0, o[1] - 65536.5 * g, 0], [0, 0, o[2] + np.float32(2 ** 21 + 10) * np.float32(fr.ZL)]])
    pts = np.concatenate([on, off, beside, odd])
    for nbh in (7, 1):
        got, ref = check(m, cells, pts, what=("classes", nbh), nbh=nbh)
        assert gr.has_every_class_and_two_clusters(ref)
        c = got["point_class"]
        assert (c[:len(on)] == gr.EXPLAINED).all() and (c[-len(odd):] == gr.UNKEYED).all()
        assert (c[len(on) + len(off):-len(odd)] == gr.UNMAPPED).all()
        if nbh == 7:
            assert (c[len(on):len(on) + len(off)] == gr.OFF_SURFACE).all()
        assert (got["point_label"][-len(odd):] == gr.NO_ROW).all() and (got["point_label"][:len(on)] == gr.NO_ROW).all()
    # the largest index the codec has is keyed, and has no neighbour beyond it
    rim = np.float32([[o[0] + 65535 * g - 0.1, 1, 1], [o[0] + 65534 * g - 0.1, 1, 1]])
    got, _ = check(m, cells, rim, what="rim")
    assert list(got["counts"]) == [1, 2, 2, 1] and one(got)["sx_max"] == 65535


# ---- hand-drawn: point order and filters ---------------------------------------------------------------------------------------------

def _floor_scan_with_boxes(cloud):
    """the floor's own points, points lifted off its plane over its western strip, and boxes: 3-D ones above the floor, one astride
    the seams inside it, two cells that touch at a corner, four beside the floor, two high up, one cell on its own"""
    boxes = gr.box_cells((-3, -2), (2, 3), (2, 4)) + gr.box_cells((-1, 0), (-1, 0), (-1, 1)) + gr.box_cells((3, 3), (3, 3), (3, 3)) \
        + gr.box_cells((4, 4), (4, 4), (4, 4)) + gr.box_cells((8, 9), (0, 1), (0, 0)) + gr.box_cells((-6, -6), (5, 6), (6, 6)) \
        + gr.box_cells((6, 6), (-6, -6), (4, 4))
    off = gr.off_plane(cloud)
    return np.concatenate([gr.floor_scan(cloud), gr.cell_points(boxes, per=3), off[off[:, 0] < -2.0]])


def test_labels_follow_the_smallest_index_in_any_point_order():
    m, cells, cloud = floor()
    pts = _floor_scan_with_boxes(cloud)
    base, ref = check(m, cells, pts, what="natural")
    assert gr.has_every_class_and_two_clusters(ref)

    def strip(recs):          # the records but their labels, in an order of their own
        order = np.lexsort((recs["sz_min"], recs["sy_min"], recs["sx_min"]))
        return [recs[k][order].tobytes() for k in gr.RECORD.names if k != "label"]

    for seed in (1, 2, 3):
        perm = np.random.default_rng(seed).permutation(len(pts))
        got, _ = check(m, cells, pts[perm], what=("shuffled", seed))
        assert strip(got["clusters"]) == strip(base["clusters"])                        # the records but their labels
        assert (np.diff(got["clusters"]["label"].astype(np.int64)) > 0).all()
        inv = np.argsort(perm)
        for r in got["clusters"]:                                                       # the label is the smallest index of the cluster's points
            assert int(r["label"]) == int(np.flatnonzero(got["point_label"] == r["label"]).min())
        assert np.array_equal(got["point_class"][inv], base["point_class"])


@pytest.mark.parametrize("seed", [None, 1, 2])
def test_serpentine_of_3000_cells_is_one_cluster(seed):
    m, cells, cloud = floor()
    lanes = [(ix, iy, 5) for ix, iy in fr.serpentine(half=38)]
    assert 2900 <= len(lanes) <= 3100
    pts = gr.cell_points(lanes, per=1)
    if seed is not None:
        pts = pts[np.random.default_rng(seed).permutation(len(pts))]                    # neighbouring cells in different workgroups
    for conn in (26, 6):
        got, _ = check(m, cells, pts, what=("serpentine", seed, conn), connectivity=conn)
        assert list(got["counts"]) == [1, len(lanes), len(lanes), 1] and one(got)["label"] == 0
    loose = gr.cell_points([(ix, iy, 5) for ix, iy in fr.serpentine(half=38, connectors=False)], per=1)
    assert check(m, cells, loose)[0]["counts"][3] == 39


def test_the_filters_change_exactly_what_the_restatement_says():
    m, cells, cloud = floor()
    pts = _floor_scan_with_boxes(cloud)
    base = want(m, cells, pts)
    assert gr.has_every_class_and_two_clusters(base) and len(base["clusters"]) == 7
    for kw in (dict(min_points=2), dict(min_points=3), dict(min_points=4), dict(classes=1 << gr.OFF_SURFACE), dict(classes=1 << gr.UNMAPPED),
               dict(classes=gr.BOTH), dict(novel_d2=2.0), dict(novel_d2=4000.0), dict(min_count=10)):
        got, ref = check(m, cells, pts, what=kw, **kw)
    for mcp, mcc in ((2, 1), (10, 1), (1, 2), (1, 4), (1 << 30, 1), (4, 3), (0, 0)):
        got, _ = check(m, cells, pts, what=(mcp, mcc), ref=base, min_cluster_points=mcp, min_cluster_cells=mcc)
        assert got["counts"][3] == len(base["clusters"])
    assert want(m, cells, pts, min_points=4)["novel_cells"] < base["novel_cells"]
    assert want(m, cells, pts, classes=1 << gr.UNMAPPED)["novel_points"] < base["novel_points"]
    assert len(gr.listed(base, 10, 1)[0]) < len(base["clusters"]) and len(gr.listed(base, 1, 2)[0]) < len(base["clusters"])


# ---- count edges ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_point_counts_at_the_wave_and_workgroup_edges(n):
    m, cells, cloud = floor()
    pts = _floor_scan_with_boxes(cloud)
    pts = pts[np.random.default_rng(5).permutation(len(pts))][:n]
    for host in (False, True):
        got, ref = check(m, cells, pts, what=(n, host), host=host)
    if n >= 63:
        assert got["counts"][1] > 0 and got["counts"][0] > 0
    if n == 0:
        assert list(got["counts"]) == [0, 0, 0, 0]


@pytest.mark.parametrize("n", [es.CAP, es.CAP + 1, es.CAP + es.BASE])      # (the last: whole waves on a second trip, their held sums merged)
def test_the_classify_grid_cap_as_a_cyclic_batch(n):
    m, cells, cloud = floor()
    scan = _floor_scan_with_boxes(cloud)
    base = scan[np.random.default_rng(9).permutation(len(scan))]
    base = np.concatenate([base, gr.cell_points(gr.box_cells((-30, 30), (20, 40), (7, 9)), per=1)])[:es.BASE]
    assert len(base) == es.BASE
    ref = want(m, cells, base)
    assert gr.has_every_class_and_two_clusters(ref)
    mult = es.multiplicity(n)
    exp = gr.repeated(ref, mult)
    rc, got = raw(m, es.cyclic(base, n), cap=len(ref["clusters"]) + 2)
    assert rc == 0
    recs, counts = gr.listed(exp)
    assert np.array_equal(got["counts"], counts), (got["counts"], counts)
    assert gr.same_records(got["clusters"], recs), gr.diff_records(got["clusters"], recs)
    assert np.array_equal(got["point_class"], es.cyclic(ref["point_class"], n)) and np.array_equal(got["point_label"], es.cyclic(ref["point_label"], n))
    assert untouched(got["buf"], len(recs))


def test_4096_points_in_one_cell_and_in_4096_cells():
    m, cells, cloud = floor()
    pts = np.repeat(gr.cell_points([(2, 2, 5)], per=1), 4096, 0)
    pts[:, 0] += np.linspace(0, 0.1, 4096, dtype=np.float32)
    got, _ = check(m, cells, pts, what="one cell")
    assert list(got["counts"]) == [1, 4096, 1, 1] and one(got)["unmapped"] == 4096 and one(got)["label"] == 0
    got, _ = check(m, cells, pts, what="one cell, min_points beyond", min_points=4097)
    assert list(got["counts"]) == [0, 4096, 0, 0] and (got["point_label"] == gr.NO_ROW).all()
    slab = gr.cell_points(gr.box_cells((-32, 31), (-32, 31), (4, 4)), per=1)            # 4096 cells that all touch: the table at half load
    assert len(slab) == 4096
    got, _ = check(m, cells, slab[np.random.default_rng(4).permutation(4096)], what="4096 cells")
    assert list(got["counts"]) == [1, 4096, 4096, 1]


@pytest.mark.parametrize("k", [1023, 1024, 1025])
def test_cluster_counts_astride_the_list_tile(k):
    m, cells, cloud = floor()
    iso = [(3 * (j % 40) - 60, 3 * (j // 40) - 40, 6) for j in range(k)]                # isolated cells: every one a cluster of its own
    pts = gr.cell_points(iso, per=1)
    got, _ = check(m, cells, pts, what=k)
    assert list(got["counts"]) == [k, k, k, k] and np.array_equal(got["clusters"]["label"], np.arange(k))
    got, _ = check(m, cells, pts, what=(k, "cut"), cap=k - 1)
    assert got["counts"][0] == k and len(got["clusters"]) == k - 1


# ---- agreement with gndt_score_poses -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nbh", [1, 7])
@pytest.mark.parametrize("stride", [12, 16])
def test_the_class_is_a_function_of_score_poses_own_d2(nbh, stride):
    m, cells, cloud = site()
    scan = site_scan(cloud)
    a = np.radians(2.0)
    T = np.array([[np.cos(a), -np.sin(a), 0, 0.21], [np.sin(a), np.cos(a), 0, -0.13], [0, 0, 1, 0.03]])
    for pose in (None, T):
        q = gr.moved(scan, pose)
        xyz = scan if stride == 12 else np.concatenate([scan, np.ones((len(scan), 1), np.float32)], 1)
        sc = m.score_poses(dev(xyz), np.eye(4)[:3] if pose is None else pose, neighbourhood=nbh, per_point=0)
        d2 = sc["d2"].cpu().numpy()
        _, _, _, _, keyed = qr.keys(q, np.float32(m.cloudFirst), m.gridLen, m.zLen)
        cls = gr.class_of(keyed, d2)
        assert all((cls == c).any() for c in (gr.EXPLAINED, gr.OFF_SURFACE, gr.UNMAPPED)), np.bincount(cls, minlength=4)
        rc, got = raw(m, scan, pose=pose, stride=stride, nbh=nbh)
        assert rc == 0 and np.array_equal(got["point_class"], cls), np.flatnonzero(got["point_class"] != cls)[:10]
        assert got["counts"][0] >= 2 and got["counts"][1] == int((cls >= gr.OFF_SURFACE).sum())
        assert (got["point_label"] != gr.NO_ROW).tolist() == (cls >= gr.OFF_SURFACE).tolist()
        for d in (2.0, 50.0):
            rc, other = raw(m, scan, pose=pose, stride=stride, nbh=nbh, novel_d2=d)
            assert rc == 0 and np.array_equal(other["point_class"], gr.class_of(keyed, d2, d))
        if pose is not None:                   # segmenting fl32(T P) at the identity is the same computation
            rc, ident = raw(m, q, stride=stride, nbh=nbh)
            assert rc == 0
            for k in ("point_class", "point_label", "clusters", "counts"):
                assert ident[k].tobytes() == got[k].tobytes(), k


def test_the_site_against_the_restatement():
    m, cells, cloud = site()
    scan = site_scan(cloud)[::3]
    got, ref = check(m, cells, scan, what="site")
    assert gr.has_every_class_and_two_clusters(ref)
    check(m, cells, scan, what="site, 6", connectivity=6, nbh=1, min_points=2, min_cluster_cells=2)


# ---- the interface -------------------------------------------------------------------------------------------------------------------

def test_a_short_list_is_cut_and_nothing_is_written_beyond():
    m, cells, cloud = floor()
    pts = _floor_scan_with_boxes(cloud)
    ref = want(m, cells, pts)
    k = len(ref["clusters"])
    assert k >= 4
    for host in (False, True):
        for cap in (1, k - 1, k, k + 3):
            check(m, cells, pts, what=("cap", cap, host), ref=ref, cap=cap, host=host)
        rc, got = raw(m, pts, cap=0, host=host)                                         # count-only
        assert rc == 0 and got["counts"][0] == k and untouched(got["buf"], 0)


def test_every_combination_of_null_outputs_and_runs_of_equal_cells():
    m, cells, cloud = floor()
    pts = _floor_scan_with_boxes(cloud)
    ref = want(m, cells, pts)
    for host in (False, True):
        for wc in (False, True):
            for wl in (False, True):
                for cap in (None, 0):
                    check(m, cells, pts, what=(host, wc, wl, cap), ref=ref, host=host, want_class=wc, want_label=wl, cap=cap)
    runs = np.concatenate([np.repeat(gr.cell_points([(j % 3, 0, z)], per=1), c, 0)
                           for j, (c, z) in enumerate([(1, 5), (63, 6), (64, 7), (65, 8), (1, 5), (130, 9), (2, 6), (61, 5)])])
    check(m, cells, runs, what="runs across wave borders")


def test_repeat_calls_streams_and_a_small_call_after_a_large_one():
    import torch
    m, cells, cloud = floor()
    pts = _floor_scan_with_boxes(cloud)
    first, ref = check(m, cells, pts, what="first")
    s = torch.cuda.Stream()
    for stream in (None, s, None, s):
        rc, got = raw(m, pts, stream=stream)
        assert rc == 0
        for k in ("point_class", "point_label", "clusters", "counts", "buf"):
            assert got[k].tobytes() == first[k].tobytes(), (k, stream)
    big = np.concatenate([pts] * 40 + [gr.cell_points(gr.box_cells((-40, 40), (-40, 40), (9, 10)), per=2)])       # a larger table and scratch
    assert check(m, cells, big[::7], what="large")[0]["counts"][0] > 0
    rc, got = raw(m, big)
    assert rc == 0
    small, _ = check(m, cells, pts[:300], what="small after large")
    for host in (True, False):
        rc, got = raw(m, pts, host=host)
        assert rc == 0
        for k in ("point_class", "point_label", "clusters", "counts"):
            assert got[k].tobytes() == first[k].tobytes(), (k, host)
    after = m.export()
    for k in FIELDS:
        assert np.asarray(after[k]).tobytes() == np.asarray(cells[k]).tobytes(), k      # the map is not modified


def test_after_an_update_and_after_a_crop():
    cloud = fr.cells_cloud(gr.floor_cells())
    m = build(cloud, fr.P, ATOMIC)
    box = gr.cell_points(gr.box_cells((1, 2), (1, 2), (3, 3)), per=9)
    pts = np.concatenate([gr.floor_scan(cloud), box])
    got, _ = check(m, m.export(), pts, what="before")
    assert (got["point_class"][-len(box):] == gr.UNMAPPED).all()
    m.change2DMap("slope", dev(box))                                     # the box joins the map: its points are explained by their own nodes
    got, _ = check(m, m.export(), pts, what="update")
    assert (got["point_class"][-len(box):] == gr.EXPLAINED).all() and got["counts"][1] == 0
    m.crop_box((1, 8, -8, 8), "keep_inside")                              # the floor's west half leaves: its points find no node
    got, ref = check(m, m.export(), pts, what="crop")
    west = pts[:, 0] < fr.ORIGIN[0] - 0.6
    assert west.any() and (got["point_class"][west] == gr.UNMAPPED).all() and (got["point_class"][-len(box):] == gr.EXPLAINED).all()
    m.crop_box((100, 101, 1, 2), "keep_inside")
    assert m.sync()[0] == 0                                               # a map without rows: everything keyed is unmapped
    got, _ = check(m, m.export(), pts, what="empty map")
    assert (got["point_class"] == gr.UNMAPPED).all()


def test_python_wrappers_shapes_and_cluster_boxes():
    import torch
    m, cells, cloud = floor()
    box = gr.box_cells((2, 4), (-5, -4), (3, 6)) + gr.box_cells((-1, 0), (7, 7), (-1, 0))
    pts = np.concatenate([gr.floor_scan(cloud), gr.cell_points(box, per=3)])
    ref = want(m, cells, pts)
    k = len(ref["clusters"])
    assert k == 2
    for src in (dev(pts), pts, dev(np.concatenate([pts, np.ones((len(pts), 1), np.float32)], 1))):
        on_dev = hasattr(src, "cpu")
        seg = m.segment_scan(src, labels=True)
        assert isinstance(seg["label"], torch.Tensor) == on_dev
        for f in gr.RECORD.names:
            got = np.ascontiguousarray(np.ascontiguousarray(to_np(seg[f])).astype(gr.RECORD[f]))
            assert seg[f].shape == (k,) and got.tobytes() == np.ascontiguousarray(ref["clusters"][f]).tobytes(), f
        assert list(to_np(seg["counts"])) == [k, ref["novel_points"], ref["novel_cells"], k]
        assert np.array_equal(to_np(seg["point_class"]), ref["point_class"]) and seg["point_class"].dtype in (np.uint8, torch.uint8)
        assert np.array_equal(to_np(seg["point_label"]).view(np.uint32), ref["point_label"])
        wide = m.segment_scan(src, max_clusters=5)
        assert "point_class" not in wide and wide["label"].shape == ((5,) if on_dev else (k,)) and int(to_np(wide["counts"])[0]) == k
        short = m.segment_scan(src, max_clusters=1)
        assert short["label"].shape == (1,) and int(to_np(short["counts"])[0]) == k and int(to_np(short["label"])[0]) == int(ref["clusters"]["label"][0])
        boxes, cen = m.cluster_boxes(wide)
        assert boxes.shape == (wide["label"].shape[0], 2, 3) and cen.shape == (wide["label"].shape[0], 3)
        boxes, cen = to_np(boxes), to_np(cen)
        o = np.float64(fr.ORIGIN)
        want_lo = o + np.float64([2, -5, 3]) * [fr.GL, fr.GL, fr.ZL]                    # the first box: cells 2..4, -5..-4, levels 3..6
        want_hi = o + np.float64([5, -3, 7]) * [fr.GL, fr.GL, fr.ZL]
        assert np.allclose(boxes[0, 0], want_lo, atol=1e-5) and np.allclose(boxes[0, 1], want_hi, atol=1e-5)
        assert np.allclose(boxes[1, 0], o + np.float64([-1, 7, -1]) * [fr.GL, fr.GL, fr.ZL], atol=1e-5)         # astride the seams
        assert np.allclose(boxes[1, 1], o + np.float64([1, 8, 1]) * [fr.GL, fr.GL, fr.ZL], atol=1e-5)
        first = gr.cell_points(gr.box_cells((2, 4), (-5, -4), (3, 6)), per=3).astype(np.float64)
        assert np.allclose(cen[0], first.mean(0), atol=2e-3) and (cen[:k] >= boxes[:k, 0]).all() and (cen[:k] <= boxes[:k, 1]).all()
        if on_dev:
            assert np.isnan(boxes[k:]).all() and np.isnan(cen[k:]).all() and not np.isnan(boxes[:k]).any()
    both = m.segment_scan(dev(pts), classes=("off_surface", "unmapped"), connectivity=6, neighbourhood=1, min_points=2, min_cluster_cells=2)
    assert int(to_np(both["counts"])[3]) >= 1
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        src = dev(pts)
    seg = m.segment_scan(src, pose=np.eye(4), stream=s)
    s.synchronize()
    assert seg["label"].shape == (k,) and list(to_np(seg["cells"])) == list(ref["clusters"]["cells"])
    empty = m.segment_scan(dev(np.zeros((0, 3), np.float32)), labels=True)
    assert empty["label"].shape == (0,) and list(to_np(empty["counts"])) == [0, 0, 0, 0] and empty["point_class"].shape == (0,)


def test_refused_arguments():
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd._lib import SegmentParams
    m, cells, cloud = floor()
    pts = _floor_scan_with_boxes(cloud)[:500]
    for host in (False, True):
        assert raw(m, pts, host=host)[0] == 0
        for bad in (dict(nbh=0), dict(nbh=2), dict(nbh=-7), dict(connectivity=1), dict(connectivity=8), dict(connectivity=18), dict(min_count=1),
                    dict(min_count=2), dict(min_count=-3), dict(cov_rel=-1.0), dict(cov_floor=float("nan")), dict(novel_d2=-0.5),
                    dict(novel_d2=float("inf")), dict(classes=1), dict(classes=2), dict(classes=1 << 4), dict(classes=gr.BOTH | 1),
                    dict(reserved=(1, 0)), dict(reserved=(0, 7)), dict(stride=8), dict(stride=20), dict(clusters=False), dict(counts=False)):
            kw = dict(bad)
            stride = kw.pop("stride", 12)
            if stride in (12, 16):
                assert raw(m, pts, host=host, **kw)[0] == ERR_INVALID, bad
        for ok in (dict(min_count=3), dict(connectivity=6), dict(connectivity=26), dict(classes=gr.BOTH), dict(min_count=50)):
            assert raw(m, pts, host=host, **ok)[0] == 0, ok
    prm = SegmentParams(7)
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    recs = torch.zeros(64, dtype=torch.int32, device="cuda")
    xyz = dev(pts)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    call = lambda *a: m._L.gndt_segment_scan_device(*a)
    n = len(pts)
    assert call(m._h, p(xyz), n, 12, None, C.byref(prm), None, None, None, 0, p(cnt), None) == 0
    for stride in (0, 8, 20):
        assert call(m._h, p(xyz), n, stride, None, C.byref(prm), None, None, None, 0, p(cnt), None) == ERR_INVALID
    assert call(m._h, None, n, 12, None, C.byref(prm), None, None, None, 0, p(cnt), None) == ERR_INVALID                  # null points
    assert call(m._h, p(xyz), 1 << 32, 12, None, C.byref(prm), None, None, None, 0, p(cnt), None) == ERR_INVALID           # n >= 2^32
    assert call(m._h, p(xyz), n, 12, None, C.byref(prm), None, None, p(recs), 0, p(cnt), None) == ERR_INVALID             # clusters with cap 0
    assert call(m._h, p(xyz), n, 12, None, C.byref(prm), None, None, p(recs, 4), 1, p(cnt), None) == ERR_INVALID          # not aligned
    assert call(m._h, p(xyz), n, 12, None, C.byref(prm), None, None, p(recs, 8), 1, p(cnt), None) == 0
    assert call(m._h, p(xyz), n, 12, None, None, None, None, None, 0, p(cnt), None) == ERR_INVALID                        # null params
    assert call(None, p(xyz), n, 12, None, C.byref(prm), None, None, None, 0, p(cnt), None) == ERR_INVALID
    assert m._L.gndt_segment_scan(None, None, 0, 12, None, C.byref(prm), None, None, None, 0, None) == ERR_INVALID
    with pytest.raises(g.GndtError) as err:
        m.segment_scan(xyz, classes=1 << gr.EXPLAINED)
    assert err.value.code == ERR_INVALID
    # no finished build
    e = g.TwoDmap(0.5, 0.25)
    e.setCloudFirst((0.0, 0.0, 0.0))
    with pytest.raises(g.GndtError) as err:
        e.segment_scan(xyz)
    assert err.value.code == ERR_INVALID
    # a capturing stream: refused, and the capture goes on
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    with g.graph_capture(graph, stream=s):
        rc = call(m._h, p(xyz), n, 12, None, C.byref(prm), None, None, None, 0, p(cnt), C.c_void_p(s.cuda_stream))
        x.add_(1.0)
    assert rc == ERR_INVALID
    graph.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    check(m, cells, pts, what="after the refused capture")
