"""CPU tier: scan segmentation's per-element code (grid_ndt_amd/csrc/gndt_segment.hpp: the class of a point, the cell table, the links
with the frontiers' union-find, the record reduction), compiled with g++ into tests/_segment_shim.so and run one item after another in
natural and in shuffled item order, against the restatement (tests/segment_ref.py: score_ref's d2, a dict of cells, a breadth-first
search) on maps the oracle builds and on 300 random occupancy lattices — every class, label, record field and count, for equality;
parent[x] <= x after every union; the table at exactly half load and with every point in one cell; and the product entry points refuse
to run without a GPU.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import frontier_ref as fr
from tests import score_ref as sr
from tests import segment_ref as gr
from tests.host_emulation import MAP, HostMap, load_shim

_shim = None


def shim():
    global _shim
    if _shim is None:
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        _shim = load_shim("segment_shim.cpp", "_segment_shim.so", {
            "gshim_table_slots": ([u64], u64),
            "gshim_z_image": ([C.c_float], u32),
            "gshim_z_bits": ([u32], u32),
            "gshim_segment": ([C.c_int, vp, u32, u32, vp, MAP, u32, vp, C.c_float, vp, vp, vp, vp, vp, u32, vp, vp], C.c_int64),
        })
    return _shim


def run(m, pts, pose=None, nbh=7, novel_d2=0.0, classes=0, min_points=0, connectivity=0, min_cluster_points=0, min_cluster_cells=0,
        order=None, cap=None, **score_params):
    """the passes over the scan on map m -> dict(point_class, point_label, clusters [min(listed, cap)], counts, tail, table); 0 means
    the default, which the entry point settles before the kernels see it"""
    pts = np.ascontiguousarray(pts, np.float32)
    n = len(pts)
    prm = sr.defaults(**score_params)
    score = np.array([prm["cov_rel"], prm["cov_floor"]], np.float64)
    rule = np.array([classes or gr.BOTH, max(min_points, 1), connectivity or 26, max(min_cluster_points, 1), max(min_cluster_cells, 1)], np.uint32)
    cap = n if cap is None else cap
    cls = np.full(max(n, 1), 0xEE, np.uint8)
    lab = np.full(max(n, 1), 0xDEADBEEF, np.uint32)
    clusters = np.full(max(cap, 1) * 18, 0xA5A5A5A5, np.uint32).view(gr.RECORD)
    counts = np.full(4, 0xDEADBEEF, np.uint32)
    table = np.zeros(3, np.uint32)
    o = None if order is None else np.ascontiguousarray(order, np.uint32)
    T = None if pose is None else np.ascontiguousarray(sr.as_poses(pose)[0]).reshape(12)
    rc = shim().gshim_segment(nbh, pts.ctypes.data, pts.shape[1], n, None if T is None else T.ctypes.data, m.shim_map(), prm["min_count"],
                              score.ctypes.data, float(novel_d2) if novel_d2 else float(gr.NOVEL_D2), rule.ctypes.data,
                              None if o is None else o.ctypes.data, cls.ctypes.data, lab.ctypes.data, clusters.ctypes.data,
                              cap, counts.ctypes.data, table.ctypes.data)
    assert rc == 0, f"table full ({rc})" if rc < 0 else f"parent[x] <= x failed at index {rc - 1}"
    k = min(int(counts[0]), cap)
    return dict(point_class=cls[:n], point_label=lab[:n], clusters=clusters[:k], counts=counts, tail=clusters[k:], table=table)


def want(m, pts, **kw):
    kw = {k: v for k, v in kw.items() if k not in ("order", "cap", "min_cluster_points", "min_cluster_cells")}
    return gr.segment(m.cells, m.origin, m.P["grid_len"], m.P["z_len"], pts, **kw)


def check(m, pts, what="", ref=None, **kw):
    got = run(m, pts, **kw)
    ref = want(m, pts, **kw) if ref is None else ref
    recs, counts = gr.listed(ref, kw.get("min_cluster_points", 0), kw.get("min_cluster_cells", 0))
    assert np.array_equal(got["counts"], counts), (what, got["counts"], counts)
    assert np.array_equal(got["point_class"], ref["point_class"]), (what, np.flatnonzero(got["point_class"] != ref["point_class"])[:10])
    assert np.array_equal(got["point_label"], ref["point_label"]), (what, np.flatnonzero(got["point_label"] != ref["point_label"])[:10])
    assert gr.same_records(got["clusters"], recs), (what, gr.diff_records(got["clusters"], recs))
    return got, ref


# ---- scenes: a map the oracle builds and a scan with points of every class -----------------------------------------------------------
def _floor_scene():
    cloud = fr.cells_cloud(gr.floor_cells())
    boxes = gr.box_cells((-3, -2), (1, 2), (2, 4)) + gr.box_cells((-1, 0), (-1, 0), (-1, 1)) + gr.box_cells((3, 3), (3, 3), (3, 3)) \
        + gr.box_cells((4, 4), (4, 4), (4, 4)) + gr.box_cells((8, 9), (0, 1), (0, 0)) + gr.box_cells((-6, -6), (5, 6), (6, 6))
    odd = np.float32([[np.nan, 0, 0], [0, np.inf, 0], [1e9, 0, 0], [0, 0, -1e7]])
    scan = np.concatenate([gr.floor_scan(cloud), gr.cell_points(boxes, per=3), gr.off_plane(cloud), odd])
    return cloud, fr.P, scan


def _site_scene():
    cloud = scenes.drivable_site(n=60_000, half=12.0)
    rng = np.random.default_rng(3)
    ground = cloud[1::4, :3]
    lifted = cloud[2::9, :3] + np.float32([0, 0, 0.12])
    boxes = [rng.uniform(lo, hi, size=(k, 3)) for lo, hi, k in (((-5, -5, 0.8), (-3.6, -4.2, 2.4), 500), ((2, 3, 1.0), (2.9, 3.4, 1.6), 200),
                                                                 ((-0.4, -0.4, 0.9), (0.4, 0.4, 1.5), 300), ((13, 0, 0), (14.5, 1, 1), 150))]
    scan = np.concatenate([ground, lifted] + boxes).astype(np.float32)
    return cloud, scenes.COST_PARAMS, scan


SCENES = {"floor": _floor_scene, "site": _site_scene}
_maps = {}


def _scene(name):
    if name not in _maps:
        cloud, P, scan = SCENES[name]()
        _maps[name] = (HostMap(cloud, P), scan)
    return _maps[name]


# ---- 1. the pieces -------------------------------------------------------------------------------------------------------------------
def test_z_image_orders_like_the_floats_and_comes_back():
    z = np.float32([-np.inf, -3e38, -1.5, -1e-40, -0.0, 0.0, 1e-40, 1.5, 3e38, np.inf])
    img = [shim().gshim_z_image(float(v)) for v in z]
    assert img == sorted(img) and len(set(img)) == len(img)
    assert [int(v) for v in gr.z_image(z)] == img
    for v, i in zip(z, img):
        assert shim().gshim_z_bits(i) == int(np.float32(v).view(np.uint32))


def test_table_slots_keep_n_cells_at_half_load():
    for n, slots in ((0, 1024), (1, 1024), (512, 1024), (513, 2048), (4096, 8192), (4097, 16384), (131072, 262144), (1 << 30, 1 << 31)):
        assert shim().gshim_table_slots(n) == slots


# ---- 2. scenes against the restatement, in natural and shuffled item order -----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("nbh", (1, 7))
def test_every_class_label_record_and_count_is_the_restatement(name, nbh):
    m, scan = _scene(name)
    ref = want(m, scan, nbh=nbh)
    assert gr.has_every_class_and_two_clusters(ref), (name, np.bincount(ref["point_class"], minlength=4), len(ref["clusters"]))
    rng = np.random.default_rng(7)
    first, _ = check(m, scan, what=(name, nbh), ref=ref, nbh=nbh)
    for k in range(2):
        got, _ = check(m, scan, what=(name, nbh, "order", k), ref=ref, nbh=nbh, order=rng.permutation(len(scan)))
        assert got["clusters"].tobytes() == first["clusters"].tobytes() and got["point_label"].tobytes() == first["point_label"].tobytes()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_parameters_change_what_the_restatement_says(name):
    m, scan = _scene(name)
    base = want(m, scan)
    assert gr.has_every_class_and_two_clusters(base)
    rng = np.random.default_rng(11)
    for kw in (dict(classes=1 << gr.OFF_SURFACE), dict(classes=1 << gr.UNMAPPED), dict(min_points=2), dict(min_points=4), dict(connectivity=6),
               dict(novel_d2=2.0), dict(novel_d2=400.0), dict(min_count=6), dict(cov_rel=0.1, cov_floor=1e-3)):
        check(m, scan, what=(name, kw), order=rng.permutation(len(scan)), **kw)
    changed = [want(m, scan, **kw) for kw in (dict(classes=1 << gr.UNMAPPED), dict(min_points=4), dict(connectivity=6))]
    assert changed[0]["novel_points"] < base["novel_points"] and changed[1]["novel_cells"] < base["novel_cells"]
    assert len(changed[2]["clusters"]) >= len(base["clusters"])
    # the cluster-size filters leave clusters out of the list, not out of the labels or of counts[3]
    for mcp, mcc in ((0, 0), (2, 1), (10, 1), (1, 2), (1, 4), (1 << 30, 1), (4, 3)):
        check(m, scan, what=(name, mcp, mcc), ref=base, min_cluster_points=mcp, min_cluster_cells=mcc)


def test_a_pose_is_the_moved_scan_at_the_identity():
    m, scan = _scene("floor")
    a = np.radians(3.0)
    T = np.array([[np.cos(a), -np.sin(a), 0, 0.31], [np.sin(a), np.cos(a), 0, -0.17], [0, 0, 1, 0.02]])
    Tinv = np.linalg.inv(np.vstack([T, [0, 0, 0, 1]]))[:3]
    back = sr.transform(Tinv, scan)                       # a scan that T takes (nearly) onto the scene's
    got, ref = check(m, back, what="pose", pose=T)
    assert gr.has_every_class_and_two_clusters(ref)
    q = sr.transform(T, back)
    ident, _ = check(m, q, what="moved")
    assert ident["clusters"].tobytes() == got["clusters"].tobytes() and np.array_equal(ident["point_label"], got["point_label"])
    assert np.array_equal(ident["point_class"], got["point_class"])


def test_a_short_list_is_cut_and_the_rest_untouched():
    m, scan = _scene("floor")
    full = run(m, scan)
    n = int(full["counts"][0])
    assert n >= 3
    for cap in (0, 1, n - 1, n, n + 3):
        got = run(m, scan, cap=cap)
        assert np.array_equal(got["counts"], full["counts"])
        assert got["clusters"].tobytes() == full["clusters"][:cap].tobytes()
        assert (got["tail"].view(np.uint32) == 0xA5A5A5A5).all()


# ---- 3. the table's edges ------------------------------------------------------------------------------------------------------------
def test_the_table_at_exactly_half_load():
    m, _ = _scene("floor")
    cells = gr.box_cells((-16, 15), (-8, 7), (3, 3))          # 512 isolated-by-nothing cells in one slab: one cluster of 512 cells
    assert len(cells) == 512
    pts = gr.cell_points(cells, per=1)
    rng = np.random.default_rng(2)
    got, ref = check(m, pts, what="half load", order=rng.permutation(512))
    assert list(got["table"][:2]) == [512, 1024] and int(got["counts"][2]) == 512 and int(got["counts"][3]) == 1
    far = [(3 * k - 700, 40, 9) for k in range(512)]          # and 512 cells that touch nothing
    got, ref = check(m, gr.cell_points(far, per=1), what="half load, isolated")
    assert list(got["table"][:2]) == [512, 1024] and int(got["counts"][3]) == 512


def test_every_point_in_one_cell():
    m, _ = _scene("floor")
    pts = np.repeat(gr.cell_points([(2, 2, 5)], per=1), 4096, 0)
    pts[:, 0] += np.linspace(0, 0.1, 4096, dtype=np.float32)
    for order in (None, np.random.default_rng(1).permutation(4096)):
        got, ref = check(m, pts, what="one cell", order=order)
        assert list(got["counts"]) == [1, 4096, 1, 1] and int(got["table"][0]) == 1
        assert int(got["clusters"]["unmapped"][0]) == 4096 and int(got["clusters"]["label"][0]) == 0
    got, _ = check(m, pts, what="one cell, min_points beyond", min_points=4097)
    assert list(got["counts"]) == [0, 4096, 0, 0] and (got["point_label"] == gr.NO_ROW).all()


def test_runs_of_equal_cells_across_wave_borders():
    m, _ = _scene("floor")
    runs = [(1, 5), (63, 6), (64, 7), (65, 8), (1, 5), (130, 9), (2, 6), (61, 5)]          # (points, level): a cell again after others
    pts = np.concatenate([np.repeat(gr.cell_points([(k % 3, 0, z)], per=1), c, 0) for k, (c, z) in enumerate(runs)])
    got, ref = check(m, pts, what="runs")
    assert int(got["counts"][2]) == 7 and int(got["counts"][1]) == len(pts)


# ---- 4. random occupancy lattices ----------------------------------------------------------------------------------------------------
def lattice_scan(rng, m_cloud):
    """a random occupancy of the cells around and above the floor, one to three points a cell, the floor's own points among them, in
    a shuffled point order; the lattice lies across the seams at 0 on all three axes"""
    fill = rng.uniform(0.04, 0.1)          # (26-connected cells percolate at about 0.1: several clusters below)
    side, lo, hi = int(rng.integers(6, 11)), -2, int(rng.integers(3, 7))
    cells = [(ix, iy, iz) for ix in range(-side, side) for iy in range(-side, side) for iz in range(lo, hi) if rng.random() < fill]
    pts = [gr.cell_points(cells[k::3], per=k + 1) for k in range(3)] + [gr.floor_scan(m_cloud, every=int(rng.integers(5, 12)))]
    pts = np.concatenate(pts)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


def test_fuzz_300_random_occupancy_lattices():
    m, _ = _scene("floor")
    cloud = fr.cells_cloud(gr.floor_cells())
    rng = np.random.default_rng(20250301)
    for k in range(300):
        pts = lattice_scan(rng, cloud)
        base = want(m, pts)
        # the restatement alone: the fuzz cannot pass on empty answers
        assert gr.has_every_class_and_two_clusters(base) and base["clusters"]["cells"].max() >= 2, k
        check(m, pts, what=(k, "base"), ref=base)
        kw = dict(nbh=int(rng.choice([1, 7])), classes=int(rng.choice([0, 4, 8, 12])), min_points=int(rng.integers(0, 4)),
                  connectivity=int(rng.choice([0, 6, 26])))
        check(m, pts, what=(k, kw), order=rng.permutation(len(pts)), min_cluster_points=int(rng.integers(0, 6)),
              min_cluster_cells=int(rng.integers(0, 4)), **kw)


# ---- 5. the product ------------------------------------------------------------------------------------------------------------------
def test_no_cpu_fallback_for_segment_scan(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    with pytest.raises(g.GndtError) as e:
        m.segment_scan(np.zeros((10, 3), np.float32))
    assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
    # the device entry point: without a device no handle is made, and a null handle is refused before anything else
    from grid_ndt_amd._lib import SegmentParams
    counts = np.zeros(4, np.uint32)
    assert m._h is None
    for fn, extra in ((m._L.gndt_segment_scan_device, (None,)), (m._L.gndt_segment_scan, ())):
        assert fn(None, None, 0, 12, None, C.byref(SegmentParams(7)), None, None, None, 0, C.c_void_p(counts.ctypes.data), *extra) != 0
