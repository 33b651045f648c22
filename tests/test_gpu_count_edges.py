"""GPU tier: the consumers at the counts where their launches change shape (tests/edge_shapes.py derives every count from the headers'
constants): the second trip of the grid-stride loops (item 524 288 on), the carry of the one-workgroup scans (row 1 048 576 on), the
reduce strides of the score sums (tile 4096, and 2048 for the derivatives), and the tile, vector and wave tails.  Every case compares
with the consumer's own restatement under that consumer's own tolerance rule; nothing is looser than in the consumer's module.

Batches on the small map ("41x25") repeat a base list of 4093 items (prime), so the restatement runs once on the base and a batch's
expected outputs are ref[i % 4093]; counts, pass words and sums are sums over the multiplicities.  The row-count edges run on one-storey
lattices of exactly that many rows (edge_shapes.edge_lattice), built once per module and shared by the cases that only read them; a
crop rebuilds its map from the shared device cloud.  Every case asserts that the region it exists for is populated.

Measured wall time of the cases on the MI355X (pytest --durations=0; the whole module: 228 cases in 25 s).  The first case of a
group also pays what the group shares, and is named where that matters:
  cast                 28 cases  <= 0.04 s each (the very first 1.7 s: the library, the small map and its cost flood)
  clear, count-only     7 cases  <= 0.03 s (the first 0.24 s);  clear at 524 289 rays  0.04 s
  query                10 cases  <= 0.12 s
  raster               12 cases  <= 0.05 s
  scan scoring         16 cases  <= 0.14 s;  score derivatives  10 cases  <= 0.15 s
  crop                 85 cases  <= 0.07 s; the first case on each million-row lattice 0.42 s and 0.31 s (its points, drawn and uploaded)
  frontiers            44 cases  < 0.01 s; the first case on each million-row lattice 3.6 s and 4.0 s: frontier_ref's restatement of
                                 that map (a Python loop over rows), computed once and shared by the lattice's four cases
  coarsen               2 cases  1.4 s (1025 rows) and 2.3 s (725 x 724: the oracle's map of 4.7 M points at the doubled lengths)
  merge                 2 cases  0.02 s and 6.2 s (725 x 724: the oracle solves 524 900 eigenproblems; the device's share is milliseconds)
  clear by rows         1 case   0.31 s;  map-to-map scoring  2 cases  0.14 s and 0.29 s
  surface patches       8 cases  <= 0.02 s; the first case on each million-row lattice 0.87 s and 0.83 s: patch_ref.patches_fast's
                                 restatement of that map, computed once and shared by the lattice's four cases (three calls each)"""
import numpy as np
import pytest

from tests import cast_ref as cf
from tests import clear_ref as cr
from tests import edge_shapes as es
from tests import frontier_ref as fr
from tests import parity
from tests import patch_ref as pr
from tests import query_ref as qr
from tests import raster_ref as rr
from tests import score_derivs_ref as dr
from tests import score_maps_ref as mr
from tests import score_ref as sr
from tests.test_gpu_crop import FIELDS, _assert_same, _filtered
from tests.test_gpu_frontiers import cfg as frontier_cfg
from tests.test_gpu_frontiers import raw as frontier_raw
from tests.test_gpu_frontiers import untouched
from tests.test_gpu_patches import check as patch_check
from tests.gpu_kit import debug_option, dev

pytestmark = pytest.mark.gpu

AUTO, ATOMIC, PARTITION = 0, 1, 2
CAP, BASE = es.CAP, es.BASE
P, ORIGIN = es.P, es.ORIGIN
GL, ZL = P["grid_len"], P["z_len"]
DEBUG_CLEAR_EXTENT = 5
GOAL, ROBOT = (5.25, 3.25, fr.Z_FLOOR), {"radius": 0.25}
_cache = {}


def _np(x):
    if isinstance(x, dict):
        return {k: _np(v) for k, v in x.items()}
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _build(cloud_dev, strategy=AUTO, P=P, origin=ORIGIN):
    import grid_ndt_amd as g
    m = g.TwoDmap(P["grid_len"], P["z_len"], strategy=strategy)
    m.setInterval(P["slope_interval"])
    m.setCloudFirst(origin)
    m.create2DMap("slope", cloud_dev)
    m.sync()
    return m


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def small():
    """the small map, built once and only read: dict(m, cells, cost) with the cost flood of GOAL on it"""
    def make():
        m = _build(dev(es.small_cloud()[1:]))
        cells = m.export()
        assert cells["num_nodes"] == 41 * 25 and ((cells["flags"] & 2) != 0).all()
        assert m.computeCost(GOAL, robot=ROBOT)["rc"] == 0
        cost = m.cost_export()
        assert (cost["state"] != 0).sum() > 500
        return dict(m=m, cells=cells, cost=cost)
    return cached("small", make)


def take(ref, n, keys):
    idx = np.arange(n) % BASE
    return {k: ref[k][idx] for k in keys}


# ---- batch edges on the small map -----------------------------------------------------------------------------------------------------

def _cast_ref(mode, per_ray):
    def make():
        sensor, origins, ends = es.cast_base()
        return cf.cast(small()["cells"], ORIGIN, GL, ZL, origins if per_ray else sensor, ends, mode=mode)
    return cached(("cast", mode, per_ray), make)


@pytest.mark.parametrize("per_ray", [False, True], ids=["shared_origin", "origin_per_ray"])
@pytest.mark.parametrize("mode", [cf.VOXEL, cf.NDT], ids=["voxel", "ndt"])
@pytest.mark.parametrize("n", es.CAST_COUNTS)
def test_cast_batch_edges(n, mode, per_ray):
    m = small()["m"]
    sensor, origins, ends = es.cast_base()
    ref = _cast_ref(mode, per_ray)
    want = take(ref, n, ("row", "range", "d2"))
    mult = es.multiplicity(n)
    st_want = {"rays": int(mult[ref["status"] != cf.SKIPPED].sum()), "skipped": int(mult[ref["status"] == cf.SKIPPED].sum()),
               "hits": int(mult[ref["status"] == cf.HIT].sum())}
    assert st_want["rays"] + st_want["skipped"] == n
    if n > CAP:                                                     # the second trip answers: a hit among the rays >= 524 288
        assert (want["row"][CAP:] != cf.NO_ROW).any()
    if n >= CAP + 65:
        assert {cf.HIT, cf.MISS, cf.SKIPPED} <= set(ref["status"][es.tail_items(n)].tolist())
    o = dev(es.cyclic(origins, n)) if per_ray else sensor
    e = dev(es.cyclic(ends, n))
    out, st = m.cast_rays(o, e, mode={cf.VOXEL: "voxel", cf.NDT: "ndt"}[mode], stats=True)
    cf.assert_same(_np(out), want, (n, mode, per_ray, "stats"))
    assert st == st_want
    cf.assert_same(_np(m.cast_rays(o, e, mode={cf.VOXEL: "voxel", cf.NDT: "ndt"}[mode])), want, (n, mode, per_ray, "no stats"))


@pytest.mark.parametrize("n", es.CAST_COUNTS)
def test_clear_count_only_batch_edges(n):
    s = small()
    sensor, pts = es.clear_base()
    want, rays, skipped = es.clear_words(s["cells"], sensor, pts, n)
    if n > CAP:                                                     # the second trip's own rays pass rows and protect rows
        tail, _, _ = cr.passes(s["cells"], ORIGIN, GL, ZL, sensor, pts[es.tail_items(n)])
        assert ((tail & cr.PROTECTED) != 0).any() and ((tail & ~cr.PROTECTED) > 0).any()
    st, got = s["m"].clear_rays(sensor, dev(es.cyclic(pts, n)), count_only=True, passes=True)
    got = got.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want), (n, np.flatnonzero(got != want)[:8])
    assert (st["rays"], st["skipped"], st["cleared"]) == (rays, skipped, 0)
    assert st["protected_rows"] == int(((want & cr.PROTECTED) != 0).sum()) > 0


def test_clear_at_524289_rays_drops_the_rows_of_the_summed_words():
    """min_passes = 3 on a map held in the node table: the cleared rows are clear_ref.cleared_rows of the summed words, and the export
    afterwards is the export before it without them (one node a column: the columns and slopes left are the rows left)"""
    n, min_passes = CAP + 1, 3
    sensor, pts = es.clear_base()
    m = _build(dev(es.small_cloud()[1:]), ATOMIC)
    before = m.export()
    words, rays, skipped = es.clear_words(before, sensor, pts, n)
    drop = cr.cleared_rows(words, min_passes)
    assert 0 < drop.sum() < len(drop) and (((words & cr.PROTECTED) != 0) & ((words & ~cr.PROTECTED) >= min_passes)).any()
    st, _ = m.clear_rays(sensor, dev(es.cyclic(pts, n)), min_passes=min_passes, passes=True)
    assert (st["rays"], st["skipped"], st["cleared"]) == (rays, skipped, int(drop.sum()))
    want = {k: before[k][~drop] for k in FIELDS}
    want.update(num_nodes=int((~drop).sum()), num_columns=int((~drop).sum()), num_slopes=int((~drop).sum()))
    _assert_same(m.export(), want)


@pytest.mark.parametrize("what", ["nearest_slope", "node_cost"])
@pytest.mark.parametrize("n,ilp", [(CAP, 1), (CAP + 1, 1), (CAP, 4), (CAP + 1, 4), (es.QUERY_ILP4_COUNT, 4)])
def test_query_batch_edges(n, ilp, what):
    import grid_ndt_amd as g
    s = small()
    m, cells, cost = s["m"], s["cells"], s["cost"]
    base = es.query_base()
    if what == "nearest_slope":
        rows = cached("q_ns", lambda: qr.nearest_slope_rows(cells, base, ORIGIN, GL, ZL))
    else:
        rows = cached("q_node", lambda: qr.node_rows(cells, base, ORIGIN, GL, ZL))
    idx = np.arange(n) % BASE
    want = rows[idx]
    assert (want[-65:] >= 0).any() and (want[-65:] == qr.NO_ROW).any()      # the last wave's items: with a row and without
    if n > ilp * CAP:
        assert (want[ilp * CAP:] >= 0).any()
    t = dev(es.cyclic(base, n))
    g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_QUERY_ILP, ilp)
    try:
        if what == "nearest_slope":
            got = m.query(t, "nearest_slope").cpu().numpy().astype(np.int64)
            assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        else:
            got, h, st = (x.cpu().numpy() for x in m.query(t, "node", cost=True))
            got = got.astype(np.int64)
            assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
            hit = want >= 0
            h_want = np.where(hit, cost["h"][np.maximum(want, 0)], qr.FLT_MAX).astype(np.float32)
            st_want = np.where(hit, cost["state"][np.maximum(want, 0)], 0)
            assert np.array_equal(h.view(np.uint32), h_want.view(np.uint32)) and np.array_equal(st.astype(np.int64), st_want.astype(np.int64))
            assert (h_want[hit] < qr.FLT_MAX).any() and (st_want != 0).any()
    finally:
        g.TwoDmap.set_debug_option(g.TwoDmap.DEBUG_QUERY_ILP, 1)


# 1024 x 512 pixels: exactly one trip, the map in the middle.  725 x 724 = 524 900 pixels: 612 in the second trip, the last 612 of the
# last image row — which is the map's last line of columns (sy = 25), the map's columns sx = 1 .. 41 among its last 42 pixels.
RASTER_BOXES = {"1024x512": (-500, 524, -240, 272), "725x724": (-683, 42, -699, 25)}
RASTER_LAYERS = ("row", "z", "rough", "nodes", "h", "state")


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("mode", ["lowest", "highest", "nearest_z"])
@pytest.mark.parametrize("name", sorted(RASTER_BOXES))
def test_raster_boxes_around_one_trip(name, mode, host):
    from grid_ndt_amd.map2d import raster_shape
    s = small()
    box = RASTER_BOXES[name]
    w, h = raster_shape(box)
    assert f"{w}x{h}" == name and (w * h == CAP if name == "1024x512" else w * h == CAP + 612)
    z_ref = fr.Z_FLOOR + 0.5
    want = rr.raster(s["cells"], box, mode, z_ref, h_bits=s["cost"]["h"].view(np.uint32), state=s["cost"]["state"])
    flat = want["row"].reshape(-1)
    assert (flat >= 0).sum() == 41 * 25
    if w * h > CAP:                                                 # pixels of the second trip on the map and off it
        assert (flat[CAP:] >= 0).sum() == 41 and (flat[CAP:] < 0).sum() == 612 - 41
    got = s["m"].raster(box, mode, z_ref, layers=RASTER_LAYERS, host=host)
    for k in RASTER_LAYERS:
        assert rr.same(_np(got[k]), want[k]), (name, mode, host, k)
    off = flat < 0                                                  # the documented sentinels off the map
    assert (np.asarray(_np(got["z"])).reshape(-1)[off].view(np.uint32) == rr.QNAN_BITS).all()
    assert (np.asarray(_np(got["h"])).reshape(-1)[off] == rr.FLT_MAX).all() and (np.asarray(_np(got["state"])).reshape(-1)[off] == 0).all()
    assert (np.asarray(_np(got["nodes"])).reshape(-1)[off] == 0).all()


def _score_ref(nbh):
    def make():
        s = small()
        return sr.score(s["cells"], ORIGIN, GL, ZL, es.scan_base(), es.scan_poses(), nbh, per_point=2)
    return cached(("score", nbh), make)


@pytest.mark.parametrize("nbh", [1, 7])
@pytest.mark.parametrize("n", es.SCORE_COUNTS)
def test_scan_scoring_tile_and_reduce_edges(n, nbh):
    """per-point rows exact, per-point d2 within 1 ulp of fp32, counts exact, score and d2_sum at score_ref.RTOL = 1e-9 against the
    multiplicity-weighted fsum of the base terms: every term is non-negative, so the device's n additions stay within n 2^-53 =
    1.2e-10 of it at 2^20 points"""
    m = small()["m"]
    ref = _score_ref(nbh)
    mult = es.multiplicity(n)
    want = es.stack_poses([es.weighted_score(per, mult) for per in ref["poses_out"]])
    assert (want["terms"] > 0).all() and want["matched"][0] <= n
    if nbh == 7 and n > 16:
        assert want["terms"][0] > want["matched"][0]
    last = ref["poses_out"][2]
    if n % es.EDGES["kScoreTile"] == 1:                             # the one point of the last tile has a term
        assert last["row"][(n - 1) % BASE] != sr.NO_ROW and ref["poses_out"][0]["row"][(n - 1) % BASE] != sr.NO_ROW
    got = _np(m.score_poses(dev(es.cyclic(es.scan_base(), n)), es.scan_poses(), neighbourhood=nbh, per_point=2))
    sr.assert_pose_sums(got, want, what=(n, nbh))
    sr.assert_per_point(got["d2"], got["row"], take(last, n, ("row", "d2")), what=(n, nbh))


def _derivs_ref(nbh):
    def make():
        s = small()
        return dr.derivs(s["cells"], ORIGIN, GL, ZL, es.scan_base(), es.scan_poses(), nbh)
    return cached(("derivs", nbh), make)


@pytest.mark.parametrize("nbh", [1, 7])
@pytest.mark.parametrize("n", [256, 257, es.EDGES["derivs_reduce_points"], es.EDGES["derivs_reduce_points"] + 1, es.EDGES["score_reduce_points"] + 1])
def test_score_derivs_tile_and_reduce_edges(n, nbh):
    """test_gpu_score_derivs.py's rule (score_derivs_ref.assert_derivs) on the multiplicity-weighted sums of the base points' values"""
    m = small()["m"]
    mult = es.multiplicity(n)
    sums = [es.weighted_score(per, mult) for per in _score_ref(nbh)["poses_out"]]
    want = es.stack_poses([dict(s, **es.weighted_derivs(per, mult)) for s, per in zip(sums, _derivs_ref(nbh)["poses_out"])])
    assert (want["terms"] > 0).all() and (np.abs(want["H"]).max((1, 2)) > 0).all()
    if n % es.EDGES["kScoreTile"] == 1:
        assert _score_ref(nbh)["poses_out"][0]["row"][(n - 1) % BASE] != sr.NO_ROW
    got = _np(m.score_derivs(dev(es.cyclic(es.scan_base(), n)), es.scan_poses(), neighbourhood=nbh))
    dr.assert_derivs(got, want, what=(n, nbh))
    assert np.array_equal(got["H"], got["H"].transpose(0, 2, 1))


# ---- row-count edges on lattices --------------------------------------------------------------------------------------------------------

def lattice(n):
    """edge_lattice(n), uploaded once: dict(dev: the points behind the origin on the device, ix, iy: the cells)"""
    def make():
        pts, (ix, iy) = es.edge_lattice(n)
        assert len(ix) == n and len(pts) == 1 + 9 * n
        return dict(dev=dev(pts[1:]), ix=ix, iy=iy)
    return cached(("lattice", n), make)


def _crop_boxes(cells):
    x1, y1 = int(cells["sx"].max()), int(cells["sy"].max())
    first = (int(cells["sx"][0]),) * 2 + (int(cells["sy"][0]),) * 2
    last = (int(cells["sx"][-1]),) * 2 + (int(cells["sy"][-1]),) * 2
    return {"all": (1, x1, 1, y1), "none": (x1 + 10, x1 + 20, 1, y1), "last_row": last, "first_row": first,
            "half_lines": (1, x1, 1, max(1, y1 // 2))}      # the first half of every line of cells: a count and an offset in every tile


CROP_CASES = [(n, PARTITION) for n in es.CROP_ROWS] + [(n, ATOMIC) for n in es.CROP_ROWS if n >= 1023]


@pytest.mark.parametrize("box", ["all", "none", "last_row", "first_row", "half_lines"])
@pytest.mark.parametrize("n,strategy", CROP_CASES, ids=[f"{n}-{'rows' if s == PARTITION else 'table'}" for n, s in CROP_CASES])
def test_crop_row_count_edges(n, strategy, box):
    """export = filtered export, bit for bit, with the three counts; a NEAREST_SLOPE query of every cell's centre names the row of its
    cell in the cropped map, and no row where the cell left"""
    L = lattice(n)
    m = _build(L["dev"], strategy)
    mine = m.export()
    assert mine["num_nodes"] == n and np.array_equal(mine["sx"], L["ix"] + 1) and np.array_equal(mine["sy"], L["iy"] + 1)
    b = _crop_boxes(mine)[box]
    want = _filtered(mine, b, "keep_inside")
    kept = (mine["sx"] >= b[0]) & (mine["sx"] <= b[1]) & (mine["sy"] >= b[2]) & (mine["sy"] <= b[3])
    assert want["num_nodes"] == {"all": n, "none": 0, "last_row": 1, "first_row": 1}.get(box, want["num_nodes"])
    if box == "half_lines" and n >= 1023:                          # tiles that keep some rows and drop some (at 1024 x 1024: every tile)
        tiles = np.add.reduceat(kept.astype(np.int64), np.arange(0, n, es.EDGES["kCropTile"]))
        partial = (tiles > 0) & (tiles < es.EDGES["kCropTile"])
        assert partial[:-1].all() if n == 1 << 20 else partial.any()
    if n > es.EDGES["scan_carry_rows"]:                            # the row behind the scan's first chunk: kept, or dropped, by this box
        behind = kept[es.EDGES["scan_carry_rows"]:]
        assert behind.all() if box in ("all", "last_row", "half_lines") else not behind.any()
    m.crop_box(b, "keep_inside")
    got = m.export()
    _assert_same(got, want)
    centres = es.cell_centres(mine["sx"], mine["sy"])
    rows = m.query(dev(centres), "nearest_slope").cpu().numpy().astype(np.int64)
    expect = np.where(kept, np.cumsum(kept) - 1, qr.NO_ROW)
    assert np.array_equal(rows, expect), np.flatnonzero(rows != expect)[:8]


def _lattice_map(n):
    """edge_lattice(n) built once and only read: dict(m, cells)"""
    def make():
        m = _build(lattice(n)["dev"])
        cells = m.export()
        assert cells["num_nodes"] == n
        return dict(m=m, cells=cells)
    return cached(("lattice map", n), make)


def _frontier_map(n):
    def make():
        L = _lattice_map(n)
        return dict(L, ref=fr.Map(L["cells"]).frontiers(**frontier_cfg()))
    return cached(("frontier", n), make)


@pytest.mark.parametrize("long_list", [False, True], ids=["cut_list", "whole_list"])
@pytest.mark.parametrize("min_size", [1, 5])
@pytest.mark.parametrize("n", list(es.CROP_ROWS))
def test_frontier_row_count_edges(n, min_size, long_list):
    """candidates = slopes (no flood): labels, the four counts and every record field equal frontier_ref; min_size 5 drops the holes'
    clusters of four and the last row's cluster of one; a list shorter than the count is cut and nothing behind it is written"""
    f = _frontier_map(n)
    ref = f["ref"]
    recs, counts = fr.listed(ref, min_size)
    front = ref["label"] != fr.NO_ROW
    assert front[-1] and ref["label"][-1] == n - 1                 # the last row: a cluster of its own, its root in the last tile
    if n >= 1023:
        tiles = np.add.reduceat(front.astype(np.int64), np.arange(0, n, es.EDGES["kCropTile"]))
        assert (tiles > 0).all() if n == 1 << 20 else (tiles > 0).mean() > 0.5
        assert (ref["clusters"]["size"] == 4).sum() >= 1 and (min_size == 1 or 0 < len(recs) < len(ref["clusters"]))
    if n > CAP:
        assert front[CAP:].sum() > 100 and (ref["clusters"]["label"] >= CAP).sum() > 10
    cap = len(recs) + 7 if long_list else len(recs) // 2
    rc, got = frontier_raw(f["m"], frontier_cfg(), min_size=min_size, cap=cap)
    assert rc == 0
    assert np.array_equal(got["counts"], counts), (got["counts"], counts)
    assert np.array_equal(got["label"], ref["label"]), np.flatnonzero(got["label"] != ref["label"])[:8]
    want = recs[:cap]
    assert fr.same_records(got["clusters"], want), fr.diff_records(got["clusters"], want)
    assert untouched(got["buf"], len(want))


def _patch_map(n):
    """the lattice's map with its rows and patch_ref.patches_fast's answer for the whole map, computed once for the lattice's cases"""
    def make():
        L = _lattice_map(n)
        rows = pr.Rows(L["cells"])
        return dict(L, rows=rows, ref=pr.patches_fast(rows, pr.rule()))
    return cached(("patches", n), make)


def _hole_line_box(n):
    """a box one line of cells wide along the lattice's last line with holes, from its first cell to between its second and third
    hole: the holes cut the floor inside it into three patches, whose rows lie in the map's last third"""
    W, H = es.CROP_ROWS[n]
    holes = es.pitch_holes(W, H, 37 if W > 41 else 5, 41 if H > 41 else 5)
    ix = max(h[0] for h in holes)
    iy = sorted(h[1] for h in holes if h[0] == ix)
    return (ix + 1, ix + 1, 1, (iy[1] + iy[2]) // 2 + 1)


@pytest.mark.parametrize("call", ["whole", "min_size_2", "cap_1", "box"])
@pytest.mark.parametrize("n", [es.EDGES["scan_carry_rows"], es.EDGES["scan_carry_rows"] + 1])
def test_patch_row_count_edges(n, call):
    """surface patches on the million-row lattices: the floor and the last row's cell on its own are two patches, labelled 0 and
    n - 1 — mark, link and flatten in their second trip (row 524 288 on), k_patch_rank at tile 1024 on 1 048 577 rows, the scan's
    second chunk; the reductions in their ninth trip.  test_gpu_patches.check against patch_ref.patches_fast (thin: centroid and
    normal asserted, var printed): both entry points with the moment pass's LDS stage, the device's without it"""
    f = _patch_map(n)
    whole = f["ref"]
    tile = es.EDGES["kCropTile"]
    assert n > CAP and n > 8 * es.PATCH_TRIP - 1 and whole["patches"]["label"].tolist() == [0, n - 1] and whole["patches"]["nodes"].tolist() == [n - 1, 1]
    assert (whole["label"][CAP:] == 0).sum() > CAP - 2000                                  # rows of the second trip join the floor
    if n > es.EDGES["scan_carry_rows"]:
        assert int(whole["patches"]["label"][-1]) // tile >= es.EDGES["kCropScanT"]         # the last root: tile 1024, the scan's second chunk
    R = pr.rule()
    kw, ref, counts = dict(cap=5), whole, (2, n, 2, 0)
    if call == "min_size_2":
        kw, counts = dict(cap=5, min_size=2), (1, n, 2, 0)
    elif call == "cap_1":
        kw = dict(cap=1)
    elif call == "box":
        box = _hole_line_box(n)
        ref = pr.patches_fast(f["rows"], R, box)
        kw, counts = dict(cap=5, box=box), (3, ref["rows"], 3, 0)
        assert len(ref["patches"]) == 3 and ref["rows"] > 50 and ref["patches"]["label"].min() > 2 * n // 3
    for lds, host in ((1, False), (1, True), (0, False)):
        with debug_option("DEBUG_PATCH_LDS", lds, 1):
            got, _ = patch_check(f["m"], None, R, planes="thin", ref=ref, host=host, what=("patches", n, call, lds, host), **kw)
        assert tuple(got["counts"]) == counts and len(got["patches"]) == min(counts[0], kw["cap"])
        if call != "box":
            assert int(got["patches"]["nodes"][0]) == n - 1 and int(got["patches"]["points"][0]) == 9 * (n - 1)


def _plain(W, H):
    """the W x H floor without holes, built ATOMIC (the map lives in the node table): dict(m, cloud, cells)"""
    def make():
        cloud = es.lattice_points(W, H)
        m = _build(dev(cloud[1:]), ATOMIC)
        cells = m.export()
        assert cells["num_nodes"] == W * H
        return dict(m=m, cloud=cloud, cells=cells)
    return cached(("plain", W, H), make)


PLAIN = {"725x724": (725, 724), "1025": (25, 41)}         # 524 900 nodes: 612 behind the first trip; 1025: one node behind 16 whole waves


def _source_untouched(s):
    after = s["m"].export()
    for k in FIELDS:
        assert np.array_equal(np.ascontiguousarray(after[k]).view(np.uint32), np.ascontiguousarray(s["cells"][k]).view(np.uint32)), k


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_coarsen_past_one_trip_of_source_nodes(name):
    """test_gpu_coarsen's assertion: parity with the oracle's map of the same point stream at the doubled lengths"""
    s = _plain(*PLAIN[name])
    assert name != "725x724" or s["cells"]["num_nodes"] > CAP
    out = s["m"].coarsen(2, 2).export()
    assert 0 < out["num_nodes"] < s["cells"]["num_nodes"]
    parity.assert_parity(out, parity.ref_from_cloud(s["cloud"], dict(P, grid_len=2 * GL, z_len=2 * ZL)))
    _source_untouched(s)


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_merge_past_one_trip_of_source_nodes(name):
    """test_gpu_merge's assertion: the merge under the identity into an empty handle of the source's geometry has parity with the
    oracle's map of the source's point stream (the oracle solves 524 900 eigenproblems for the larger map: most of this case's time)"""
    import grid_ndt_amd as g
    s = _plain(*PLAIN[name])
    src, cloud = s["m"], s["cloud"]
    assert name != "725x724" or s["cells"]["num_nodes"] > CAP
    d = g.TwoDmap(GL, ZL, strategy=ATOMIC)
    d.setInterval(P["slope_interval"])
    d.setCloudFirst(cloud[0])
    st = d.merge_from(src)
    n = s["cells"]["num_nodes"]
    assert (st["source_nodes"], st["merged_nodes"], st["merged_points"], st["new_nodes"]) == (n, n, len(cloud) - 1, n)
    parity.assert_parity(d.export(), parity.ref_from_cloud(cloud, P))
    _source_untouched(s)


def test_clear_by_rows_past_one_trip_of_rows():
    """a few thousand rays along the last line of a 524 900-row map held in the node table: the per-row passes (k_clear_extent on, then
    off) and the clear itself (k_clear_kill) against clear_ref, with cleared rows behind row 524 288"""
    import grid_ndt_amd as g
    W, H = PLAIN["725x724"]
    cloud = es.lattice_points(W, H)
    m = _build(dev(cloud[1:]), ATOMIC)
    before = m.export()
    rng = np.random.default_rng(59)
    sensor = np.float32([(W - 1) * GL + 0.25, 200 * GL + 0.2, 0.2])
    k = 3000
    ends = np.stack([(W - 1 - rng.integers(0, 12, k)) * GL + 0.25, rng.integers(60, 700, k) * GL + 0.25, np.full(k, 0.2)], 1).astype(np.float32)
    words, rays, skipped = cr.passes(before, ORIGIN, GL, ZL, sensor, ends)
    drop = cr.cleared_rows(words, 2)
    assert drop[CAP:].sum() > 50 and (~drop[CAP:]).sum() > 50 and drop[:CAP].sum() > 50
    try:
        for ext in (1, 0):
            g.TwoDmap.set_debug_option(DEBUG_CLEAR_EXTENT, ext)
            st, got = m.clear_rays(sensor, dev(ends), count_only=True, passes=True)
            got = got.cpu().numpy().view(np.uint32)
            assert np.array_equal(got, words), (ext, np.flatnonzero(got != words)[:8])
            assert (st["rays"], st["skipped"], st["cleared"]) == (rays, skipped, 0)
        g.TwoDmap.set_debug_option(DEBUG_CLEAR_EXTENT, 1)
        st, _ = m.clear_rays(sensor, dev(ends), min_passes=2, passes=True)
    finally:
        g.TwoDmap.set_debug_option(DEBUG_CLEAR_EXTENT, 0)
    assert st["cleared"] == int(drop.sum())
    want = {f: before[f][~drop] for f in FIELDS}
    want.update(num_nodes=int((~drop).sum()), num_columns=int((~drop).sum()), num_slopes=int((~drop).sum()))
    _assert_same(m.export(), want)


@pytest.mark.parametrize("name", ["1025", "725x724"])
def test_map_to_map_scoring_of_a_lattice_against_itself(name):
    """every node has 9 points, so every source row counts; the identity and one small pose; test_gpu_score_maps.py's rule: counts
    and rows exact, sums at score_ref.RTOL, per-node d2 within 1 ulp of fp32 (and g, H entry-wise on the 1025-row map)"""
    s = _plain(*PLAIN[name])
    m, cells = s["m"], s["cells"]
    poses = es.scan_poses()[[0, 1]]
    poses[1, 0, 3], poses[1, 1, 3] = 0.03, -0.02
    want = mr.score(cells, ORIGIN, GL, ZL, cells, poses, 1, per_node=1)
    assert want["terms"][0] == cells["num_nodes"] and want["terms"][1] > cells["num_nodes"] // 2
    got = _np(m.score_map(m, poses, neighbourhood=1, per_node=1))
    mr.assert_pose_sums(got, want, what=name)
    mr.assert_per_node(got["d2"], got["row"], want["poses_out"][1], what=name)
    if name == "1025":
        for nbh in (1, 7):
            wd = mr.derivs(cells, ORIGIN, GL, ZL, cells, poses, nbh)
            mr.assert_derivs(_np(m.score_map_derivs(m, poses, neighbourhood=nbh)), wd, what=(name, nbh))
