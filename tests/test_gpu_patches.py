"""GPU tier: surface patches (gndt_patches_device / gndt_patches, TwoDmap.patches / patch_planes / patch_rows).  Every map is built on
the device; every label, count and integer field is compared for equality with the restatement (tests/patch_ref.py) on the rows the
handle's own export() returns.  The hand scene on three build paths through both entry points, one-patch planes at the wave and tile
edges, a spiral corridor of one long chain, a checkerboard of two tilts, two storeys with a stair, a box that cuts a patch in two,
scratch reuse, and every refused argument.

Plane fields (centroid, normal, var, kind's orientation bits) are compared with the restatement — never with a second run — on the
patches whose C has its two larger eigenvalues at least 100 x the least, in the scenes drawn for it (the hand scene, the storeys, the
checkerboard, the U): 1e-10 m absolute on centroid, 1e-10 on every component of the oriented normal, 1e-10 x value on var, the
footprints' bound.  Measured on the MI355X over this tier (PLANES_MEASURED below): 0 on centroid, 5.0e-16 on normal, 3.2e-12 x value
on var (the storeys' stair), so the bound stays as it is.  The flat lattices of the row-count edges and the
spiral are thinner than a thousandth of their extent (a ripple of 2 mm over 16 m and more): var holds no ten digits there whoever sums
it (tests/patch_ref.py planes_agree), so they assert centroid and normal and print var's deviation."""
import ctypes as C

import numpy as np
import pytest

from tests import edge_shapes as es
from tests import frontier_ref as fr
from tests import patch_ref as pr
from tests.gpu_kit import Padded, PaddedCall, build, dev, tails_untouched, to_np

pytestmark = pytest.mark.gpu

# the worst deviations of the compared patches over this tier on the MI355X (pytest -s prints every scene's): centroid, normal, var rel
PLANES_MEASURED = dict(centroid=0.0, normal=5.0e-16, var_rel=3.2e-12)        # inside 1e-10: the footprints' bound stays
# the same over tests/test_gpu_patch_edges.py, the patch cases of test_gpu_count_edges.py and test_gpu_scratch_reuse.py: the stripes
# (every patch well posed and compared) 0, 3.4e-16 and 6.9e-16; the thin floors, where var is printed only, 6.4e-13 x value on the two
# floors of 266 305 rows and 2.5e-12 on the million-row lattices
PLANES_MEASURED_EDGES = dict(centroid=0.0, normal=3.4e-16, var_rel=6.9e-16, var_rel_thin=2.5e-12)
ERR_INVALID = 1
ATOMIC, PARTITION, TILE = 1, 2, 5
WORD_FILL = 0x5A5A5A5A
PAD = 3                      # sentinel records on either side of the list
WORDS = 32                   # 4-byte words of a gndt_patch
FIELDS = ("sx", "sy", "sz", "count", "first_idx", "mean", "cov", "rough", "normal", "flags")
TILE_ROWS = es.EDGES["kCropTile"]
_scenes = {}


def params(R, min_size=1, reserved=(0, 0, 0, 0)):
    from grid_ndt_amd._lib import PatchParams
    return PatchParams(int(R["candidates"]), int(R["connectivity"]), float(R["cos_min"]), float(R["max_offset"]), float(R["max_var"]),
                       float(R["cos_level"]), float(R["sin_level"]), int(min_size), (C.c_uint32 * 4)(*reserved))


def raw(m, R, box=None, min_size=1, cap=None, labels=True, stream=None, host=False, reserved=(0, 0, 0, 0), counts=True, patches=True):
    """The C entry points.  cap None: as many records as the map has rows.  -> (rc, dict(label, patches [min(counts[0], cap)], counts,
    tails: what lay behind the label rows, the list's written records and the counts))"""
    from grid_ndt_amd._lib import CropBox
    n = int(m.sync()[0])
    cap = n if cap is None else cap
    prm = params(R, min_size, reserved)
    buf, lab, cnt = Padded(cap, words=WORDS, front=PAD, back=PAD), Padded(max(n, 1), back=4), Padded(4, back=4)
    rc = PaddedCall(host, stream)(m._L.gndt_patches, m._L.gndt_patches_device, m._h, None if box is None else C.byref(CropBox(*box)),
                                  C.byref(prm), lab if labels else None, buf if cap and patches else None, cap, cnt if counts else None)
    k = min(int(cnt.body[0]), cap) if rc == 0 else 0
    body = buf.a[PAD * WORDS:]
    return rc, dict(label=lab.body[:n], patches=body[:k * WORDS].view(pr.RECORD), counts=cnt.body,
                    front=buf.a[:PAD * WORDS], tails=dict(label=lab.tail, patches=body[k * WORDS:], counts=cnt.tail))


def check(m, ref_map, R, box=None, min_size=1, what="", planes=None, ref=None, **kw):
    """one call against the restatement -> (the call's answer, the restatement).  planes: "all" compares the plane fields under the
    issue's bounds, "thin" centroid and normal only (var printed), None nothing.  ref: the restatement's answer for (R, box) where the
    caller has it already — Map.patches' or patch_ref.patches_fast's (ref_map may then be None); it is left as it was"""
    rc, got = raw(m, R, box=box, min_size=min_size, **kw)
    assert rc == 0, (what, m._L.gndt_last_error(m._h))
    ref = ref_map.patches(R, box) if ref is None else dict(ref)
    recs, counts = pr.listed(ref, min_size)
    assert np.array_equal(got["counts"], counts), (what, got["counts"], counts)
    if kw.get("labels", True):
        assert np.array_equal(got["label"], ref["label"]), what
    cap = kw.get("cap")
    want = recs if cap is None else recs[:cap]
    assert pr.same_integers(got["patches"], want), (what, pr.diff_integers(got["patches"], want))
    assert tails_untouched(got) and (got["front"] == WORD_FILL).all(), what
    if planes == "all":
        ref["compared"] = pr.planes_agree(ref_map, R, ref, got["patches"], want, what)
    elif planes == "thin":
        dc, dn, dv = pr.plane_deviation(got["patches"], want)
        print(f"patch planes {what} (thin): centroid {dc:.3e} m, normal {dn:.3e}, var rel {dv:.3e} (not asserted)")
        assert dc <= pr.PLANE_ABS and dn <= pr.PLANE_ABS, (what, dc, dn)
        ref["deviation"] = (dc, dn, dv)
    return got, ref


def drawn(name, make, P=pr.P, strategy=0):
    """a map drawn from a cloud -> (m, ref_map, export)"""
    key = (name, strategy)
    if key not in _scenes:
        m = build(make(), P, strategy)
        cells = m.export()
        _scenes[key] = (m, pr.Map(cells), cells)
    return _scenes[key]


def hand(strategy=0):
    return drawn("hand", lambda: pr.hand_scene()[0], pr.P_HAND, strategy)


# ---- the hand scene ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strategy", [ATOMIC, PARTITION, TILE], ids=["atomic", "partition", "tile"])
def test_the_hand_scene_on_three_build_paths_through_both_entry_points(strategy):
    m, ref_map, cells = hand(strategy)
    groups = pr.hand_scene()[1]
    want = pr.hand_labels(ref_map, groups)
    R = pr.rule()
    for host in (False, True):
        got, ref = check(m, ref_map, R, host=host, planes="all", what=("hand", strategy, host))
        assert np.array_equal(got["label"], want) and tuple(got["counts"]) == (4, 135, 4, 0) and ref["compared"] == 4
        assert sorted(got["patches"]["nodes"].tolist()) == [9, 32, 32, 62]
        assert sorted((got["patches"]["kind"] & 7).tolist()) == [pr.HORIZONTAL, pr.HORIZONTAL, pr.VERTICAL, pr.INCLINED]
        check(m, ref_map, R, host=host, labels=False, planes="all", what=("hand, no labels", strategy, host))
        for conn in (1, 2, 0):
            check(m, ref_map, pr.rule(pr.SLOPES, conn), host=host, planes="all", what=("hand", strategy, host, conn))
        # counts only: nothing else is written
        rc, only = raw(m, R, cap=0, labels=False, host=host)
        assert rc == 0 and np.array_equal(only["counts"], got["counts"]) and tails_untouched(only) and (only["front"] == WORD_FILL).all()


def test_the_map_is_the_same_bits_afterwards_and_repeat_calls_on_two_streams_agree():
    import torch
    m, ref_map, cells = hand()
    R = pr.rule()
    first, _ = check(m, ref_map, R, what="first")
    s = torch.cuda.Stream()
    for stream in (None, s, None, s):
        rc, got = raw(m, R, stream=stream)
        assert rc == 0 and got["label"].tobytes() == first["label"].tobytes() and np.array_equal(got["counts"], first["counts"])
        assert pr.same_integers(got["patches"], first["patches"])
    after = m.export()
    for k in FIELDS:
        assert np.asarray(after[k]).tobytes() == np.asarray(cells[k]).tobytes(), k


# ---- one-patch planes at the wave and tile edges -----------------------------------------------------------------------------------

PLANES = {63: (8, 8), 64: (8, 8), 65: (9, 8), TILE_ROWS - 1: (32, 32), TILE_ROWS: (32, 32), TILE_ROWS + 1: (33, 32), 2 * TILE_ROWS + 1: (65, 32)}


@pytest.mark.parametrize("n", sorted(PLANES))
def test_one_patch_planes_at_the_wave_and_tile_edges(n):
    W, H = PLANES[n]
    assert TILE_ROWS == 1024 and W * H >= n
    m, ref_map, cells = drawn(("plane", n), lambda: es.lattice_points(W, H, count=n), fr.P)
    assert ref_map.n == n
    for host in (False, True):
        got, _ = check(m, ref_map, pr.rule(), host=host, planes="thin", what=("plane", n, host))
        rec = got["patches"]
        assert tuple(got["counts"]) == (1, n, 1, 0) and (got["label"] == 0).all()
        assert int(rec["nodes"][0]) == n and int(rec["points"][0]) == 9 * n and int(rec["kind"][0]) == pr.HORIZONTAL | pr.SLOPES_ONLY
    got, _ = check(m, ref_map, pr.rule(pr.SLOPES, 1), what=("plane, 6", n))
    assert tuple(got["counts"]) == (1, n, 1, 0)


@pytest.mark.parametrize("seed", [None, 1, 2])
def test_a_spiral_corridor_is_one_patch_labelled_by_its_smallest_row(seed):
    cells_in = pr.spiral()
    assert len(cells_in) == 3961
    m, ref_map, cells = drawn(("spiral", seed), lambda: pr.flat_cloud(cells_in, seed))
    for conn in (1, 3):
        got, _ = check(m, ref_map, pr.rule(pr.NODES, conn), planes="thin", what=("spiral", seed, conn))
        assert tuple(got["counts"]) == (1, 3961, 1, 0) and (got["label"] == 0).all() and int(got["patches"]["nodes"][0]) == 3961
    # a box across the spiral leaves a stack of separate arms
    got, ref = check(m, ref_map, pr.rule(), box=(-100, 100, 1, 3), what=("spiral, strip", seed))
    assert got["counts"][0] > 40


# ---- the checkerboard ---------------------------------------------------------------------------------------------------------------

def test_a_checkerboard_of_two_tilts_is_every_node_under_6_and_two_patches_under_26():
    m, ref_map, cells = drawn("checker", pr.checkerboard)
    n = pr.CHECKER_N ** 2
    for host in (False, True):
        got, _ = check(m, ref_map, pr.rule(pr.NODES, 1), host=host, what=("checker 6", host))
        assert tuple(got["counts"]) == (n, n, n, 0) and np.array_equal(got["label"], np.arange(n, dtype=np.uint32))
        got, ref = check(m, ref_map, pr.rule(pr.NODES, 3), host=host, planes="all", what=("checker 26", host))
        assert tuple(got["counts"]) == (2, n, 2, 0) and got["patches"]["nodes"].tolist() == [n // 2, n // 2] and ref["compared"] == 2
        got18, _ = check(m, ref_map, pr.rule(pr.NODES, 2), host=host, what=("checker 18", host))
        assert got18["label"].tobytes() == got["label"].tobytes()
        # a list shorter than the patches: counts[0] says so, the records beyond stay as they were
        for cap in (1, 50, n - 1, n, n + 5):
            got, _ = check(m, ref_map, pr.rule(pr.NODES, 1), host=host, cap=cap, what=("checker cap", cap, host))
            assert int(got["counts"][0]) == n and len(got["patches"]) == min(cap, n)
        # min_size filters the list, not the labels
        got, _ = check(m, ref_map, pr.rule(pr.NODES, 1), host=host, min_size=2, what=("checker min_size", host))
        assert tuple(got["counts"]) == (0, n, n, 0) and np.array_equal(got["label"], np.arange(n, dtype=np.uint32))
        got, _ = check(m, ref_map, pr.rule(pr.NODES, 3), host=host, min_size=n // 2 + 1, what=("checker min_size 26", host))
        assert tuple(got["counts"]) == (0, n, 2, 0) and len(set(got["label"].tolist())) == 2


# ---- two storeys, a box, reuse -------------------------------------------------------------------------------------------------------

def test_two_storeys_stay_two_patches_and_the_stair_is_inclined():
    m, ref_map, cells = drawn("storeys", lambda: pr.two_storeys()[0], pr.P_HAND)
    nodes = pr.two_storeys()[1]
    for host in (False, True):
        got, ref = check(m, ref_map, pr.rule(), host=host, planes="all", what=("storeys", host))
        rec = got["patches"]
        assert tuple(got["counts"]) == (3, 112, 3, 0) and ref["compared"] == 3
        by = {int(r["nodes"]): r for r in rec}
        assert sorted(by) == sorted(nodes.values())
        assert int(by[64]["kind"]) & 7 == pr.HORIZONTAL and int(by[32]["kind"]) & 7 == pr.HORIZONTAL and int(by[16]["kind"]) & 7 == pr.INCLINED
        assert abs(by[32]["centroid"][2] - by[64]["centroid"][2] - 1.0) < 1e-3 and abs(by[16]["normal"][0] / by[16]["normal"][2] + 0.5) < 1e-3
        assert (int(by[16]["sz_min"]), int(by[16]["sz_max"])) == (1, 5)


def test_a_box_cuts_a_patch_in_two():
    m, ref_map, cells = drawn("u", pr.u_shape)
    for host in (False, True):
        got, _ = check(m, ref_map, pr.rule(), host=host, planes="all", what=("u", host))
        assert tuple(got["counts"]) == (1, 15, 1, 0)
        got, _ = check(m, ref_map, pr.rule(), box=(1, 5, 3, 6), host=host, planes="all", what=("u, boxed", host))
        assert tuple(got["counts"]) == (2, 8, 2, 0) and got["patches"]["nodes"].tolist() == [4, 4]
        got, _ = check(m, ref_map, pr.rule(), box=(20, 30, 1, 5), host=host, what=("u, outside", host))
        assert tuple(got["counts"]) == (0, 0, 0, 0) and (got["label"] == pr.NO_ROW).all()


def test_a_call_after_a_larger_call_and_as_the_first_builder_of_the_column_index():
    # a fresh handle: the patch call is the first consumer, so it builds the map's column index
    m = build(pr.checkerboard(), pr.P)
    ref_map = pr.Map(m.export())
    n = pr.CHECKER_N ** 2
    got, _ = check(m, ref_map, pr.rule(pr.NODES, 1), what="first consumer")           # n patches listed: the larger call
    assert int(got["counts"][0]) == n
    got, _ = check(m, ref_map, pr.rule(pr.NODES, 3), cap=2, planes="all", what="after a larger call")
    assert tuple(got["counts"]) == (2, n, 2, 0)
    got, _ = check(m, ref_map, pr.rule(pr.NODES, 3), cap=1, host=True, what="after a larger call, host")
    assert len(got["patches"]) == 1
    # the index it built serves the frontiers
    f = m.frontiers("slopes")
    assert int(to_np(f["counts"])[1]) == 4 * pr.CHECKER_N - 4
    # a larger map on the same handle, then the small one again
    big = build(pr.flat_cloud(pr.spiral(), 1), pr.P)
    check(big, pr.Map(big.export()), pr.rule(), what="big")
    small = pr.checkerboard(4)
    big.create2DMap("slope", dev(small[1:, :3]))
    big.sync()
    check(big, pr.Map(big.export()), pr.rule(pr.NODES, 3), planes="all", what="small after big")


# ---- the Python interface -------------------------------------------------------------------------------------------------------------

def test_python_patches_planes_and_rows():
    m, ref_map, cells = hand()
    ref = ref_map.patches(pr.rule())
    recs, counts = pr.listed(ref)
    for host in (False, True):
        p = m.patches(labels=True, host=host)
        assert np.array_equal(to_np(p["counts"]).view(np.uint32), counts)
        for k in pr.INTEGER_FIELDS:
            assert np.array_equal(to_np(p[k]).astype(np.int64), recs[k].astype(np.int64)), (k, host)
        assert np.array_equal(to_np(p["labels"]).view(np.uint32), ref["label"])
        assert np.abs(to_np(p["centroid"]) - recs["centroid"]).max() <= pr.PLANE_ABS and np.abs(to_np(p["normal"]) - recs["normal"]).max() <= pr.PLANE_ABS
        cen, nrm, off = (to_np(v) for v in m.patch_planes(p))
        assert cen.shape == (4, 3) and nrm.shape == (4, 3) and np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-12)
        assert np.allclose(off, (recs["centroid"] * recs["normal"]).sum(1), atol=1e-9)
        for which in range(4):
            rows = to_np(m.patch_rows(p, p["labels"], which))
            assert np.array_equal(rows, np.flatnonzero(ref["label"] == recs["label"][which]))
        # a list with room to spare: the device list keeps its capacity (nodes 0 behind the patches), the host list is cut
        p = m.patches(max_patches=6, host=host)
        assert to_np(p["nodes"]).tolist() == recs["nodes"].tolist() + ([] if host else [0, 0])
        assert np.isnan(to_np(m.patch_planes(p)[0])[4:]).all()
        p = m.patches("slopes", 6, max_angle_deg=30.0, min_size=10, max_patches=1, host=host)
        want, wc = pr.listed(ref_map.patches(pr.rule(pr.SLOPES, 1, max_angle_deg=30.0)), 10)
        assert np.array_equal(to_np(p["counts"]).view(np.uint32), wc) and to_np(p["label"]).tolist() == want["label"][:1].tolist()
    with pytest.raises(ValueError):
        m.patches(connectivity=8)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_refused_arguments():
    import torch
    import grid_ndt_amd as g
    m, ref_map, cells = hand()
    ok = pr.rule()
    nan, inf = float("nan"), float("inf")
    for host in (False, True):
        assert raw(m, ok, host=host)[0] == 0
        for bad in (dict(candidates=2), dict(candidates=-1), dict(connectivity=4), dict(cos_min=1.5), dict(cos_min=-0.1), dict(cos_min=nan),
                    dict(max_offset=-1.0), dict(max_offset=inf), dict(max_var=-1e-3), dict(max_var=nan), dict(cos_level=1.01),
                    dict(cos_level=-0.5), dict(sin_level=-0.1), dict(sin_level=inf)):
            assert raw(m, dict(ok, **bad), host=host)[0] == ERR_INVALID, bad
        assert raw(m, dict(ok, cos_min=1.0, max_offset=0.0, max_var=0.0, sin_level=2.0), host=host)[0] == 0
        for word in range(4):
            assert raw(m, ok, reserved=tuple(int(i == word) for i in range(4)), host=host)[0] == ERR_INVALID
        for box in ((3, 2, 1, 1), (1, 1, 3, 2), (-65536, 1, 1, 2), (1, 2, 1, 65536), (0, 0, 1, 2), (1, 2, 0, 0)):
            assert raw(m, ok, box=box, host=host)[0] == ERR_INVALID, box
        whole, full = raw(m, ok, host=host), raw(m, ok, box=(-65535, 65535, -65535, 65535), host=host)
        assert full[0] == 0 and pr.same_integers(full[1]["patches"], whole[1]["patches"]) and np.array_equal(full[1]["counts"], whole[1]["counts"])
        assert raw(m, ok, patches=False, host=host)[0] == ERR_INVALID            # NULL patches with patch_cap > 0
        assert raw(m, ok, counts=False, host=host)[0] == ERR_INVALID             # NULL counts
    prm = params(ok)
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    recs = torch.zeros(3 * WORDS, dtype=torch.int32, device="cuda")
    lab = torch.zeros(ref_map.n + 1, dtype=torch.int32, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    call = m._L.gndt_patches_device
    assert call(m._h, None, C.byref(prm), None, p(recs), 0, p(cnt), None) == ERR_INVALID      # patches with patch_cap 0
    assert call(m._h, None, C.byref(prm), None, p(recs, 4), 1, p(cnt), None) == ERR_INVALID   # not aligned as the struct is
    assert call(m._h, None, C.byref(prm), p(lab, 2), None, 0, p(cnt), None) == ERR_INVALID    # labels not aligned
    assert call(m._h, None, C.byref(prm), None, None, 0, p(cnt, 1), None) == ERR_INVALID      # counts not aligned
    assert call(m._h, None, C.byref(prm), None, p(recs, 8), 1, p(cnt), None) == 0             # 8 bytes are enough
    torch.cuda.synchronize()
    assert int(recs[2]) == 0 and int(recs[3]) == 62 and int(recs[0]) == 0 and int(recs[2 + WORDS]) == 0     # the floor, and only it
    assert call(m._h, None, None, None, None, 0, p(cnt), None) == ERR_INVALID                 # NULL params
    assert call(None, None, C.byref(prm), None, None, 0, p(cnt), None) == ERR_INVALID
    assert m._L.gndt_patches(None, None, C.byref(prm), None, None, 0, None) == ERR_INVALID
    # no finished build
    e = g.TwoDmap(0.5, 0.25)
    e.setCloudFirst((0.0, 0.0, 0.0))
    with pytest.raises(g.GndtError) as err:
        e.patches()
    assert err.value.code == ERR_INVALID
    # a capturing stream: refused, and the capture goes on
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    with g.graph_capture(graph, stream=s):
        rc = call(m._h, None, C.byref(prm), None, None, 0, p(cnt), C.c_void_p(s.cuda_stream))
        x.add_(1.0)
    assert rc == ERR_INVALID
    graph.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    check(m, ref_map, ok, planes="all", what="after the refused capture")
