"""CPU tier: the surface patches' second restatement, patch_ref.patches_fast (sorted keys, searchsorted, hooking and pointer jumping,
ufunc.at, one batched eigh), which the GPU tier needs at a hundred thousand and a million rows, where patch_ref.Map.patches (a dict
and a search, a Python loop over rows) takes minutes.

First against Map.patches on every scene the patch tests draw and on the 200 random lattices, under both candidate modes and
connectivity 1, 2, 3 and 0: labels, counts, every integer field, kind and the well-posed flags for equality — and centroid, normal and
var TO THE BIT: both add the members in ascending row (ufunc.at takes its indices one after the other), one term at a time from the
same float64 expressions, and the batched eigh is LAPACK's one call a matrix.  That held on every scene here; PLANE_ABS / VAR_REL
between the two restatements were never needed.

Then against the header's own row code (tests/patch_shim.cpp through test_patch_host.run) on the oracle's maps of the two scenes of
tests/test_gpu_patch_edges.py that no loop restatement reaches: two floors over three trips of the reductions (266 305 rows) and
stripes over the trip edge (134 400 rows) — every label, count and integer field for equality, planes by planes_agree: the header's
row logic is right at those counts before a GPU sees them."""
import numpy as np
import pytest

from tests import edge_shapes as es
from tests import patch_ref as pr
from tests.host_emulation import HostMap
from tests.test_patch_host import Lattice, run

RULES = [(cand, conn) for cand in (pr.NODES, pr.SLOPES) for conn in (1, 2, 3, 0)]


def same_as_the_loop(cells, R, box=None, what="", ref_map=None):
    """patches_fast against Map.patches -> the loop's answer"""
    ref_map = pr.Map(cells) if ref_map is None else ref_map
    slow = ref_map.patches(R, box)
    fast = pr.patches_fast(cells, R, box)
    assert np.array_equal(fast["label"], slow["label"]) and fast["label"].dtype == slow["label"].dtype, what
    assert fast["rows"] == slow["rows"] and np.array_equal(fast["cand"], slow["cand"]), what
    a, b = fast["patches"], slow["patches"]
    for ms in (1, 2):
        assert np.array_equal(pr.listed(fast, ms)[1], pr.listed(slow, ms)[1]), (what, ms)
    assert pr.same_integers(a, b), (what, pr.diff_integers(a, b))
    assert np.array_equal(a["kind"], b["kind"]), what
    for k in ("centroid", "normal", "var"):
        assert a[k].tobytes() == b[k].tobytes(), (what, k, float(np.abs(a[k] - b[k]).max()))
    posed = slow["posed"]
    assert not len(b) or posed[-1] == pr.well_posed(ref_map, R, slow, b[-1])
    keep, spread = pr.well_posed_fast(fast, a)
    assert np.array_equal(keep, np.array([p[0] for p in posed], bool)), what
    assert np.array_equal(spread, np.array([p[1] for p in posed], np.float64)), what
    return slow


SCENES = {
    "hand": (lambda: pr.hand_scene()[0], pr.P_HAND, (None,)),
    "storeys": (lambda: pr.two_storeys()[0], pr.P_HAND, (None,)),
    "checkerboard": (pr.checkerboard, pr.P, (None,)),
    "spiral": (lambda: pr.flat_cloud(pr.spiral()), pr.P, (None, (-100, 100, 1, 3))),
    "spiral, seed 1": (lambda: pr.flat_cloud(pr.spiral(), 1), pr.P, (None,)),
    "spiral, seed 2": (lambda: pr.flat_cloud(pr.spiral(), 2), pr.P, (None,)),
    "u": (pr.u_shape, pr.P, (None, (1, 5, 3, 6), (20, 30, 1, 5))),
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_drawn_scenes_give_the_loops_answer_to_the_bit(name):
    make, P, boxes = SCENES[name]
    m = HostMap(make(), P)
    ref_map = pr.Map(m.cells)
    patches = 0
    for cand, conn in RULES:
        for box in boxes:
            slow = same_as_the_loop(m.cells, pr.rule(cand, conn), box, (name, cand, conn, box), ref_map)
            patches += len(slow["patches"])
    assert patches > 0
    if name == "checkerboard":                      # every node under 6, the two colours under 18 and 26
        n = pr.CHECKER_N ** 2
        assert [len(pr.patches_fast(m.cells, pr.rule(pr.NODES, c))["patches"]) for c in (1, 2, 3)] == [n, 2, 2]
    if name.startswith("spiral"):                   # one chain of 3 961 rows in three row orders: the hooking's long path
        fast = pr.patches_fast(m.cells, pr.rule(pr.NODES, 1))
        assert len(fast["patches"]) == 1 and int(fast["patches"]["nodes"][0]) == 3961 and fast["rounds"] >= 1


def test_200_random_lattices_give_the_loops_answer_to_the_bit():
    rng = np.random.default_rng(20241021)
    some = refused = 0
    for k in range(200):
        g = Lattice(rng)
        ref_map = pr.Map(g.cells)
        for cand, conn in RULES:
            slow = same_as_the_loop(g.cells, pr.rule(cand, conn, max_offset=0.125, max_var=0.004), None, (k, cand, conn), ref_map)
            some += int((slow["patches"]["nodes"] >= 2).sum())
            refused += int((~slow["pairs"][2]).sum())
    assert some > 1000 and refused > 1000


def test_no_rows_and_no_candidates():
    cells = dict(num_nodes=0, **{k: np.zeros((0,) + s, t) for k, s, t in (("sx", (), np.int32), ("sy", (), np.int32), ("sz", (), np.int32),
                 ("flags", (), np.uint32), ("count", (), np.uint32), ("rough", (), np.float32), ("mean", (3,), np.float32),
                 ("normal", (3,), np.float32), ("cov", (6,), np.float32))})
    fast = pr.patches_fast(cells, pr.rule())
    assert len(fast["label"]) == 0 and len(fast["patches"]) == 0 and fast["rows"] == 0
    m = HostMap(pr.u_shape(), pr.P)
    same_as_the_loop(m.cells, pr.rule(), (20, 30, 1, 5), "outside")


# ---- the header's row code at the counts of the GPU tier's large scenes ---------------------------------------------------------------

LARGE = {"floors, 30 rows into the wave": lambda: es.floors_cells(es.FLOORS_A[0], es.FLOORS_N),
         "floors, 3 rows into the wave": lambda: es.floors_cells(es.FLOORS_A[1], es.FLOORS_N),
         "stripes over the trip edge": lambda: es.stripes_cells(*es.TRIP_STRIPES)}


@pytest.mark.parametrize("name", sorted(LARGE))
def test_the_shim_on_the_oracles_maps_of_the_large_scenes(name):
    """spread_slack: planes_agree's own allowance for the oracle's maps — a floor of 130 000 nodes is 2 mm thin over 250 m"""
    ix, iy = LARGE[name]()
    n = len(ix)
    m = HostMap(es.cells_points(ix, iy), es.P)
    assert m.n == n > es.PATCH_TRIP and np.array_equal(m.sx, ix + 1) and np.array_equal(m.sy, iy + 1)       # row r is cell r
    for R, box, min_size in ((pr.rule(), None, 1), (pr.rule(pr.SLOPES, 1), None, 1), (pr.rule(), (1, 200, 1, 100), 2)):
        ref = pr.patches_fast(m.cells, R, box)
        recs, counts = pr.listed(ref, min_size)
        cap = len(recs) + 3
        got = run(m, R, box, min_size, cap=cap)
        assert np.array_equal(got["counts"], counts), (name, got["counts"], counts)
        assert np.array_equal(got["label"], ref["label"]), name
        assert pr.same_integers(got["patches"], recs), (name, pr.diff_integers(got["patches"], recs))
        assert (got["tail"].view(np.uint32) == 0xA5A5A5A5).all()
        assert pr.planes_agree(None, R, ref, got["patches"], recs, name, spread_slack=True) == len(recs) > 0
        if box is None:
            if name.startswith("floors"):
                a = es.FLOORS_A[0] if "30" in name else es.FLOORS_A[1]
                assert tuple(counts) == (2, n, 2, 0) and recs["label"].tolist() == [0, a] and recs["nodes"].tolist() == [a, n - a]
            else:
                H, lines = es.TRIP_STRIPES
                assert tuple(counts) == (lines, n, lines, 0) and np.array_equal(recs["label"], np.arange(lines) * H) and (recs["nodes"] == H).all()
