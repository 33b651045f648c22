"""GPU tier: the clearance field (gndt_clearance_device / gndt_clearance, TwoDmap.clearance / clearance_vectors).  Every map is built on
the device; hops, nearest, sides and counts are compared for equality with the restatement (tests/clearance_ref.py) on the handle's own
export, every scene once with the one-workgroup kernel allowed and once without it.  Hand-drawn maps whose answer is known beforehand —
a corridor between plateaus, two storeys, a low ceiling, a column taller than the step mask — then the site and the bridge, repeat
calls and streams, crop and update, sentinel-filled outputs, the Python interface and every refused argument; and lattices with exact
row counts at the kernels' edges — the slots and the limit of the one-workgroup kernel, max_hops at 1, at 1024 and around the field's
depth, the second trip of the grid-stride loops.  No tolerance anywhere:
the one step that is not IEEE arithmetic is the gates' acosf, and every compared scene keeps its angle decisions more than 1e-3 degrees
from the threshold."""
import ctypes as C

import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import clearance_ref as cr
from tests import frontier_ref as fr
from tests.gpu_kit import Padded, PaddedCall, build, debug_option, dev, robot_arg, to_np
from tests.gpu_kit import tails_untouched as untouched

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
ATOMIC = 1
SENTINEL = 0x5A5A5A5A
PAD = 5                      # sentinel entries behind num_nodes
MARGIN = 1e-3
LDS_ROWS = 9216              # the largest map the one-workgroup kernel takes
FIELDS = ("sx", "sy", "sz", "count", "first_idx", "mean", "cov", "rough", "normal", "flags")
_scenes = {}


def one_workgroup(on):
    """gndt_debug_set_option(GNDT_DEBUG_CLEARANCE_ONE_WORKGROUP, .) for a block; the default comes back whatever happens in it"""
    return debug_option("DEBUG_CLEARANCE_ONE_WORKGROUP", 1 if on else 0, 1)


def raw(m, mask=cr.BLOCKED, max_hops=32, robot=None, outs=("hops", "nearest", "sides"), stream=None, host=False, reserved=(0,) * 6, counts=True):
    """The C entry points, every output num_nodes + PAD entries of sentinel.  -> (rc, dict(hops, nearest, sides: the outputs asked for,
    cut to num_nodes; counts; tails: what lies behind num_nodes))"""
    from grid_ndt_amd._lib import ClearanceParams
    n = int(m.sync()[0])
    prm = ClearanceParams(mask, max_hops, (C.c_uint32 * 6)(*reserved))
    buf = {k: Padded(n, np.uint8, back=PAD, fill=SENTINEL & 0xFF) if k == "sides" else Padded(n, back=PAD, fill=SENTINEL) for k in outs}
    cnt = Padded(4, fill=SENTINEL)
    rc = PaddedCall(host, stream)(m._L.gndt_clearance, m._L.gndt_clearance_device, m._h, robot_arg(robot, cr.ROBOT), C.byref(prm),
                                  *[buf.get(k) for k in ("hops", "nearest", "sides")], cnt if counts else None)
    out = {k: p.body for k, p in buf.items()}
    out.update(counts=cnt.a, tails={k: p.tail for k, p in buf.items()})
    return rc, out


def check(m, f, mask=cr.BLOCKED, max_hops=32, what="", **kw):
    """one call against the restatement -> the call's answer"""
    rc, got = raw(m, mask, max_hops, **kw)
    assert rc == 0, (what, m._L.gndt_last_error(m._h))
    want = f.clearance(mask, max_hops)
    assert np.array_equal(got["counts"], want["counts"]), (what, got["counts"], want["counts"])
    for k in kw.get("outs", ("hops", "nearest", "sides")):
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(got[k] != want[k])[:8])
    assert untouched(got), what
    return got


def both_paths(m, f, mask=cr.BLOCKED, max_hops=32, what="", **kw):
    """the call with the one-workgroup kernel allowed and without it: the restatement's answer and the same bytes"""
    with one_workgroup(True):
        a = check(m, f, mask, max_hops, what=(what, "one workgroup"), **kw)
    with one_workgroup(False):
        b = check(m, f, mask, max_hops, what=(what, "a launch a hop"), **kw)
    for k in a:
        if k != "tails":
            assert a[k].tobytes() == b[k].tobytes(), (what, k)
    return a


def drawn(name, make, P=fr.P, robot=None):
    """a map drawn from a cloud -> (m, restatement, export)"""
    if name not in _scenes:
        m = build(make(), P)
        cells = m.export()
        f = cr.Field(cells, robot)
        assert f.angle_margin_deg > MARGIN, (name, f.angle_margin_deg)
        _scenes[name] = (m, f, cells)
    return _scenes[name]


def site(name):
    if name == "site":
        return drawn("site", scenes.drivable_site, scenes.COST_PARAMS)
    return drawn("bridge", scenes.bridge_ground, scenes.BRIDGE_PARAMS)


# ---- maps whose answer is known beforehand -------------------------------------------------------------------------------------------

def test_corridor_between_plateaus():
    m, f, cells = drawn("corridor", cr.corridor_cloud, cr.CORRIDOR_P)
    assert cells["num_nodes"] == 156 and ((cells["flags"] & 2) != 0).all()
    got = both_paths(m, f, what="corridor")
    assert tuple(got["counts"]) == (48, 156, 3, 0)
    across = {-3: 2, -2: 1, -1: 0, 1: 0, 2: 1, 3: 2, 4: 3, 5: 2, 6: 1, 7: 0, 8: 0, 9: 1, 10: 2}       # signed indices step over 0
    assert all(int(got["hops"][r]) == across[int(cells["sx"][r])] for r in range(156))
    # the nearest barrier of a row is in its own line across the corridor, and a source's is itself
    near = got["nearest"]
    assert (cells["sy"][near] == cells["sy"]).all() and (near[got["hops"] == 0] == np.flatnonzero(got["hops"] == 0)).all()
    # blocked: the side towards the step, on both sides of it; nothing is open inside the map
    mid = (cells["sy"] > 1) & (cells["sy"] < 12)
    assert (got["sides"][mid & (cells["sx"] == 1)] == 0b1000).all() and (got["sides"][mid & (cells["sx"] == -1)] == 0b0100).all()
    assert (got["sides"][mid & (cells["sx"] == 4)] == 0).all()
    got = both_paths(m, f, max_hops=2, what="corridor, 2 hops")
    line = cells["sx"] == 4
    assert (got["hops"][line] == cr.BEYOND).all() and (got["nearest"][line] == cr.NO_ROW).all() and (got["hops"][~line] <= 2).all()
    assert tuple(got["counts"]) == (48, 144, 2, 0)
    got = both_paths(m, f, cr.BLOCKED | cr.OPEN, what="corridor, open")
    ring = (cells["sx"] == -3) | (cells["sx"] == 10) | (cells["sy"] == 1) | (cells["sy"] == 12)
    assert (got["hops"][ring] == 0).all() and int(got["counts"][0]) == 48 + int(ring.sum()) - 8


def _storeys():
    up = fr.Z_FLOOR + 4 * fr.ZL
    ground = [(ix, iy, fr.Z_FLOOR) for ix in range(-5, 5) for iy in range(-5, 5)]
    deck = [(ix, iy, up) for ix in range(-3, 3) for iy in range(-3, 3)]
    return fr.cells_cloud(ground + deck, 12)


def test_two_storeys_do_not_see_each_other():
    m, f, cells = drawn("storeys", _storeys)
    top = cells["sz"] == cells["sz"].max()
    assert int(top.sum()) == 36 and cells["num_nodes"] == 136
    lin = lambda s: np.where(s > 0, s - 1, s)
    x, y = lin(cells["sx"]), lin(cells["sy"])
    # BLOCKED: the deck's edge stands a metre over the ground beside it; the ground has no barrier at all
    got = both_paths(m, f, what="storeys")
    deck_edge = np.minimum(np.minimum(x + 3, 2 - x), np.minimum(y + 3, 2 - y))
    assert np.array_equal(got["hops"][top], deck_edge[top]) and (got["hops"][~top] == cr.BEYOND).all()
    assert tuple(got["counts"]) == (20, 36, 2, 0) and top[got["nearest"][top]].all()
    # with the map's edge as a barrier the ground has its own field, under the deck as beside it
    got = both_paths(m, f, cr.BLOCKED | cr.OPEN, what="storeys, open")
    ground_edge = np.minimum(np.minimum(x + 5, 4 - x), np.minimum(y + 5, 4 - y))
    assert np.array_equal(got["hops"][~top], ground_edge[~top]) and np.array_equal(got["hops"][top], deck_edge[top])
    assert top[got["nearest"][top]].all() and not top[got["nearest"][~top]].any()


def _ceiling():
    floor = [(ix, iy, 0.26) for ix in range(-4, 4) for iy in range(-3, 3)]
    lid = [(ix, iy, 0.56) for ix in range(-4, -1) for iy in range(-3, 3)]           # 0.3 m above the floor's first three lines
    return fr.cells_cloud(floor + lid, 5)


def test_a_low_ceiling_is_a_barrier_for_the_robot_it_is_too_low_for():
    m, f, cells = drawn("ceiling", _ceiling)
    low = cells["sz"] == cells["sz"].min()
    under = low & (cells["sx"] <= -2)
    assert int(low.sum()) == 48 and int(under.sum()) == 18 and int((~low).sum()) == 18
    got = both_paths(m, f, cr.OVERHEAD, what="ceiling")                             # radius 0.25: 0.3 m is within 2 r and beyond the reach
    assert np.array_equal(got["hops"] == 0, under) and int(got["counts"][0]) == 18
    lin_x = np.where(cells["sx"] > 0, cells["sx"] - 1, cells["sx"])
    assert np.array_equal(got["hops"][low & ~under], (lin_x + 2)[low & ~under]) and (got["hops"][~low] == cr.BEYOND).all()
    slim = cr.Field(cells, dict(radius=0.1))                                          # 0.3 m is not within 0.2 m
    got = both_paths(m, slim, cr.OVERHEAD, robot=dict(radius=0.1), what="ceiling, slim")
    assert tuple(got["counts"]) == (0, 0, 0, 0) and (got["hops"] == cr.BEYOND).all()


def test_a_step_through_a_pit_column_taller_than_the_step_mask():
    """The pit's points come first in the cloud and the cell's floor points last, so the exporter (a column's rows in order of first
    sight) puts the floor's slope behind the pit's nodes: the arrangement the test takes, asserted below."""
    from tests.test_clearance_host import shim
    m, f, cells = drawn("pit", cr.pit_cloud)
    step_rows = shim().clshim_step_rows()
    col = np.flatnonzero((cells["sx"] == 4) & (cells["sy"] == 1))
    slopes = np.flatnonzero((cells["flags"] & 2) != 0)
    assert len(col) == 37 > step_rows and (np.diff(col) == 1).all()
    assert [int(r - col[0]) for r in slopes if r in col] == [36] and 36 >= step_rows
    got = both_paths(m, f, what="pit")
    by_x = {int(cells["sx"][r]): int(got["hops"][r]) for r in slopes}
    assert by_x == {1: 6, 2: 5, 3: 4, 4: 3, 5: 2, 6: 1, 7: 0, 8: 0} and tuple(got["counts"]) == (2, 8, 6, 0)
    assert (got["sides"][np.setdiff1d(col, slopes)] == 0xFF).all() and (got["hops"][np.setdiff1d(col, slopes)] == cr.BEYOND).all()
    got = both_paths(m, f, max_hops=3, what="pit, 3 hops")
    assert sorted(int(cells["sx"][r]) for r in slopes if got["hops"][r] == cr.BEYOND) == [1, 2, 3]


# ---- the site and the bridge -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["site", "bridge"])
def test_site_scenes_are_the_restatement(name):
    m, f, cells = site(name)
    if name == "site":
        assert cells["num_nodes"] > LDS_ROWS          # a launch a hop whatever the option says
    for mask in (cr.BLOCKED, cr.BLOCKED | cr.OPEN):
        got = both_paths(m, f, mask, what=(name, mask))
        assert got["counts"][0] > 50 and got["counts"][2] >= 3
    both_paths(m, f, cr.BLOCKED, max_hops=3, what=(name, "3 hops"))


# ---- kernel-edge shapes: lattices with exact row counts (tests/clearance_ref.LATTICES) ------------------------------------------------

def lattice(name):
    """a lattice map -> (m, restatement, export); its premises (tests/test_clearance_host.lattice_premises, which the CPU tier asserts
    on the oracle's build) asserted on the device's own rows when it is first drawn"""
    from tests.test_clearance_host import lattice_premises
    new = ("lattice", name) not in _scenes
    m, f, cells = drawn(("lattice", name), lambda: cr.lattice(name, fr.P))
    if new:
        lattice_premises(name, cells, f)
    return m, f, cells


@pytest.mark.parametrize("rows,max_hops", [(r, h) for r in (1023, 1024, 1025, 9216, 9217) for h in (64, 1)])
def test_lattices_at_the_slot_edges_and_the_limit_of_the_one_workgroup_kernel(rows, max_hops):
    """gndt_api_clearance.hip `wg = ... n <= kClrLdsRows`, and k_clearance_wg's `row = threadIdx.x + j * kClrWgThreads; if (row >= n)
    break` with its one-bit-a-slot `pending` and `fresh`: 1023 / 1024 / 1025 rows end a slot one thread short, exactly and one thread
    into the next; 9216 rows use all 144 KB of keys with the flag words right behind them; 9217 is the first map that takes a launch
    a hop whatever the option says (both_paths then runs that path twice)."""
    m, f, cells = lattice(rows)
    n = int(cells["num_nodes"])
    assert n == rows and (n < LDS_ROWS if rows < 9216 else n == LDS_ROWS if rows == 9216 else n > LDS_ROWS)
    for mask in (cr.BLOCKED, cr.BLOCKED | cr.OPEN):
        got = both_paths(m, f, mask, max_hops, what=(rows, mask, max_hops))
        want = f.clearance(mask, max_hops)
        assert (got["hops"] == 0).any() and got["counts"][2] == want["counts"][2] and got["counts"][2] >= (6 if max_hops == 64 else 1)
        if mask == cr.BLOCKED and max_hops == 64:
            assert ((got["hops"] > 32) & (got["hops"] != cr.BEYOND)).any()
        if max_hops == 1:
            assert (got["hops"] == cr.BEYOND).any() and (got["hops"] == 1).any()


def test_max_hops_of_one_the_limit_the_depth_one_less_and_an_odd_one_behind_it():
    """gndt_api_clearance.hip `k_clearance_finish(key[F.max_hops & 1], ...)` and the `max_hops + 1` flag words: with an odd max_hops
    behind the field's depth the rounds stop early and the answer is read from buffer 1, which the last working round has to have
    brought up to date (clearance_round_stores); max_hops = 1024 clears and walks 1025 of the 1032 flag words; max_hops = depth makes
    the last round the one that finds the last ring, depth - 1 leaves that ring out.  k_clearance_wg: `last`, its `fresh` copies."""
    m, f, cells = lattice(1025)
    full = f.clearance(cr.BLOCKED, 1024)
    depth = int(full["counts"][2])
    odd = (depth + 3) | 1
    assert 3 < depth < odd - 1 and odd & 1 and odd <= 1024           # (round depth + 1 finds nothing: round depth + 2 <= odd never works)
    for max_hops in (1, 1024, odd, depth, depth - 1, odd):
        got = both_paths(m, f, cr.BLOCKED, max_hops, what=("max_hops", max_hops))
        assert got["counts"][2] == min(max_hops, depth) and got["counts"][0] == full["counts"][0]
        ring = full["hops"] == depth
        assert ring.any() and ((got["hops"][ring] == cr.BEYOND).all() if max_hops < depth else (got["hops"][ring] == depth).all())
        if max_hops >= depth:
            assert np.array_equal(got["hops"], full["hops"]) and np.array_equal(got["nearest"], full["nearest"])
    for on in (True, False):
        with one_workgroup(on):
            check(m, f, cr.BLOCKED, odd, host=True, what=("odd, host", on))


def test_the_second_trip_of_the_grid_stride_loops():
    """k_clearance_steps and k_clearance_round `for (t0 = blockIdx.x * blockDim.x; t0 < total; t0 += gsz)` with 2048 workgroups of 256
    threads (four lanes a row), k_clearance_finish `row += gsz` with 512 (one lane a row): on 131 769 rows all three go 697 rows into
    their second trip — ten workgroups of live quads, one with 228 live and 28 dead lanes around the quad exchange, the rest dead.
    Those rows hold finite and BEYOND answers (lattice_premises)."""
    m, f, cells = lattice(131769)
    n = int(cells["num_nodes"])
    assert 4 * n > 2048 * 256 and n > 512 * 256 and n > LDS_ROWS
    for host in (False, True):
        got = check(m, f, cr.BLOCKED, 64, host=host, what=("second trip", host))
        tail = got["hops"][512 * 256:]
        assert (tail == cr.BEYOND).any() and (tail != cr.BEYOND).any() and got["counts"][2] == 64


def test_repeat_calls_and_a_second_stream_give_the_same_bytes_and_change_nothing():
    import torch
    m, f, cells = site("bridge")
    goal = (9.5, 3.0, 1.0)
    assert m.computeCost(goal)["rc"] == 0
    cost = m.cost_export()
    first = check(m, f, what="first")
    s = torch.cuda.Stream()
    for on in (True, False):
        with one_workgroup(on):
            for stream in (None, s, None, s):
                rc, got = raw(m, stream=stream)
                assert rc == 0
                for k in ("hops", "nearest", "sides", "counts"):
                    assert got[k].tobytes() == first[k].tobytes(), (k, stream, on)
            # an answer of another shape in between (the scratch is reused)
            check(m, f, cr.OPEN, 2, what="between")
            rc, got = raw(m, host=True)
            assert rc == 0 and all(got[k].tobytes() == first[k].tobytes() for k in ("hops", "nearest", "sides", "counts"))
    after, cost_after = m.export(), m.cost_export()
    for k in FIELDS:
        assert np.asarray(after[k]).tobytes() == np.asarray(cells[k]).tobytes(), k
    assert cost_after["h"].tobytes() == cost["h"].tobytes() and cost_after["state"].tobytes() == cost["state"].tobytes()


def test_after_a_crop_and_after_an_update():
    cloud = scenes.drivable_site(200_000)
    m = build(cloud, scenes.COST_PARAMS, ATOMIC)

    def fresh(what):
        f = cr.Field(m.export())
        assert f.angle_margin_deg > MARGIN, what
        got = both_paths(m, f, cr.BLOCKED | cr.OPEN, what=what)
        assert got["counts"][0] > 0
        return got

    before = fresh("before")
    x0, x1 = int(m.export()["sx"].min()), int(m.export()["sx"].max())
    m.crop_box((x0 + 5, x1 - 5, -1000, 1000), "keep_inside")
    cropped = fresh("crop")
    assert len(cropped["hops"]) < len(before["hops"])
    m.change2DMap("slope", dev(cloud[1:1000, :3] + np.float32([0.0, 0.0, 0.02])))
    fresh("update")
    # the middle of the site: a map of thousands of rows that the one-workgroup kernel still holds, many hops deep
    xm, w = (x0 + x1) // 2, (x1 - x0) // 5
    m.crop_box((xm - w, xm + w, -1000, 1000), "keep_inside")
    assert 2000 < m.sync()[0] <= LDS_ROWS
    small = fresh("middle")
    assert small["counts"][2] >= 5
    # everything cropped away: four zero counts, nothing else written
    m.crop_box((x1 + 50, x1 + 60, 1, 2), "keep_inside")
    assert m.sync()[0] == 0
    for host in (False, True):
        rc, got = raw(m, host=host)
        assert rc == 0 and tuple(got["counts"]) == (0, 0, 0, 0) and untouched(got)
        cl = m.clearance(sides=True, host=host)
        assert all(len(cl[k]) == 0 for k in ("hops", "nearest", "sides")) and not to_np(cl["counts"]).any()


def test_outputs_are_optional_and_nothing_is_written_beyond_the_rows():
    m, f, cells = drawn("pit", cr.pit_cloud)
    full = check(m, f, cr.BLOCKED | cr.OPEN, what="all three")
    assert (full["sides"][(cells["flags"] & 2) == 0] == 0xFF).all() and ((cells["flags"] & 2) == 0).sum() == 36
    for on in (True, False):
        with one_workgroup(on):
            for host in (False, True):
                for outs in (("hops",), ("nearest",), ("sides",), ("hops", "sides"), ("nearest", "sides"), ("hops", "nearest")):
                    got = check(m, f, cr.BLOCKED | cr.OPEN, outs=outs, host=host, what=(outs, host, on))
                    assert set(got) == set(outs) | {"counts", "tails"}


# ---- the Python interface ----------------------------------------------------------------------------------------------------------

def test_python_defaults_host_and_streams():
    import torch
    m, f, cells = site("bridge")
    want = f.clearance(cr.BLOCKED, 32)
    s = torch.cuda.Stream()
    for kw in (dict(), dict(host=True), dict(stream=s)):
        cl = m.clearance(**kw)
        if "stream" in kw:
            s.synchronize()
        assert set(cl) == {"hops", "nearest", "counts"} and (isinstance(cl["hops"], np.ndarray) == bool(kw.get("host")))
        assert np.array_equal(to_np(cl["hops"]).view(np.uint32), want["hops"]) and np.array_equal(to_np(cl["nearest"]).view(np.uint32), want["nearest"])
        assert np.array_equal(to_np(cl["counts"]).view(np.uint32), want["counts"])
        assert (to_np(cl["hops"])[want["hops"] == cr.BEYOND] == m.CLEARANCE_BEYOND).all()
    for host in (False, True):
        cl = m.clearance(robot=dict(radius=0.25), max_hops=2, sources=("blocked", "open"), hops=False, nearest=False, sides=True, host=host)
        assert set(cl) == {"sides", "counts"} and np.array_equal(to_np(cl["sides"]), f.sides)
        assert np.array_equal(to_np(cl["counts"]).view(np.uint32), f.clearance(3, 2)["counts"])
        cl = m.clearance(sources="open", max_hops=5, host=host)
        assert np.array_equal(to_np(cl["hops"]).view(np.uint32), f.clearance(cr.OPEN, 5)["hops"])
        assert np.array_equal(to_np(m.clearance(sources=6, host=host)["hops"]).view(np.uint32), f.clearance(6, 32)["hops"])


def test_clearance_vectors_are_the_gather_and_subtraction_on_the_export():
    m, f, cells = site("bridge")
    mean = np.asarray(cells["mean"], np.float32)
    for host in (False, True):
        cl = m.clearance(host=host)
        vec = m.clearance_vectors(cl)
        assert (hasattr(vec, "cpu") != host) and tuple(vec.shape) == (cells["num_nodes"], 3)
        near = to_np(cl["nearest"]).astype(np.int64)
        none = near < 0
        assert none.any() and not none.all()
        want = mean[np.where(none, 0, near)] - mean
        got = to_np(vec)
        assert np.isnan(got[none]).all() and got[~none].tobytes() == want[~none].tobytes()
        assert (got[to_np(cl["hops"]) == 0] == 0).all()          # a source's barrier is where it stands


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_refused_arguments():
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd._lib import ClearanceParams
    m, f, cells = drawn("corridor", cr.corridor_cloud, cr.CORRIDOR_P)
    for host in (False, True):
        assert raw(m, host=host)[0] == 0
        for mask in (8, 9, 0x80000000, 0xFFFFFFFF):
            assert raw(m, mask, host=host)[0] == ERR_INVALID, mask
        assert raw(m, max_hops=1025, host=host)[0] == ERR_INVALID and raw(m, max_hops=0xFFFFFFFF, host=host)[0] == ERR_INVALID
        rc, got = raw(m, max_hops=1024, host=host)
        assert rc == 0 and np.array_equal(got["hops"], f.clearance(1, 1024)["hops"])
        for k in range(6):
            assert raw(m, reserved=tuple(int(j == k) for j in range(6)), host=host)[0] == ERR_INVALID, k
        assert raw(m, outs=(), host=host)[0] == ERR_INVALID                   # all three outputs NULL
        assert raw(m, counts=False, host=host)[0] == ERR_INVALID              # NULL counts
        # zeros are the defaults: BLOCKED, 32 hops
        rc, got = raw(m, 0, 0, host=host)
        want = f.clearance(cr.BLOCKED, 32)
        assert rc == 0 and np.array_equal(got["hops"], want["hops"]) and np.array_equal(got["counts"], want["counts"])
    prm = ClearanceParams(1, 4)
    n = int(cells["num_nodes"])
    buf = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int32, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    call = m._L.gndt_clearance_device
    assert call(m._h, None, C.byref(prm), p(buf, 2), None, None, p(cnt), None) == ERR_INVALID        # hops not aligned
    assert call(m._h, None, C.byref(prm), None, p(buf, 1), None, p(cnt), None) == ERR_INVALID        # nearest not aligned
    assert call(m._h, None, C.byref(prm), p(buf), None, None, p(cnt, 2), None) == ERR_INVALID        # counts not aligned
    assert call(m._h, None, C.byref(prm), None, None, p(buf, 1), p(cnt, 4), None) == 0               # bytes go anywhere
    assert call(m._h, None, None, p(buf), None, None, p(cnt), None) == ERR_INVALID                   # NULL params
    assert call(None, None, C.byref(prm), p(buf), None, None, p(cnt), None) == ERR_INVALID
    assert m._L.gndt_clearance(None, None, C.byref(prm), None, None, None, None) == ERR_INVALID
    torch.cuda.synchronize()
    # no finished build
    e = g.TwoDmap(0.5, 0.25)
    e.setCloudFirst((0.0, 0.0, 0.0))
    with pytest.raises(g.GndtError) as err:
        e.clearance()
    assert err.value.code == ERR_INVALID
    # a capturing stream: refused, and the capture goes on
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    x = torch.zeros(16, device="cuda")
    with g.graph_capture(graph, stream=s):
        rc = call(m._h, None, C.byref(prm), p(buf), None, None, p(cnt), C.c_void_p(s.cuda_stream))
        x.add_(1.0)
    assert rc == ERR_INVALID
    graph.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0
    both_paths(m, f, what="after the refused capture")
