"""CPU tier of the scripted handle lives (tests/stream_model.py).  A second, independent account of what a handle holds — the points in
its node table with their stream indices, moved by the operations as the library defines them (a crop by the columns of the points'
keys, a clear by the nodes tests/clear_ref.py kills on the handle's own export, a remove by the points handed in, a merge as the
source's table appended at the stream position) — is finalised at every checkpoint by the kernels' own arithmetic on the host
(tests/host_emulation.py: accumulate, finalize) and must pass parity.assert_parity, non-adversarial and with parity's tolerances as
they are, against the model's oracle map; first_idx is remapped by the model.  So the model's equivalences hold in the kernels'
arithmetic, and the reference alone stays inside parity's caps on these scenes.

Also: every script meets the conditions it is named for, from the model alone (node counts on the intended side of 900 and 1024, table
growths by the restated cap_for_nodes, crops that keep some and drop some, clears that kill some and not all, removes that kill), and
the comparison is sensitive: a model that forgets a crop, a remove or a merge fails the check."""
import numpy as np
import pytest

from tests import clear_ref as cr
from tests import host_emulation as he
from tests import parity
from tests import query_ref as qr
from tests import stream_model as sm

P, ORIGIN = sm.P, sm.ORIGIN


class HostHandle:
    def __init__(self):
        self.pts, self.idx, self.pos = np.zeros((0, 3), np.float32), np.zeros(0, np.int64), 0

    def add(self, pts, idx):
        self.pts = np.concatenate([self.pts, np.ascontiguousarray(pts[:, :3], np.float32)])
        self.idx = np.concatenate([self.idx, np.asarray(idx, np.int64)])

    def keep(self, mask):
        self.pts, self.idx = self.pts[mask], self.idx[mask]

    def export(self):
        if len(self.pts) == 0:
            return sm.empty_map()
        t = he.accumulate(self.pts, ORIGIN, P["grid_len"], P["z_len"], idx=self.idx)
        return he.finalize(*t, P["slope_interval"], P["demand"])


class HostBackend:
    """the operations on HostHandle; check: the handle's export against the model's oracle map"""

    def __init__(self):
        self.h, self.checks = {}, 0

    def new(self, h, **kw):
        self.h[h] = HostHandle()

    def build(self, h, cloud):
        self.h[h] = HostHandle()
        self.update(h, cloud)

    def update(self, h, pts):
        x = self.h[h]
        x.add(pts, x.pos + np.arange(len(pts)))
        x.pos += len(pts)

    def remove(self, h, pts):
        x = self.h[h]
        rec = lambda a: np.ascontiguousarray(a, np.float32).view([("p", np.void, 12)]).ravel()
        gone = np.isin(rec(x.pts), rec(pts))
        assert int(gone.sum()) == len(pts)              # every point handed in is in the table, once
        x.keep(~gone)

    def crop(self, h, box):
        x = self.h[h]
        if len(x.pts):
            sx, sy, _ = sm.point_keys(x.pts)
            x.keep(sm.inside(sx, sy, box))

    def clear(self, h, sensor, ends, count_only):
        x = self.h[h]
        cells = x.export()
        if count_only or cells["num_nodes"] == 0:
            return
        words, _, _ = cr.passes(cells, ORIGIN, P["grid_len"], P["z_len"], sensor, ends)
        drop = cr.cleared_rows(words, 1)
        x.keep(~np.isin(qr.pack(*sm.point_keys(x.pts)), qr.pack(cells["sx"], cells["sy"], cells["sz"])[drop]))

    def merge(self, h, src):
        x, s = self.h[h], self.h[src]
        x.add(s.pts, x.pos + s.idx)
        x.pos += s.pos

    def reset(self, h):
        self.h[h] = HostHandle()

    def accumulate(self, h, pts, base):
        x = self.h[h]
        x.add(pts, base + np.arange(len(pts)))
        x.pos = max(x.pos, base + len(pts))

    def finalize(self, h):
        pass

    def stats_to(self, h, dst):
        x, s = self.h[dst], self.h[h]
        x.add(s.pts, s.idx)
        x.pos = max(x.pos, int(s.idx.max()) + 1 if len(s.idx) else 0)

    def reserve(self, h, max_points, max_nodes):
        pass

    def deferred(self, h, on):
        pass

    def query(self, h, m):
        pass

    def refused(self, h, what, pts=None):
        pass

    def check(self, h, label, m):
        got, want = self.h[h].export(), m.expected()
        rep = parity.assert_parity(m.remap(got), want)
        self.checks += 1
        if want["num_nodes"]:
            # the NODE answers on the two exports name the same keys
            q = m.query_points()
            a, b = sm.query_rows(got, q), sm.query_rows(want, q)
            assert np.array_equal(a >= 0, b >= 0)
        return rep


@pytest.fixture(scope="module")
def logs():
    """every script once through the host backend: {name: log}; a checkpoint that fails parity fails here"""
    out = {}
    for name, make in sm.SCRIPTS.items():
        b = HostBackend()
        out[name] = sm.run(make(), b)
        assert b.checks == sum(1 for e in out[name] if e["kind"] == "check") >= 4, name
    return out


@pytest.mark.parametrize("name", list(sm.SCRIPTS))
def test_every_checkpoint_passes_parity_and_the_script_meets_its_conditions(logs, name):
    log = logs[name]
    for e in log:
        if e["kind"] == "check":
            x = e["expect"]
            assert e["nodes"] <= x.get("nodes_max", 1 << 30) and e["nodes"] >= x.get("nodes_min", 0), (name, e)
            assert e["alive"] <= 70_000, (name, e)
        elif e["kind"] == "crop":
            assert (e["kept"] == 0 and e["dropped"] > 0) if e["to_empty"] else (e["kept"] > 0 and e["dropped"] > 0), (name, e)
        elif e["kind"] == "clear" and "killed" in e:
            assert 0 < e["killed"] < e["nodes"], (name, e)
        elif e["kind"] == "remove":
            assert e["nodes_after"] < e["nodes_before"], (name, e)


def test_the_named_transitions(logs):
    labels = lambda name: {e["label"]: e for e in logs[name] if e["kind"] == "check"}
    # the map on both sides of do_finalize's small-map test and of the one-workgroup kernel's limit, in the order the names say
    s = labels("small_then_stream")
    assert s["second small build: one workgroup"]["nodes"] <= sm.SMALL_SEEN < sm.SMALL_KERNEL < s["one frame removed"]["nodes"]
    assert s["small again through n_dead"]["nodes"] == s["second small build: one workgroup"]["nodes"]
    t = [e for e in logs["small_seen_then_tails"] if e["kind"] == "check"]
    assert t[0]["nodes"] <= sm.SMALL_SEEN and all(e["nodes"] > sm.SMALL_KERNEL for e in t[1:]) and len(t) == 7
    # table growths by the restated rule: at least two in growth_and_reserve, one under un-emitted frames in deferred_crossings
    g = [e for e in logs["growth_and_reserve"] if e["kind"] == "update"]
    assert sum(bool(e.get("grows")) for e in g) >= 2, g
    d = [e for e in logs["deferred_crossings"] if e["kind"] == "update"]
    assert not d[0]["grows"] and not d[1]["grows"] and d[2]["grows"]
    # the stream position grows tenfold within a script: the order's word arrays grow in mid-stream
    for name in ("deferred_crossings", "growth_and_reserve"):
        u = [e["stream_pos"] for e in logs[name] if e["kind"] == "update"]
        assert u[-1] >= 10 * u[1] > 0, (name, u)
    # emptied twice, and the indices went on
    e = labels("to_empty_and_back")
    assert e["nothing left"]["nodes"] == 0 and e["empty through n_dead"]["nodes"] == 0 and e["and back"]["nodes"] > 0
    r = labels("rebuild_between")
    assert r["large then small on the table"]["nodes"] <= sm.SMALL_SEEN and r["partition build"]["alive"] >= 65_536


def test_the_table_sizing_restatement():
    assert [sm.cap_for_nodes(n) for n in (0, 1024, 1025, 4096, 4097)] == [2048, 2048, 4096, 8192, 16384]
    t = sm.TableSim()
    assert not t.update(37, 0) and t.cap == 2048 and t.bound == 37
    assert not t.update(500, 30) and t.bound == 537
    assert t.update(3000, 60) and t.cap == 8192 and t.bound == 3060           # the real count is fetched before the table moves
    assert not t.update(1000, 400) and t.bound == 4060
    assert not t.reserve(8000, 4000) and t.reserve(200000, 4000) and t.cap == 131072


@pytest.mark.parametrize("effect, name", [("crop", "small_seen_then_tails"), ("remove", "small_then_stream"), ("merge", "merge_and_stats")])
def test_a_model_that_forgets_an_effect_fails_the_check(effect, name):
    """a cropped column kept, a removed frame kept, a merged source missing: the host handle does the operation, the model does not"""
    script = sm.SCRIPTS[name]()
    first = next(i for i, op in enumerate(script) if op[0] == effect)
    cut = next(i for i in range(first, len(script)) if script[i][0] == "check") + 1
    sm.run(script[:first], HostBackend())                   # (up to the operation everything passes)
    with pytest.raises(AssertionError):
        sm.run(script[:cut], HostBackend(), forget=(effect,))
