"""GPU tier of the scripted handle lives (tests/stream_model.py): one test per script, through TwoDmap on device tensors.  A handle
that keeps its map in the node table carries host-side state from call to call (incr_ok, table_dirty, emit_pending, pending_words,
words_init, small_ok, small_used, table_nodes_seen, results_valid, stream_pos, nodes_bound, n_dead, result_serial) and do_finalize picks
one of four paths from it; the other GPU tests reach each entry point on a handle whose history is one or two calls long.  Here a
handle lives through a written-down sequence of update, remove, crop, clear, merge, rebuild, reset / accumulate / finalize, statistics
export and merge, reserve and the deferred-emit switch, and at every checkpoint

  * parity.assert_parity(export, the oracle's map of the model's alive points), first_idx remapped by the model: keys, order, counts,
    first-seen indices and labels exact, statistics to parity's own gates;
  * sync() returns the expected (nodes, columns, slopes);
  * a NODE query of 37 alive points, a few dead ones and a few that were never added returns exactly the row the export holds for the
    point's key and no row where it holds none: the column index follows result_serial through every kind of producer.

Refusals are checked by their code and by an export that is unchanged byte for byte.  No hipGraph capture here (tools/fuzz_graph.py and
the capture tests own that ground).  tests/test_stream_model_host.py proves the model on the CPU; tests/test_gpu_poisoned.py runs these
tests once more on memory that does not start out as zeros (group "stream").

Wall time per script on the MI355X (pytest --durations=0, call phase): small_then_stream 1.81 s (the first of the module: the
library's code is loaded here), small_seen_then_tails 0.25 s, deferred_crossings 0.09 s, growth_and_reserve 0.23 s, rebuild_between
0.16 s, to_empty_and_back 0.02 s, merge_and_stats 0.25 s; small_seen_each_tail 2.19 s and the reserve test at the end 1.94 s, each run
alone, the load of the library's code included; the module with its eight scripts 3.6 s."""
import numpy as np
import pytest

from tests import parity
from tests import stream_model as sm
from tests.gpu_kit import dev

pytestmark = pytest.mark.gpu

P, ORIGIN = sm.P, sm.ORIGIN
ERR_INVALID = 1
FIELDS = ("sx", "sy", "sz", "count", "first_idx", "mean", "cov", "rough", "normal", "flags")
PARTITION_FAMILY = (2, 3, 6, 7)          # TwoDmap.STRATEGY_NAMES: the builds that keep no node table


def _same_bytes(a, b):
    assert (a["num_nodes"], a["num_columns"], a["num_slopes"]) == (b["num_nodes"], b["num_columns"], b["num_slopes"])
    for k in FIELDS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), k


class GpuBackend:
    def __init__(self):
        self.m, self.checks = {}, 0

    def new(self, h, **kw):
        import grid_ndt_amd as g
        m = g.TwoDmap(P["grid_len"], P["z_len"], **kw)
        m.setInterval(P["slope_interval"])
        m.setCloudFirst(ORIGIN)
        self.m[h] = m

    def build(self, h, cloud):
        self.m[h].create2DMap("slope", dev(cloud))

    def update(self, h, pts):
        self.m[h].change2DMap("slope", dev(pts))

    def remove(self, h, pts):
        self.m[h].del2DMap("slope", dev(pts))

    def crop(self, h, box):
        self.m[h].crop_box(box, "keep_inside")

    def clear(self, h, sensor, ends, count_only):
        st = self.m[h].clear_rays(sensor, dev(ends), count_only=count_only)
        assert st["rays"] == len(ends) and (st["cleared"] == 0) == bool(count_only), st

    def merge(self, h, src):
        n = self.m[src].sync()[0]
        st = self.m[h].merge_from(self.m[src])
        assert st["merged_nodes"] == st["source_nodes"] == n and st["skipped"] == 0, st

    def reset(self, h):
        self.m[h].reset("slope")

    def accumulate(self, h, pts, base):
        self.m[h].accumulate("slope", dev(pts), first_idx_base=base)

    def finalize(self, h):
        self.m[h].finalize()

    def stats_to(self, h, dst):
        import torch
        st = self.m[h].stats_export()
        torch.cuda.synchronize()
        st = {k: v.clone() for k, v in st.items()}
        half = st["key"].shape[0] // 2
        for sl in (slice(0, half), slice(half, None)):
            self.m[dst].stats_merge(*[st[k][sl].contiguous() for k in ("key", "sums", "count", "first_idx")])

    def reserve(self, h, max_points, max_nodes):
        self.m[h].reserve(max_points, max_nodes)

    def deferred(self, h, on):
        self.m[h].set_deferred_emit(on)

    def query(self, h, model):
        q = model.query_points()
        rows = self.m[h].query(dev(q)).cpu().numpy().astype(np.int64)
        assert np.array_equal(rows, sm.query_rows(model.expected(), q))
        return rows, q

    def refused(self, h, what, pts=None):
        import grid_ndt_amd as g
        m = self.m[h]
        assert m.last_strategy() in PARTITION_FAMILY, m.last_strategy()
        before = m.export()
        with pytest.raises(g.GndtError) as e:
            {"update": lambda: m.change2DMap("slope", dev(pts)), "remove": lambda: m.del2DMap("slope", dev(pts)),
             "stats_export": lambda: m.stats_export()}[what]()
        assert e.value.code == ERR_INVALID, (what, e.value.code)
        _same_bytes(m.export(), before)

    def check(self, h, label, model):
        m, want = self.m[h], model.expected()
        out = m.export()
        parity.assert_parity(model.remap(out), want)
        slopes = int(np.count_nonzero(want["flags"] & 2)) if want["num_nodes"] else 0
        assert m.sync() == (want["num_nodes"], want["num_columns"], slopes), (label, m.sync())
        rows, q = self.query(h, model)
        assert np.array_equal(rows, sm.query_rows(out, q)), label
        if want["num_nodes"]:
            assert (rows[:37] >= 0).all() and (rows[-3:] == -1).all(), label
        else:
            assert (rows == -1).all(), label
        self.checks += 1


@pytest.mark.parametrize("name", list(sm.SCRIPTS))
def test_script(name):
    b = GpuBackend()
    log = sm.run(sm.SCRIPTS[name](), b)
    assert b.checks == sum(1 for e in log if e["kind"] == "check") >= 4


def test_a_reserve_moves_the_rows_of_a_partition_map_with_what_they_hold():
    """gndt_reserve on a handle whose map does not live in the node table (a PARTITION build keeps nothing its rows could be made from
    again): after a reserve that has to move the result rows and their column sizes the export is what it was, byte for byte, and the
    NODE query, whose column index is built from them after the reserve, answers as the export says."""
    b = GpuBackend()
    b.new("p", strategy=sm.AUTO)
    m = b.m["p"]
    cloud = sm.patch(46, 66000, 30.0)
    model = sm.Model()
    model.place(cloud)
    b.build("p", cloud)
    assert m.last_strategy() in PARTITION_FAMILY
    before = m.export()
    m.reserve(1000, 0)                                       # less than the build has allocated: nothing moves
    _same_bytes(m.export(), before)
    m.reserve(1_000_000, 0)                                  # 300 000 rows and more: the result arrays move
    _same_bytes(m.export(), before)
    b.check("p", "after the reserve", model)
    assert m.last_strategy() in PARTITION_FAMILY
    b.build("p", cloud)
    b.check("p", "built again", model)
