"""GPU tier: every block shape of k_bucket_blocked (gndt_blocked.hpp).  The kernel lays 512 nodes out as 2^shx x 2^shy columns x 2^shz
levels, shz = 0 .. 5: 512, 256, 128, 64, 32 or 16 columns per block.  The scenes of tests/blocked_scenes.py make the handle take each
of them — the column prefix across waves (128 columns and more), columns shorter than the four-wide level loop (one and two levels),
16-column blocks, boxes that do not straddle the origin, a moved origin, level padding, nodes below min_points, adjacent-level means
about one slope interval apart — and the handle says which layout it took (TwoDmap.block_layout()), so a scene that stops reaching its
shape fails instead of passing on another one.  Whatever the shape, the map is the oracle's by parity.compare's strict gates
(tests/test_blocked_scenes_host.py: the oracle alone passes them on these scenes, no node on a widened allowance)."""
import numpy as np
import pytest

from tests import blocked_scenes as bs
from tests import parity
from tests.gpu_kit import dev, handle

pytestmark = pytest.mark.gpu

BLOCKED = 7             # GNDT_STRATEGY_PARTITION_BLOCKED
ERR_KEY_RANGE = 4


def _is_the_oracles_map(m, ref, P, what):
    rep = parity.compare(m.export(), ref, P["demand"], min_points=P["min_points"])
    assert rep["ok"], (what, m.STRATEGY_NAMES[m.last_strategy()], rep["fail"])
    return rep


def _shape_and_parity(name, demand, min_points=3):
    """Three builds of the scene on a fresh handle and one of another cloud of the same box: every map the oracle's, the layout after
    the first build what the layout rule gives on the oracle's map, every later build blocked and not re-run.  -> the handle."""
    P = bs.params(name, demand, min_points)
    cloud = bs.cloud(name)
    ref = parity.ref_from_cloud(cloud, P, mode=2)
    want = bs.plan(ref, bs.POINTS)
    assert (1 << want["shx"], 1 << want["shy"], 1 << want["shz"]) == bs.SCENES[name]["block"], want      # (the fixture: also CPU tier)
    m = handle(P, min_points=P["min_points"])
    m.setCloudFirst(cloud[0])
    t = dev(cloud[1:], copy=True)
    for k in range(3):
        m.create2DMap(demand, t)
        _is_the_oracles_map(m, ref, P, (name, "build", k))
        if k == 0:
            got = m.block_layout()
            print(f"[blocked shapes] {name} {demand} min_points={min_points}: {got}")
            assert got == want, (got, want)
        else:
            assert m.last_strategy() == BLOCKED and m.retry_count() == 0, (k, m.STRATEGY_NAMES[m.last_strategy()], m.retry_count())
    other = bs.cloud(name, bs.SEED + 1)
    m.create2DMap(demand, dev(other[1:], copy=True))
    _is_the_oracles_map(m, parity.ref_from_cloud(other, P, mode=2), P, (name, "other cloud"))
    assert m.last_strategy() == BLOCKED and m.retry_count() == 0, (m.STRATEGY_NAMES[m.last_strategy()], m.retry_count())
    assert m.block_layout() == want
    return m


@pytest.mark.parametrize("demand", ["slope", "true"])
@pytest.mark.parametrize("name", list(bs.SCENES))
def test_every_block_shape_is_taken_and_gives_the_oracles_map(name, demand):
    _shape_and_parity(name, demand)


@pytest.mark.parametrize("name", ["levels_4_at_interval", "levels_16_off_origin"])
def test_min_points_5(name):
    """Thousands of nodes without statistics: a neighbour one level up or down counts with its mean z only if it was seen earlier AND
    has statistics, else with 0.0f."""
    _shape_and_parity(name, "slope", min_points=5)


def test_key_range_errors_inside_a_blocked_build():
    """A level beyond 2^21 - 1 (found by the bucket kernel) and a column beyond 65535 (found by the partition, forwarded by the bucket
    kernel's first workgroup): reported, and the handle builds the clean cloud again afterwards."""
    import grid_ndt_amd as g
    name = "levels_4_at_interval"
    P = bs.params(name)
    cloud = bs.cloud(name)
    ref = parity.ref_from_cloud(cloud, P, mode=2)
    m = handle(P, min_points=P["min_points"])
    m.setCloudFirst(cloud[0])
    t = dev(cloud[1:], copy=True)
    for _ in range(2):
        m.create2DMap("slope", t)
        m.sync()
    assert m.last_strategy() == BLOCKED
    for axis, value in ((2, 2.0e5), (0, 0.5 * 70000)):       # |nz| = 2.5 M > 2^21 - 1; |nx| = 70 000 > 65 535
        bad = cloud.copy()
        bad[-1, axis] = np.float32(value)
        with pytest.raises(g.GndtError) as e:
            m.create2DMap("slope", dev(bad[1:], copy=True))
            m.sync()
        assert e.value.code == ERR_KEY_RANGE, str(e.value)
        during = m.STRATEGY_NAMES[m.last_strategy()]
        m.create2DMap("slope", t)
        _is_the_oracles_map(m, ref, P, ("after a key-range error on axis", axis))
        print(f"[blocked shapes] key-range error on axis {axis}: build with the error ran {during}, the clean build after it "
              f"{m.STRATEGY_NAMES[m.last_strategy()]}, re-runs so far {m.retry_count()}")


def test_staging_rows_run_out_inside_a_blocked_build():
    """The handle learns a cloud of 62 k nodes and sizes its staging rows for it; a cloud of the same box and size with twice the nodes
    then runs out of rows inside the blocked bucket kernel (sbase + M > stage_cap) and the build is run again with more."""
    name = "levels_4_at_interval"
    P = bs.params(name)
    b = bs.cloud(name)
    a = bs.folded(b)
    ref_a = parity.ref_from_cloud(a, P, mode=2)
    assert int(ref_a["num_nodes"]) == bs.FOLDED_NODES
    m = handle(P, min_points=P["min_points"])
    m.setCloudFirst(a[0])
    ta = dev(a[1:], copy=True)
    for k in range(2):
        m.create2DMap("slope", ta)
        _is_the_oracles_map(m, ref_a, P, ("folded cloud, build", k))
    assert m.last_strategy() == BLOCKED
    before = m.retry_count()
    m.create2DMap("slope", dev(b[1:], copy=True))
    _is_the_oracles_map(m, parity.ref_from_cloud(b, P, mode=2), P, "unfolded cloud")
    print(f"[blocked shapes] staging rows: re-runs {before} -> {m.retry_count()}, the build ended as {m.STRATEGY_NAMES[m.last_strategy()]}")
    assert m.retry_count() > before
