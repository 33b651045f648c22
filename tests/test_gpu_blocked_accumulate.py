"""GPU tier: the accumulate phase of BLOCKED buckets (gndt_blocked.hpp) — a counting sort of each chunk of a bucket's records by slot,
the slot's thread adding its run into registers.  The cases aim at what that phase adds: blocks whose records span several chunks, one
long run (a node of nearly a quarter of its block's points), weighted records (64 and 512 identical points in one record) and a record
outside its bucket's block that comes in a late chunk.  Whatever the chunks, the map is the oracle's."""
import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import parity
from tests.gpu_kit import dev, handle

pytestmark = pytest.mark.gpu

P = dict(grid_len=0.5, z_len=0.5, slope_interval=0.08)
BLOCKED = 7      # GNDT_STRATEGY_PARTITION_BLOCKED


def _blocked_builds(cloud, builds=3):
    """Builds of `cloud` on a fresh handle: the first teaches the handle the box, the later ones must take blocked buckets and give
    the oracle's map."""
    ref = parity.ref_from_cloud(cloud, P, mode=2)
    m = handle(P)
    m.setCloudFirst(cloud[0])
    t = dev(cloud[1:])
    for k in range(builds):
        m.create2DMap("slope", t)
        out = m.export()
        if k:
            assert m.last_strategy() == BLOCKED and m.retry_count() == 0, (k, m.STRATEGY_NAMES[m.last_strategy()])
        rep = parity.compare(out, ref)
        assert rep["ok"], (k, rep["fail"])
    return m


def test_blocks_of_three_chunks():
    # 200 x 200 columns x 4 levels in blocks of 8 x 8 x 8: 625 blocks of ~4 800 points — three chunks of 2 048 records each
    _blocked_builds(scenes.uniform_box(3_000_001, half_xy=50.0))


def test_one_node_of_nearly_a_quarter_of_its_block():
    # ~4 000 points per block; the host takes blocks while its largest node holds at most a quarter of that: ~960 points in one node,
    # spread over the cloud (the cloud keeps no locality) and inside the cell (no run of identical points)
    cloud = scenes.uniform_box(2_500_001, half_xy=50.0)
    rng = np.random.default_rng(7)
    at = rng.choice(np.arange(1, cloud.shape[0]), 940, replace=False)
    cloud[at, 0] = rng.uniform(10.05, 10.45, at.size).astype(np.float32)
    cloud[at, 1] = rng.uniform(-20.45, -20.05, at.size).astype(np.float32)
    cloud[at, 2] = rng.uniform(0.05, 0.45, at.size).astype(np.float32)
    _blocked_builds(cloud)


@pytest.mark.parametrize("run", [128, 1024])
def test_weighted_records_in_a_blocked_build(run):
    # a run of identical points aligned to 512: the partition folds 64 (and, for 1 024, 512) identical points into one weighted record
    cloud = scenes.uniform_box(3_000_001, half_xy=50.0)
    s = 1 + 512 * 3001
    cloud[s:s + run] = np.array([3.3, -7.1, 0.2], np.float32)
    _blocked_builds(cloud)


def test_out_of_block_record_in_a_late_chunk_reruns_hashed():
    cloud = scenes.uniform_box(3_000_001, half_xy=50.0)
    m = _blocked_builds(cloud, builds=2)
    late = cloud.copy()
    late[-1] = np.array([1.1, 1.1, 6.2], np.float32)      # the last point, 12 levels up: beyond its block's levels
    m.create2DMap("slope", dev(late[1:]))
    out = m.export()
    assert m.last_strategy() != BLOCKED and m.retry_count() >= 1
    rep = parity.compare(out, parity.ref_from_cloud(late, P, mode=2))
    assert rep["ok"], rep["fail"]
