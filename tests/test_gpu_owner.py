"""GPU tier: the owner-partitioned build of a sharded cloud (include/gndt.h, gndt_build_owned_device and its four steps).

One MI355X plays W ranks: W handles, every "rank" splits its contiguous range of the cloud by column owner, the runs are
handed over with device copies (what ncclSend / ncclRecv do between GPUs), every rank builds the columns it owns from the
records it received and learns the global row of each of its rows from everybody's column pairs.  The union of the ranks'
rows, scattered by global_row, must be the oracle's map of the whole cloud — keys, order, first-seen indices and labels bit
for bit, statistics within the parity tolerances.  The RCCL composition itself runs with world_size 1 on the box."""
import numpy as np
import pytest

from grid_ndt_amd import scenes
from tests import parity

pytestmark = pytest.mark.gpu

TERRAIN = dict(grid_len=0.2, z_len=0.2, slope_interval=0.08, demand="slope")


def _ranks(cloud, P, W, strategy=0):
    import grid_ndt_amd as g
    maps = []
    for _ in range(W):
        m = g.TwoDmap(P["grid_len"], P["z_len"], strategy=strategy, min_points=P.get("min_points", 3))
        m.setInterval(P["slope_interval"])
        m.setCloudFirst(cloud[0, :3])
        maps.append(m)
    return maps


def owner_build_on_one_gpu(cloud, P, W, bounds=None, strategy=0, locality=False, maps=None):
    """-> (assembled global map as an export() dict, per-rank details).  `locality`: the two optional steps in front
    (gndt_owner_sample_device on every rank, gndt_owner_map_device from everybody's messages) instead of hash ownership.
    `maps`: the W handles of an earlier build with the same origin, instead of fresh ones."""
    import torch
    reused = maps is not None
    maps = maps or _ranks(cloud, P, W, strategy)
    pts = torch.from_numpy(np.ascontiguousarray(cloud[1:])).cuda()
    n = int(pts.shape[0])
    bounds = bounds or [n * r // W for r in range(W + 1)]
    demand = P.get("demand", "slope")
    if locality:
        msgs = torch.cat([maps[r].owner_sample(demand, pts[bounds[r]:bounds[r + 1]]).clone() for r in range(W)]).contiguous()
        for r in range(W):
            maps[r].owner_map(msgs, W)
    elif reused:
        # (a block table stays on its handle for splits among the same W until replaced: a table for one rank is none — the hash again)
        for r in range(W):
            maps[r].owner_map(maps[r].owner_sample(demand, pts[bounds[r]:bounds[r + 1]]).clone(), 1)
    pieces = [[None] * W for _ in range(W)]
    kept = 0
    for r in range(W):
        runs = maps[r].owner_split(demand, pts[bounds[r]:bounds[r + 1]], bounds[r], n, W)
        assert len(runs) == W and sum(int(x.shape[0]) for x in runs) <= bounds[r + 1] - bounds[r]   # (weighted records fold identical points)
        for o in range(W):
            pieces[r][o] = runs[o].clone()
        kept += int(runs[r].shape[0])
    owned_points = []
    for o in range(W):
        own = torch.cat([pieces[r][o] for r in range(W)], 0).contiguous()
        owned_points.append(int(own.shape[0]))
        maps[o].build_records(demand, own, n)
    pairs = [maps[o].owned_columns().clone() for o in range(W)]
    pad = torch.full((5,), -1, dtype=torch.int64, device="cuda")              # (the all-gather's padding is skipped)
    allp = torch.cat([x for p in pairs for x in (p, pad)]).contiguous()
    outs = []
    for o in range(W):
        grow, gn, gc = maps[o].owned_global_rows(allp, n)
        outs.append((maps[o].export(), grow.cpu().numpy().astype(np.int64), gn, gc))
    N, K = outs[0][2], outs[0][3]
    glob = {k: np.zeros((N,) + v.shape[1:], v.dtype) for k, v in outs[0][0].items() if isinstance(v, np.ndarray)}
    seen = np.zeros(N, bool)
    for out, grow, gn, gc in outs:
        assert (gn, gc) == (N, K)
        assert grow.shape[0] == out["num_nodes"]
        assert not seen[grow].any()
        seen[grow] = True
        for k in glob:
            glob[k][grow] = out[k]
    assert seen.all()                                                          # the ranks' rows tile [0, N)
    glob.update(num_nodes=N, num_columns=K, num_slopes=sum(o[0]["num_slopes"] for o in outs))
    return glob, dict(owned_points=owned_points, local_nodes=[o[0]["num_nodes"] for o in outs], pairs=[int(p.shape[0]) for p in pairs],
                      kept_fraction=kept / max(1, sum(owned_points)), maps=maps, ranks=[(o[0], o[1]) for o in outs])


@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_owner_partitioned_build_of_the_campus_frame_equals_the_oracle(W):
    cloud, P = scenes.campus_frame(150_000), scenes.CAMPUS_PARAMS
    ref = parity.ref_from_cloud(cloud, P)
    glob, info = owner_build_on_one_gpu(cloud, P, W)
    parity.assert_parity(glob, ref)
    assert sum(info["local_nodes"]) == ref["num_nodes"]
    if W > 1:                                                                  # the owner hash spreads the columns
        assert min(info["local_nodes"]) > 0.5 * ref["num_nodes"] / W


def test_owner_partitioned_build_with_zero_padding_and_uneven_shards():
    """The reference's own scene: 64 k points at (0,0,0) travel as weighted records (folded where they are split, taken as
    they are by the owner's build); shards of very different sizes, one of them empty."""
    cloud, P = scenes.bridge_ground(), scenes.BRIDGE_PARAMS
    n = cloud.shape[0] - 1
    ref = parity.ref_from_cloud(cloud, P)
    glob, info = owner_build_on_one_gpu(cloud, P, 4, bounds=[0, 1000, 1000, n - 70_000, n])
    parity.assert_parity(glob, ref)
    assert sum(info["owned_points"]) < n - 60_000                              # the padding was folded


def test_owner_partitioned_large_build_takes_the_two_level_partition():
    """Above 2^20 records per rank the owner's build is the two-level pipeline reading records (index words taken as they
    are); the assembled map equals the single-GPU build of the same cloud exactly, row for row."""
    import torch
    import grid_ndt_amd as g
    cloud = scenes.terrain_cloud(5_000_000)
    P = TERRAIN
    glob, info = owner_build_on_one_gpu(cloud, P, 2)
    assert min(info["owned_points"]) > (1 << 20)
    m, one = parity.gpu_from_cloud(cloud, P, on_device=True)
    assert m.last_strategy() == 2
    for k in ("sx", "sy", "sz", "count", "first_idx", "flags"):
        assert np.array_equal(glob[k], one[k]), k
    assert glob["num_nodes"] == one["num_nodes"] and glob["num_columns"] == one["num_columns"] and glob["num_slopes"] == one["num_slopes"]
    # statistics: different summation order only
    assert np.allclose(glob["mean"], one["mean"], rtol=0, atol=1e-6)
    scale = np.abs(one["cov"]).max(axis=1, keepdims=True) + 1e-30
    assert (np.abs(glob["cov"] - one["cov"]) / scale).max() < 1e-5


@pytest.mark.parametrize("W", [2, 4, 8])
def test_locality_aware_ownership_keeps_most_points_where_they_are(W):
    """Contiguous ranges of the LiDAR-ordered terrain: with the sampled block table most records never leave their rank
    (hash ownership keeps 1/W), the load stays balanced, and the assembled map is still the oracle's."""
    cloud = scenes.terrain_cloud(1_500_000)
    ref = parity.ref_from_cloud(cloud, TERRAIN)
    glob, info = owner_build_on_one_gpu(cloud, TERRAIN, W, locality=True)
    parity.assert_parity(glob, ref)
    print("W", W, "kept", round(info["kept_fraction"], 3), "owned", info["owned_points"])
    assert info["kept_fraction"] > 0.6
    assert max(info["owned_points"]) < 1.5 * sum(info["owned_points"]) / W
    _, plain = owner_build_on_one_gpu(cloud, TERRAIN, W, locality=False)
    assert plain["kept_fraction"] < 1.3 / W


def test_locality_aware_ownership_spreads_a_hot_block_and_survives_odd_shards():
    """A cloud that sits in ONE block (the campus frame's columns within a few metres... and the zero padding) must not end up
    on one rank; empty and tiny shards publish their (empty) samples like everybody else."""
    cloud, P = scenes.bridge_ground(), scenes.BRIDGE_PARAMS
    n = cloud.shape[0] - 1
    ref = parity.ref_from_cloud(cloud, P)
    glob, info = owner_build_on_one_gpu(cloud, P, 4, bounds=[0, 1000, 1000, n - 70_000, n], locality=True)
    parity.assert_parity(glob, ref)
    assert min(info["local_nodes"]) > 0.05 * ref["num_nodes"]                 # nobody was left without work


def test_owner_build_over_rccl_with_one_rank():
    """gndt_build_owned_device end to end (RCCL from C++, world_size 1: split, self hand-over, build, column all-gather)."""
    import torch
    import grid_ndt_amd as g
    from grid_ndt_amd.dist import Communicator
    cloud, P = scenes.campus_frame(150_000), scenes.CAMPUS_PARAMS
    ref = parity.ref_from_cloud(cloud, P)
    comm = Communicator.single()
    m = _ranks(cloud, P, 1)[0]
    pts = torch.from_numpy(np.ascontiguousarray(cloud[1:])).cuda()
    grow, info = m.build_owned(comm, P["demand"], pts, 0, pts.shape[0])
    out = m.export()
    parity.assert_parity(out, ref)
    assert np.array_equal(grow.cpu().numpy(), np.arange(out["num_nodes"]))
    assert info["global_nodes"] == ref["num_nodes"] and info["global_columns"] == ref["num_columns"]
    assert info["global_slopes"] == out["num_slopes"] and info["ranks"] == 1 and info["bytes_sent"] == 0
    # a second build on the same handle (steady state) gives the same rows
    grow2, info2 = m.build_owned(comm, P["demand"], pts, 0, pts.shape[0])
    assert np.array_equal(grow2.cpu().numpy(), grow.cpu().numpy()) and info2["global_nodes"] == info["global_nodes"]


def test_owner_build_with_torch_distributed_as_the_transport():
    """grid_ndt_amd.dist.build_owned_map: the four exported steps with torch.distributed (backend nccl = RCCL, world_size 1)
    doing the hand-over — the model for hosts that bring their own transport."""
    import os
    import torch
    import torch.distributed as dist
    from grid_ndt_amd.dist import build_owned_map
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29653")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        cloud = scenes.terrain_cloud(200_000)
        ref = parity.ref_from_cloud(cloud, TERRAIN)
        m = _ranks(cloud, TERRAIN, 1)[0]
        pts = torch.from_numpy(np.ascontiguousarray(cloud[1:])).cuda()
        grow, gn, gc = build_owned_map(m, "slope", pts, 0, pts.shape[0])
        out = m.export()
        parity.assert_parity(out, ref)
        assert (gn, gc) == (ref["num_nodes"], ref["num_columns"])
        assert np.array_equal(grow.cpu().numpy(), np.arange(out["num_nodes"]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n,W", [(1, 2), (7, 4), (300, 8), (5000, 3)])
def test_owner_build_of_tiny_clouds_with_ranks_that_own_nothing(n, W):
    """Fewer points than ranks, ranks whose shard or whose set of owned columns is empty, 16-byte input points, demand "true"."""
    rng = np.random.default_rng(n)
    cloud = np.concatenate([np.float32([[0.1, 0.2, 0.3]]), (rng.random((n, 3)) * [6, 6, 0.4]).astype(np.float32)], 0)
    P = dict(grid_len=0.5, z_len=0.1, slope_interval=0.08, demand="true")
    ref = parity.ref_from_cloud(cloud, P)
    for locality in (False, True):
        glob, info = owner_build_on_one_gpu(cloud, P, W, locality=locality)
        parity.assert_parity(glob, ref, demand="true", adversarial=True)
    # the same through padded 16-byte points (pcl::PointXYZ)
    import torch
    maps = _ranks(cloud, P, 1)
    pts16 = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    pts16[:, :3] = torch.from_numpy(cloud[1:]).cuda()
    pts16[:, 3] = float("nan")                                    # the padding word is never read
    recs = maps[0].owner_split("true", pts16, 0, n, 1)[0]
    maps[0].build_records("true", recs.clone(), n)
    parity.assert_parity(maps[0].export(), ref, demand="true", adversarial=True)


def test_a_small_hash_owned_build_on_the_handles_of_a_large_locality_build():
    """Large then small on the step API: W = 3 handles build a 60 000-point cloud with the sampled block table, then a 3 000-point
    cloud of another place with hash ownership and another total_points.  Both are the oracle's maps, and every rank's rows of the
    second — keys, counts, first indices, flags, global rows — are those of the same build on three fresh handles: nothing of the
    first build (block table, records, column pairs, staging rows) shows through."""
    from tests import stream_model as sm
    W, P = 3, sm.P
    large = np.concatenate([sm.ORIGIN[None, :], sm.patch(81, 60_000, 30.0)])
    small = np.concatenate([sm.ORIGIN[None, :], sm.patch(82, 3_000, 8.0, (-9.0, 12.0))])
    glob, info = owner_build_on_one_gpu(large, P, W, locality=True)
    parity.assert_parity(glob, parity.ref_from_cloud(large, P))
    ref = parity.ref_from_cloud(small, P)
    again, used = owner_build_on_one_gpu(small, P, W, maps=info["maps"])
    parity.assert_parity(again, ref)
    fresh_glob, fresh = owner_build_on_one_gpu(small, P, W)
    parity.assert_parity(fresh_glob, ref)
    assert used["owned_points"] == fresh["owned_points"] and sum(used["local_nodes"]) == ref["num_nodes"] and min(used["local_nodes"]) > 0
    for (a, grow_a), (b, grow_b) in zip(used["ranks"], fresh["ranks"]):
        assert (a["num_nodes"], a["num_columns"], a["num_slopes"]) == (b["num_nodes"], b["num_columns"], b["num_slopes"])
        assert np.array_equal(grow_a, grow_b)
        for k in ("sx", "sy", "sz", "count", "first_idx", "flags"):
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("n", [200_000, 3_000_000])
def test_records_build_from_two_segments_equals_the_single_array_build(n):
    """gndt_build_records2_device (what gndt_build_owned_device uses so that the run a rank keeps is not copied): small builds
    (counting partition: the first segment is copied into the room) and large ones (two level-1 launches into the same regions)."""
    import torch
    cloud = scenes.terrain_cloud(n)
    ref_m, one = parity.gpu_from_cloud(cloud, TERRAIN, on_device=True)
    m = _ranks(cloud, TERRAIN, 1)[0]
    pts = torch.from_numpy(np.ascontiguousarray(cloud[1:])).cuda()
    recs = m.owner_split("slope", pts, 0, pts.shape[0], 1)[0].clone()
    for a in (0, 1, recs.shape[0] // 3, recs.shape[0] - 1, recs.shape[0]):
        first = recs[:a].clone()
        room_and_second = torch.empty_like(recs)
        room_and_second[a:] = recs[a:]
        room_and_second[:a] = float("nan")                        # (never read unless filled by the build itself)
        m.build_records2("slope", first, room_and_second, pts.shape[0])
        out = m.export()
        for k in ("sx", "sy", "sz", "count", "first_idx", "flags"):
            assert np.array_equal(out[k], one[k]), (a, k)
        scale = np.abs(one["cov"]).max(axis=1, keepdims=True) + 1e-30
        assert (np.abs(out["cov"] - one["cov"]) / scale).max() < 1e-5


def test_owner_build_whose_local_build_has_to_be_re_run():
    """A first build without a hint guesses n / 4 nodes; this cloud has more than twice that, so the build inside
    gndt_build_owned_device overflows, is re-run by the rank that owns it, and the column round is repeated (every rank would
    repeat it: they all read the "has to be re-run" word of every rank's message)."""
    import torch
    from grid_ndt_amd.dist import Communicator
    rng = np.random.default_rng(5)
    n = 4_000_000
    cloud = np.concatenate([np.float32([[0.0, 0.0, 0.0]]),
                            np.stack([rng.random(n) * 200 - 100, rng.random(n) * 200 - 100, rng.random(n) * 2 - 1], 1).astype(np.float32)], 0)
    P = dict(grid_len=0.5, z_len=0.1, slope_interval=0.08, demand="slope")
    _, one = parity.gpu_from_cloud(cloud, P, on_device=True)
    assert one["num_nodes"] > n // 2
    comm = Communicator.single()
    m = _ranks(cloud, P, 1)[0]
    pts = torch.from_numpy(np.ascontiguousarray(cloud[1:])).cuda()
    grow, info = m.build_owned(comm, "slope", pts, 0, n)
    assert m.retry_count() >= 1
    out = m.export()
    for k in ("sx", "sy", "sz", "count", "first_idx", "flags"):
        assert np.array_equal(out[k], one[k]), k
    assert info["global_nodes"] == one["num_nodes"] and info["global_columns"] == one["num_columns"]
    assert np.array_equal(grow.cpu().numpy(), np.arange(out["num_nodes"]))


@pytest.mark.parametrize("seed", range(12))
def test_owner_build_fuzz_against_the_single_gpu_build(seed):
    """Random world sizes, shard boundaries (empty shards included), cloud kinds and sizes on either side of the one-pass
    split / one-level / two-level thresholds, with and without the sampled block ownership: the assembled map is the
    single-GPU map, row for row."""
    rng = np.random.default_rng(4000 + seed)
    W = int(rng.integers(1, 9))
    kind = ("terrain", "campus", "uniform", "site")[seed % 4]
    n = int(rng.choice([3_000, 70_000, 400_000, 1_300_000, 2_600_000]))
    if kind == "terrain":
        cloud, P = scenes.terrain_cloud(n), TERRAIN
    elif kind == "campus":
        cloud, P = scenes.campus_frame(n), scenes.CAMPUS_PARAMS
    elif kind == "uniform":
        cloud, P = scenes.uniform_box(n), dict(grid_len=0.5, z_len=0.5, slope_interval=0.08, demand="slope")
    else:
        cloud, P = scenes.site_two_storey(n), dict(grid_len=0.1, z_len=0.1, slope_interval=0.08, demand="slope")
    nb = cloud.shape[0] - 1
    cuts = np.sort(rng.integers(0, nb + 1, size=W - 1)).tolist()
    bounds = [0] + cuts + [nb]
    _, one = parity.gpu_from_cloud(cloud, P, on_device=True)
    glob, info = owner_build_on_one_gpu(cloud, P, W, bounds=bounds, locality=bool(seed & 1))
    print("W", W, kind, n, "bounds", bounds, "owned", info["owned_points"])
    for k in ("sx", "sy", "sz", "count", "first_idx", "flags"):
        assert np.array_equal(glob[k], one[k]), k
    assert (glob["num_nodes"], glob["num_columns"], glob["num_slopes"]) == (one["num_nodes"], one["num_columns"], one["num_slopes"])
    scale = np.abs(one["cov"]).max(axis=1, keepdims=True) + 1e-30
    assert (np.abs(glob["cov"] - one["cov"]) / scale).max() < 1e-5
    assert np.allclose(glob["mean"], one["mean"], rtol=0, atol=2e-6)


def owner_build_with_threads(cloud, P, W, bounds=None):
    """gndt_build_owned_device ITSELF with W ranks: the ranks are W threads of this process on the one GPU, their communicators
    a thread group (gndt_comm_create_threads: device copies + host barriers where RCCL would send and receive)."""
    import threading
    import torch
    from grid_ndt_amd.dist import Communicator
    maps = _ranks(cloud, P, W)
    comms = Communicator.threads(W)
    pts = torch.from_numpy(np.ascontiguousarray(cloud[1:])).cuda()
    n = int(pts.shape[0])
    bounds = bounds or [n * r // W for r in range(W + 1)]
    res, errs = [None] * W, []

    def rank(r):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                grow, info = maps[r].build_owned(comms[r], P.get("demand", "slope"), pts[bounds[r]:bounds[r + 1]], bounds[r], n, s)
                res[r] = (maps[r].export(), grow.cpu().numpy().astype(np.int64), info)
        except Exception as e:                         # (a rank that dies leaves the others at a barrier: report, do not hang the suite)
            errs.append((r, repr(e)))
            import sys
            print(f"owner_build_with_threads: rank {r} of {W} failed: {e!r} (bounds {bounds})", file=sys.stderr, flush=True)
            os._exit(3)

    import os
    th = [threading.Thread(target=rank, args=(r,)) for r in range(W)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
        assert not t.is_alive(), "a rank is stuck"
    assert not errs, errs
    for c in comms:
        c.close()
    N, K = res[0][2]["global_nodes"], res[0][2]["global_columns"]
    glob = {k: np.zeros((N,) + v.shape[1:], v.dtype) for k, v in res[0][0].items() if isinstance(v, np.ndarray)}
    seen = np.zeros(N, bool)
    for out, grow, info in res:
        assert (info["global_nodes"], info["global_columns"], info["ranks"]) == (N, K, W)
        assert not seen[grow].any()
        seen[grow] = True
        for k in glob:
            glob[k][grow] = out[k]
    assert seen.all()
    glob.update(num_nodes=N, num_columns=K, num_slopes=res[0][2]["global_slopes"])
    return glob, [r[2] for r in res]


@pytest.mark.parametrize("W", [2, 3, 4, 8])
def test_the_owner_build_itself_with_several_ranks_on_one_gpu(W):
    """Every rank runs gndt_build_owned_device (ownership from the all-gathered samples, one-pass split, all-to-all, two-segment
    build, column round, global rows); the assembled map is the oracle's.  Only RCCL itself is replaced (thread-group
    communicators)."""
    cloud, P = scenes.terrain_cloud(1_200_000), TERRAIN
    ref = parity.ref_from_cloud(cloud, P)
    glob, infos = owner_build_with_threads(cloud, P, W)
    parity.assert_parity(glob, ref)
    assert glob["num_slopes"] == int(np.count_nonzero(ref["flags"] & 2))
    sent = sum(i["bytes_sent"] for i in infos)
    assert sent == sum(i["bytes_received"] for i in infos) and sent > 0
    kept = 1.0 - sent / 16.0 / sum(i["owned_points"] for i in infos)
    print("W", W, "kept", round(kept, 3), "owned", [i["owned_points"] for i in infos])
    assert kept > 0.5                                                          # locality-aware ownership was in force


def test_the_owner_build_itself_with_ranks_that_get_little_or_nothing():
    cloud, P = scenes.bridge_ground(), scenes.BRIDGE_PARAMS
    n = cloud.shape[0] - 1
    ref = parity.ref_from_cloud(cloud, P)
    glob, infos = owner_build_with_threads(cloud, P, 4, bounds=[0, 1000, 1000, n - 70_000, n])
    parity.assert_parity(glob, ref)
    cloud = scenes.campus_frame(30)                                            # fewer points than there are columns to go round
    ref = parity.ref_from_cloud(cloud, scenes.CAMPUS_PARAMS)
    glob, infos = owner_build_with_threads(cloud, scenes.CAMPUS_PARAMS, 5)
    parity.assert_parity(glob, ref, adversarial=True)


def test_the_owner_build_itself_repeats_the_column_round_when_a_rank_re_runs_its_build():
    """First builds without a hint guess n / 4 nodes; this cloud has more than half as many nodes as points, so both ranks' local
    builds overflow inside the collective sequence: each re-runs its own, and BOTH repeat the column round (they read the same
    "has to be re-run" words)."""
    rng = np.random.default_rng(6)
    n = 3_000_000
    cloud = np.concatenate([np.float32([[0.0, 0.0, 0.0]]),
                            np.stack([rng.random(n) * 200 - 100, rng.random(n) * 200 - 100, rng.random(n) * 2 - 1], 1).astype(np.float32)], 0)
    P = dict(grid_len=0.5, z_len=0.1, slope_interval=0.08, demand="slope")
    _, one = parity.gpu_from_cloud(cloud, P, on_device=True)
    glob, infos = owner_build_with_threads(cloud, P, 2)
    for k in ("sx", "sy", "sz", "count", "first_idx", "flags"):
        assert np.array_equal(glob[k], one[k]), k
    assert glob["num_nodes"] == one["num_nodes"] > n // 2


# ---------------------------------------------------------------------------------------------------------------------
# the assembled map (gndt_gather_owned_map_device): the consumers get ONE map
# ---------------------------------------------------------------------------------------------------------------------
def test_the_owner_build_of_a_cloud_whose_records_do_not_fit_the_partition_pipeline():
    """One column with ~4000 z levels: every node of it belongs to ONE bucket, more than any LDS table holds.  A single-GPU build
    then takes the node table in HBM; the owner's build from records used to give up with GNDT_ERR_CAPACITY (found by
    tools/fuzz_owner.py) and now does the same: k_accumulate reads the records (index words and weights as they are)."""
    rng = np.random.default_rng(21)
    n = 300_000
    xyz = np.stack([0.3 + 0.1 * rng.random(n), -0.7 + 0.1 * rng.random(n), rng.random(n) * 400.0 - 200.0], 1).astype(np.float32)
    xyz[1000:1000 + 640] = xyz[1000]                      # ten waves of identical points: weighted records through the fallback
    ground = np.stack([rng.random(n) * 40 - 20, rng.random(n) * 40 - 20, 0.02 * rng.normal(size=n)], 1).astype(np.float32)
    cloud = np.concatenate([xyz[:1], xyz, ground], 0)
    P = dict(grid_len=0.5, z_len=0.1, slope_interval=0.08, demand="slope")
    _, one = parity.gpu_from_cloud(cloud, P, on_device=True)
    ref = parity.ref_from_cloud(cloud, P)
    for W in (1, 3):
        glob, infos = owner_build_with_threads(cloud, P, W)
        rep = parity.compare(glob, ref, dense=True)            # (the pole's nodes: 30 points each at |z| up to 200 m — the fp32 oracle's own
        assert rep["ok"], rep["fail"]                           #  scatter is 1e-3 off there: held to the fp64 truth, labels to the margin)
        for k in ("sx", "sy", "sz", "count", "first_idx", "flags"):
            assert np.array_equal(glob[k], one[k]), (W, k)


def _threads(W, body):
    """Run body(r) on W threads (one per thread-group rank); returns the list of results, re-raises the first failure."""
    import threading
    res, errs = [None] * W, []

    def run(r):
        try:
            res[r] = body(r)
        except BaseException as e:            # noqa: BLE001 — collected and re-raised on the test's thread
            errs.append((r, e))

    th = [threading.Thread(target=run, args=(r,)) for r in range(W)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
        assert not t.is_alive(), "a rank is stuck"
    return res, errs


@pytest.mark.parametrize("W,root", [(2, 0), (4, 2), (8, -1), (3, -1)])
def test_gathered_owner_build_is_the_single_gpu_map_and_floods_like_it(W, root):
    """All ranks build their columns, the rows travel to `root` (or to everybody) and are scattered by their global row: that
    handle's export is the single-GPU export row for row, and gndt_compute_cost on it gives the single-GPU flood bit for bit."""
    import torch
    from grid_ndt_amd.dist import Communicator
    cloud, P = scenes.drivable_site(400_000), scenes.COST_PARAMS
    goal = np.asarray(scenes.DRIVABLE_GOAL, np.float32)
    m1, one = parity.gpu_from_cloud(cloud, P, on_device=True)
    st1 = m1.computeCost(goal)
    c1 = m1.cost_export()
    h1, s1 = c1["h"], c1["state"]
    assert st1["rc"] == 0 and st1["traversable"] > 100
    maps, comms = _ranks(cloud, P, W), Communicator.threads(W)
    pts = torch.from_numpy(np.ascontiguousarray(cloud[1:])).cuda()
    n = int(pts.shape[0])
    bounds = [n * r // W for r in range(W + 1)]

    def rank(r):
        torch.cuda.set_device(0)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            grow, info = maps[r].build_owned(comms[r], P["demand"], pts[bounds[r]:bounds[r + 1]], bounds[r], n, s)
            local_nodes = info["local_nodes"]
            maps[r].gather_owned(comms[r], root, s)
            out = maps[r].export()
            cost = None
            if root < 0 or r == root:
                st = maps[r].computeCost(goal, stream=s)
                ce = maps[r].cost_export()
                cost = (st, ce["h"], ce["state"])
            return out, local_nodes, info, cost

    res, errs = _threads(W, rank)
    assert not errs, errs
    for r in range(W):
        out, local_nodes, info, cost = res[r]
        if root >= 0 and r != root:
            assert out["num_nodes"] == local_nodes                 # the other ranks keep the columns they own
            continue
        assert (out["num_nodes"], out["num_columns"], out["num_slopes"]) == (one["num_nodes"], one["num_columns"], one["num_slopes"])
        for k in ("sx", "sy", "sz", "count", "first_idx", "flags"):
            assert np.array_equal(out[k], one[k]), (r, k)
        scale = np.abs(one["cov"]).max(axis=1, keepdims=True) + 1e-30
        assert (np.abs(out["cov"] - one["cov"]) / scale).max() < 1e-5
        assert np.allclose(out["mean"], one["mean"], rtol=0, atol=2e-6)
        st, h, state = cost
        assert st["rc"] == 0 and st["traversable"] == st1["traversable"] and st["closed"] == st1["closed"]
        assert np.array_equal(state, s1)
        # h is a sum of fp32 distances between fp32 means: identical wherever the means are bit-identical (different summation
        # order of the fp64 statistics can move a mean by an ulp)
        same = np.all(out["mean"] == one["mean"], axis=1)
        assert same.mean() > 0.99
        assert np.allclose(h, h1, rtol=1e-5, atol=1e-5)
    for c in comms:
        c.close()


@pytest.mark.parametrize("W", [1, 2, 5, 8])
def test_communicator_selftest_verifies_every_collective(W):
    """gndt_comm_selftest: all-gather, send/recv all-to-all, reduce-scatter, all-reduce (f64 sum, u32 min), each checked against what
    it must produce — on thread ranks (device copies) here, on RCCL with one rank in tests/test_gpu_bench_line.py, and by
    bench.py --gpus N before its first build on a real node."""
    import torch
    from grid_ndt_amd.dist import Communicator
    cloud, P = scenes.campus_frame(5000), scenes.CAMPUS_PARAMS
    maps, comms = _ranks(cloud, P, W), Communicator.threads(W)

    def rank(r):
        torch.cuda.set_device(0)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            return maps[r].comm_selftest(comms[r], s)

    res, errs = _threads(W, rank)
    assert not errs, errs
    assert all(rep["ok_mask"] == 15 and rep["ranks"] == W for rep in res), res
    for c in comms:
        c.close()


def test_a_second_gather_of_the_same_build_is_refused_on_every_rank():
    """After a rooted gather the root's handle holds the whole map and no longer its owned rows.  A second gather of the same build
    is refused on EVERY rank before any collective (round 3: the old root returned and the others waited in the exchange for ever);
    a new owned build makes the gather legal again."""
    import torch
    from grid_ndt_amd._lib import GndtError
    from grid_ndt_amd.dist import Communicator
    W = 3
    cloud, P = scenes.campus_frame(90_000), scenes.CAMPUS_PARAMS
    maps, comms = _ranks(cloud, P, W), Communicator.threads(W)
    pts = torch.from_numpy(np.ascontiguousarray(cloud[1:])).cuda()
    n = int(pts.shape[0])
    bounds = [n * r // W for r in range(W + 1)]

    def rank(r):
        torch.cuda.set_device(0)
        s = torch.cuda.Stream()
        codes = []
        with torch.cuda.stream(s):
            for root in (0, 1):
                maps[r].build_owned(comms[r], P["demand"], pts[bounds[r]:bounds[r + 1]], bounds[r], n, s)
                maps[r].gather_owned(comms[r], root, s)
                try:
                    maps[r].gather_owned(comms[r], (root + 1) % W, s)
                    codes.append(0)
                except GndtError as e:
                    codes.append(e.code)
        return codes

    res, errs = _threads(W, rank)
    assert not errs, errs
    assert all(c == [1, 1] for c in res), res          # GNDT_ERR_INVALID everywhere, twice; nobody hung
    for c in comms:
        c.close()


def test_a_failing_rank_takes_every_rank_out_of_the_owner_build_together():
    """One rank's shard holds a point outside the key range.  Nobody hangs: that rank reports KEY_RANGE, the others PEER, all
    at the same collective; the same communicators and handles then build a clean cloud."""
    import torch
    from grid_ndt_amd._lib import GndtError
    from grid_ndt_amd.dist import Communicator
    W = 4
    cloud, P = scenes.campus_frame(120_000), scenes.CAMPUS_PARAMS
    bad = cloud.copy()
    bad[70_000, 0] = 5.0e4                                        # |nx| = 1e5 cells of 0.5 m: beyond 65535
    maps, comms = _ranks(cloud, P, W), Communicator.threads(W)
    n = cloud.shape[0] - 1
    bounds = [n * r // W for r in range(W + 1)]
    culprit = next(r for r in range(W) if bounds[r] <= 70_000 - 1 < bounds[r + 1])

    def attempt(src):
        pts = torch.from_numpy(np.ascontiguousarray(src[1:])).cuda()

        def rank(r):
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                try:
                    grow, info = maps[r].build_owned(comms[r], P["demand"], pts[bounds[r]:bounds[r + 1]], bounds[r], n, s)
                    return ("ok", info["global_nodes"])
                except GndtError as e:
                    return ("err", e.code)
        res, errs = _threads(W, rank)
        assert not errs, errs
        return res

    res = attempt(bad)
    for r in range(W):
        assert res[r] == ("err", 4 if r == culprit else 7), (r, res)
    ref = parity.ref_from_cloud(cloud, P)
    res = attempt(cloud)
    assert all(x == ("ok", ref["num_nodes"]) for x in res), res
    for c in comms:
        c.close()


@pytest.mark.parametrize("site,where", [(4, "build"), (1, "build"), (2, "build"), (3, "gather")])
def test_an_allocation_failure_between_two_collectives_takes_every_rank_out_together(site, where):
    """VERDICT r4 (missing 5): a rank that cannot grow a buffer BETWEEN two collectives of the owner-partitioned build (or of the
    gather) used to return on its own and leave its peers waiting in the next collective for ever.  The failure is injected
    (gndt_debug_fail_next_alloc) on ONE of three thread ranks at each of the four sites — the first build's message buffers, the
    exchange's receive buffer, the column-pair buffers, the gather's buffers: within a second every rank is back, the culprit
    with NOMEM (6), the others with PEER (7); the same handles and communicators then build and gather the clean map."""
    import time
    import torch
    from grid_ndt_amd._lib import GndtError
    from grid_ndt_amd.dist import Communicator
    W, culprit = 3, 1
    cloud, P = scenes.campus_frame(150_000), scenes.CAMPUS_PARAMS
    ref = parity.ref_from_cloud(cloud, P)
    maps, comms = _ranks(cloud, P, W), Communicator.threads(W)
    pts = torch.from_numpy(np.ascontiguousarray(cloud[1:])).cuda()
    n = int(pts.shape[0])
    bounds = [n * r // W for r in range(W + 1)]

    def attempt(inject):
        def rank(r):
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                if inject and r == culprit:
                    maps[r].debug_fail_next_alloc(site, P["demand"])
                t0 = time.perf_counter()
                try:
                    grow, info = maps[r].build_owned(comms[r], P["demand"], pts[bounds[r]:bounds[r + 1]], bounds[r], n, s)
                    maps[r].gather_owned(comms[r], -1, s)
                    return ("ok", maps[r].export(), time.perf_counter() - t0)
                except GndtError as e:
                    return ("err", e.code, time.perf_counter() - t0)
        res, errs = _threads(W, rank)
        assert not errs, errs
        return res

    res = attempt(True)
    for r in range(W):
        assert res[r][:2] == ("err", 6 if r == culprit else 7), (site, r, res[r][:2])
        assert res[r][2] < 5.0, (site, r, res[r][2])          # (seconds: nobody waited for a peer that had left)
    res = attempt(False)                                     # the same handles, the same communicators: the clean map, on every rank
    for r in range(W):
        assert res[r][0] == "ok", (site, r, res[r][:2])
        rep = parity.compare(res[r][1], ref)
        assert rep["ok"], (site, r, rep["fail"])
    for c in comms:
        c.close()


def global_build_with_threads(cloud, P, W, bounds=None):
    """gndt_build_global_device with W thread-group ranks on one GPU: every rank ends with the map of the whole cloud."""
    import torch
    from grid_ndt_amd.dist import Communicator
    maps, comms = _ranks(cloud, P, W), Communicator.threads(W)
    pts = torch.from_numpy(np.ascontiguousarray(cloud[1:])).cuda()
    n = int(pts.shape[0])
    bounds = bounds or [n * r // W for r in range(W + 1)]

    def rank(r):
        torch.cuda.set_device(0)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            maps[r].build_global(comms[r], P.get("demand", "slope"), pts[bounds[r]:bounds[r + 1]], bounds[r], n, s)
            return maps[r].export()

    res, errs = _threads(W, rank)
    for c in comms:
        c.close()
    assert not errs, errs
    return res


@pytest.mark.parametrize("W", [2, 3, 8])
def test_the_global_build_itself_with_several_ranks_on_one_gpu(W):
    """BASELINE configs[2]'s literal "cell-stat all-reduce" (gndt_build_global_device) with W ranks: shard statistics, key
    all-gather, canonical order, packed sum / min all-reduce, the whole map finalised on every rank.  Only RCCL itself is
    replaced (thread-group communicators); every rank's map is the single-GPU map of the cloud row for row."""
    cloud, P = scenes.terrain_cloud(900_000), TERRAIN
    _, one = parity.gpu_from_cloud(cloud, P, on_device=True)
    n = cloud.shape[0] - 1
    bounds = None if W != 3 else [0, 17, 17, n]               # a tiny shard and an empty one
    for out in global_build_with_threads(cloud, P, W, bounds):
        assert (out["num_nodes"], out["num_columns"], out["num_slopes"]) == (one["num_nodes"], one["num_columns"], one["num_slopes"])
        for k in ("sx", "sy", "sz", "count", "first_idx", "flags"):
            assert np.array_equal(out[k], one[k]), k
        scale = np.abs(one["cov"]).max(axis=1, keepdims=True) + 1e-30
        assert (np.abs(out["cov"] - one["cov"]) / scale).max() < 1e-5
        assert np.allclose(out["mean"], one["mean"], rtol=0, atol=2e-6)


def test_a_first_build_on_a_busy_gpu_keeps_its_overflow_flags():
    """Six host threads, each with a FRESH handle, build their shards of a cloud with two hot columns at once: every shard's first
    attempt overflows a fixed-capacity region and must be re-run.  The flags used to be zeroed with hipMemset when the handle
    allocated them — a fill on the null stream, not ordered with the build's stream, that ran late on the busy GPU and wiped the
    flag the build had just raised: 3 % of such runs lost the points that had not fit (found by tools/fuzz_owner.py)."""
    rng = np.random.default_rng(31)
    n = 2_000_000
    xyz = np.stack([rng.random(n) * 60 - 30, rng.random(n) * 60 - 30, 0.05 * rng.normal(size=n)], 1)
    hot = rng.random(n) < 0.25
    xyz[hot, 0] = np.where(rng.random(hot.sum()) < 0.5, 15.3, 13.6) + 0.05 * rng.random(hot.sum())
    xyz[hot, 1] = np.where(xyz[hot, 0] > 14.0, 14.2, 15.7) + 0.05 * rng.random(hot.sum())
    xyz[hot, 2] = rng.random(hot.sum()) * 3.0
    cloud = np.concatenate([np.float32([[0.1, 0.2, 0.0]]), xyz.astype(np.float32)], 0)
    P = dict(grid_len=1.0, z_len=0.1, slope_interval=0.08, demand="slope")
    _, one = parity.gpu_from_cloud(cloud, P, on_device=True)
    bounds = [int(f * n) for f in (0, 0.12, 0.38, 0.39, 0.44, 0.87, 1.0)]      # uneven: the ranks reach their first launch at different times
    for it in range(150):
        for out in global_build_with_threads(cloud, P, 6, bounds):
            assert out["num_nodes"] == one["num_nodes"], (it, out["num_nodes"], one["num_nodes"])
            assert np.array_equal(out["count"], one["count"]), it
