"""Scan segmentation restated from the definition (include/gndt.h "scan segmentation"): the class of a point from tests/score_ref.py's
per-point d2 (rounded to float32, as gndt_score_poses reports it), the novel cells in a dict, the components by a breadth-first search,
the records in Python integers.  Shares no code with grid_ndt_amd/csrc/gndt_segment.hpp.  Also the scans the segmentation tests draw:
a floor of cells (tests/frontier_ref.cells_cloud) and boxes of points over it.  Shared by the CPU tier (tests/test_segment_host.py) and
the GPU tier (tests/test_gpu_segment.py).  Test infrastructure only."""
from collections import deque

import numpy as np

from tests import frontier_ref as fr
from tests import query_ref as qr
from tests import score_ref as sr

UNKEYED, EXPLAINED, OFF_SURFACE, UNMAPPED = 0, 1, 2, 3
NO_ROW = 0xFFFFFFFF
NOVEL_D2 = np.float32(11.345)
BOTH = (1 << OFF_SURFACE) | (1 << UNMAPPED)
RECORD = np.dtype([("label", np.uint32), ("cells", np.uint32), ("off_surface", np.uint32), ("unmapped", np.uint32),
                   ("sx_min", np.int32), ("sx_max", np.int32), ("sy_min", np.int32), ("sy_max", np.int32), ("sz_min", np.int32),
                   ("sz_max", np.int32), ("sum_x", np.int64), ("sum_y", np.int64), ("sum_z", np.int64), ("z_lo", np.float32),
                   ("z_hi", np.float32)])
assert RECORD.itemsize == 72


def z_image(z):
    """the order-preserving unsigned image of float32 values (-0 below +0)"""
    u = np.asarray(z, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def class_of(keyed, d2, novel_d2=0.0):
    """the class from whether the point has a key and its least d2 as float32 (inf: no candidate counts)"""
    lim = np.float32(novel_d2) if novel_d2 else NOVEL_D2
    d2 = np.asarray(d2, np.float32)
    return np.where(~np.asarray(keyed, bool), UNKEYED, np.where(np.isinf(d2), UNMAPPED, np.where(d2 <= lim, EXPLAINED, OFF_SURFACE))).astype(np.uint8)


def moved(pts, pose):
    """q: the points themselves without a pose, scan scoring's transform with one"""
    pts = np.asarray(pts, np.float32)[:, :3]
    return np.ascontiguousarray(pts) if pose is None else sr.transform(sr.as_poses(pose)[0], pts)


def classify(cells, origin, grid_len, z_len, pts, pose=None, nbh=sr.DIRECT7, novel_d2=0.0, min_points=3, **score_params):
    """-> (class uint8 [n], q float32 [n, 3], (sx, sy, sz) of q, d2 float32 [n])"""
    q = moved(pts, pose)
    prm = sr.defaults(min_points=min_points, **score_params)
    per = sr.score_pose(sr.Nodes(cells), origin, grid_len, z_len, q, np.eye(4)[:3], nbh, prm) if len(q) else None
    sx, sy, sz, _, ok = qr.keys(q, origin, grid_len, z_len)
    with np.errstate(over="ignore"):
        d2 = per["d2"].astype(np.float32) if len(q) else np.zeros(0, np.float32)
    if len(q):      # (the identity through score_ref's transform leaves finite points as they are but for the sign of a zero)
        same = np.isfinite(q).all(1)
        assert np.array_equal(per["q"][same], q[same])
    return class_of(ok, d2, novel_d2), q, (sx, sy, sz), d2


def _exists(k):
    return abs(k[0]) <= qr.MAX_XY and abs(k[1]) <= qr.MAX_XY and abs(k[2]) <= qr.MAX_Z


def neighbours(k, connectivity):
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                steps = abs(dx) + abs(dy) + abs(dz)
                if steps == 0 or (connectivity == 6 and steps != 1):
                    continue
                nb = tuple(fr.step(v, d) if d else v for v, d in zip(k, (dx, dy, dz)))
                if _exists(nb):
                    out.append(nb)
    return out


def segment(cells, origin, grid_len, z_len, pts, pose=None, nbh=sr.DIRECT7, novel_d2=0.0, classes=0, min_points=0, connectivity=0,
            map_min_points=3, **score_params):
    """-> dict(point_class uint8 [n], point_label uint32 [n], clusters: RECORD array of EVERY cluster in ascending label, novel_points,
    novel_cells, d2 (float32), q)"""
    classes = classes or BOTH
    min_points = max(int(min_points), 1)
    connectivity = connectivity or 26
    assert connectivity in (6, 26) and not classes & ~BOTH
    cls, q, (sx, sy, sz), d2 = classify(cells, origin, grid_len, z_len, pts, pose, nbh, novel_d2, map_min_points, **score_params)
    n = len(q)
    novel = [bool((classes >> int(c)) & 1) for c in cls]
    members = {}
    for i in range(n):
        if novel[i]:
            members.setdefault((int(sx[i]), int(sy[i]), int(sz[i])), []).append(i)
    ncells = {k: v for k, v in members.items() if len(v) >= min_points}
    label = np.full(n, NO_ROW, np.uint32)
    with np.errstate(invalid="ignore"):               # (a point without a key is in no cluster: its sum is never read)
        fixed = np.rint(q.astype(np.float64) * 1024.0).astype(np.int64) if n else np.zeros((0, 3), np.int64)
    img = z_image(q[:, 2]) if n else np.zeros(0, np.int64)
    seen, recs = set(), []
    for start in sorted(ncells, key=lambda k: ncells[k][0]):
        if start in seen:
            continue
        seen.add(start)
        comp, todo = [], deque([start])
        while todo:
            k = todo.popleft()
            comp.append(k)
            for nb in neighbours(k, connectivity):
                if nb in ncells and nb not in seen:
                    seen.add(nb)
                    todo.append(nb)
        idx = [i for k in comp for i in ncells[k]]
        lab = min(idx)
        label[idx] = lab
        lo, hi = min(idx, key=lambda i: int(img[i])), max(idx, key=lambda i: int(img[i]))
        recs.append((lab, len(comp), sum(1 for i in idx if cls[i] == OFF_SURFACE), sum(1 for i in idx if cls[i] == UNMAPPED),
                     min(k[0] for k in comp), max(k[0] for k in comp), min(k[1] for k in comp), max(k[1] for k in comp),
                     min(k[2] for k in comp), max(k[2] for k in comp), sum(int(fixed[i, 0]) for i in idx), sum(int(fixed[i, 1]) for i in idx),
                     sum(int(fixed[i, 2]) for i in idx), q[lo, 2], q[hi, 2]))
    recs.sort(key=lambda r: r[0])
    return dict(point_class=cls, point_label=label, clusters=np.array(recs, RECORD), novel_points=int(sum(novel)), novel_cells=len(ncells), d2=d2, q=q)


def listed(ref, min_cluster_points=1, min_cluster_cells=1):
    """-> (the records of the list, the call's four counts) for the cluster-size filters (0 = 1)"""
    c = ref["clusters"]
    pts = c["off_surface"].astype(np.int64) + c["unmapped"]
    keep = (pts >= max(int(min_cluster_points), 1)) & (c["cells"] >= max(int(min_cluster_cells), 1))
    return c[keep], np.array([int(keep.sum()), ref["novel_points"], ref["novel_cells"], len(c)], np.uint32)


def same_records(got, want):
    """bytes for bytes (z_lo and z_hi as their bit patterns)"""
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def diff_records(got, want):
    """what differs, for an assertion's message"""
    if got.shape != want.shape:
        return f"{got.shape[0]} records, want {want.shape[0]}"
    for k in RECORD.names:
        v = np.uint32 if RECORD[k].itemsize == 4 else np.uint64
        bad = np.flatnonzero(got[k].view(v) != want[k].view(v))
        if len(bad):
            return f"{k}: records {bad[:5]} got {got[k][bad[:5]]} want {want[k][bad[:5]]}"
    return ""


def has_every_class_and_two_clusters(ref):
    """a scene where nothing is novel proves nothing: asserted on the restatement's own output before anything is compared with it"""
    return all((ref["point_class"] == c).any() for c in (EXPLAINED, OFF_SURFACE, UNMAPPED)) and len(ref["clusters"]) >= 2


# ---- hand-drawn scans over frontier_ref's floors ---------------------------------------------------------------------------------------
GL, ZL = fr.GL, fr.ZL
P = fr.P


def floor_cells(W=16, H=16, x0=-8, y0=-8):
    """one storey of W x H columns from cell (x0, y0) on: nine points a node"""
    return [(ix, iy) for ix in range(x0, x0 + W) for iy in range(y0, y0 + H)]


def cell_points(cells, per=2, jitter=0):
    """`per` points inside each cell (ix, iy, iz) of the lattice without the hole — cell ix spans [ix * GL, (ix + 1) * GL) from the
    floor's origin, level iz spans [iz * ZL, (iz + 1) * ZL) — cell after cell; lin(s) of the cell's signed index is the lattice index"""
    cells = np.asarray(list(cells), np.float64).reshape(-1, 3)
    t = (np.arange(per, dtype=np.float64)[None, :] + 1.0) / (per + 1.0)                 # strictly inside the cell
    o = fr.ORIGIN.astype(np.float64)
    x = o[0] + (cells[:, 0:1] + 0.2 + 0.6 * t) * GL
    y = o[1] + (cells[:, 1:2] + 0.8 - 0.6 * t) * GL
    z = o[2] + (cells[:, 2:3] + 0.2 + 0.6 * t) * ZL
    return np.stack([x, y, z], 2).reshape(-1, 3).astype(np.float32)


def box_cells(x, y, z):
    """the cells of the box of lattice ranges x = (lo, hi), y, z, inclusive"""
    return [(ix, iy, iz) for ix in range(x[0], x[1] + 1) for iy in range(y[0], y[1] + 1) for iz in range(z[0], z[1] + 1)]


def signed(i):
    """the signed index of lattice position i: lin's inverse"""
    return i + 1 if i >= 0 else i


def floor_scan(cloud, every=3):
    """every `every`-th point of the floor's own cloud: points the map explains"""
    return np.ascontiguousarray(cloud[1::every, :3])


def off_plane(cloud, dz=0.11, every=7):
    """floor points lifted by dz: inside the floor's nodes or the level above them, far off their plane"""
    p = np.ascontiguousarray(cloud[2::every, :3]).copy()
    p[:, 2] += np.float32(dz)
    return p


def repeated(ref, mult, classes=0):
    """The answer for a batch in which base point i occurs mult[i] times, the first time at index i (tests/edge_shapes.cyclic), from the
    restatement `ref` of the base points at min_points 1: cells, labels, bounds and z are the base's, class counts and sums are sums
    over the multiplicities, in exact integers -> a dict like `ref` without the per-point arrays"""
    classes = classes or BOTH
    mult = np.asarray(mult, np.int64)
    cls, lab = ref["point_class"], ref["point_label"]
    fixed = np.rint(ref["q"].astype(np.float64) * 1024.0)
    out = ref["clusters"].copy()
    for r in out:
        idx = np.flatnonzero(lab == r["label"])
        r["off_surface"] = int(mult[idx][cls[idx] == OFF_SURFACE].sum())
        r["unmapped"] = int(mult[idx][cls[idx] == UNMAPPED].sum())
        for a, k in enumerate(("sum_x", "sum_y", "sum_z")):
            r[k] = sum(int(m) * int(v) for m, v in zip(mult[idx], fixed[idx, a]))
    novel = np.array([bool((classes >> int(c)) & 1) for c in cls])
    return dict(clusters=out, novel_points=int(mult[novel].sum()), novel_cells=ref["novel_cells"])
