"""Surface patches restated from the exported rows (include/gndt.h "surface patches"): a dict of keys, a breadth-first search, the link
rule in numpy float32 with one operation a line, the plane fields in float64 with the members summed in ascending row.  Shares no code
with grid_ndt_amd/csrc/gndt_patch.hpp.  patches_fast restates the same once more without the dict and the search (sorted keys,
hooking and pointer jumping, ufunc.at) for maps of a million rows; tests/test_patch_fast_ref_host.py holds the two equal to the bit.
Also the hand-drawn scene and the clouds the patch tests draw their maps with.  Test infrastructure only."""
from collections import deque

import numpy as np

NODES, SLOPES = 0, 1
HORIZONTAL, VERTICAL, INCLINED, SLOPES_ONLY = 1, 2, 4, 8
NO_ROW = 0xFFFFFFFF
RECORD = np.dtype([("label", np.uint32), ("nodes", np.uint32), ("points", np.uint64),
                   ("sx_min", np.int32), ("sx_max", np.int32), ("sy_min", np.int32), ("sy_max", np.int32), ("sz_min", np.int32),
                   ("sz_max", np.int32), ("sum_px", np.int64), ("sum_py", np.int64), ("sum_pz", np.int64),
                   ("centroid", np.float64, 3), ("normal", np.float64, 3), ("var", np.float64), ("kind", np.uint32), ("reserved", np.uint32)])
assert RECORD.itemsize == 128
INTEGER_FIELDS = ("label", "nodes", "points", "sx_min", "sx_max", "sy_min", "sy_max", "sz_min", "sz_max", "sum_px", "sum_py", "sum_pz")
OFFSETS = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
F32 = np.float32


def lin(s):
    """the position of a signed index on a line without the hole at 0"""
    return s - 1 if s > 0 else s


def rule(candidates=NODES, connectivity=3, max_angle_deg=15.0, max_offset=0.125, max_var=0.00390625, level_deg=10.0):
    """the thresholds as the float32 the library is handed (TwoDmap.patch_params computes them the same way)"""
    return dict(candidates=candidates, connectivity=connectivity, cos_min=F32(np.cos(np.deg2rad(float(max_angle_deg)))),
                max_offset=F32(max_offset), max_var=F32(max_var), cos_level=F32(np.cos(np.deg2rad(float(level_deg)))),
                sin_level=F32(np.sin(np.deg2rad(float(level_deg)))))


def link_terms(na, nb, ma, mb):
    """(c, ea, eb) of the link rule for arrays of pairs: float32, one rounded operation a line"""
    assert all(v.dtype == F32 for v in (na, nb, ma, mb))
    p0 = na[:, 0] * nb[:, 0]
    p1 = na[:, 1] * nb[:, 1]
    p2 = na[:, 2] * nb[:, 2]
    c = p0 + p1
    c = c + p2
    dx = mb[:, 0] - ma[:, 0]
    dy = mb[:, 1] - ma[:, 1]
    dz = mb[:, 2] - ma[:, 2]
    a0 = na[:, 0] * dx
    a1 = na[:, 1] * dy
    a2 = na[:, 2] * dz
    ea = a0 + a1
    ea = ea + a2
    ea = np.abs(ea)
    b0 = nb[:, 0] * dx
    b1 = nb[:, 1] * dy
    b2 = nb[:, 2] * dz
    eb = b0 + b1
    eb = eb + b2
    eb = np.abs(eb)
    return np.abs(c), ea, eb


class Rows:
    """The exported rows as arrays"""

    def __init__(self, cells):
        n = self.n = int(cells["num_nodes"])
        self.sx, self.sy, self.sz = (np.asarray(cells[k][:n], np.int64) for k in ("sx", "sy", "sz"))
        self.flags = np.asarray(cells["flags"][:n], np.uint32)
        self.count = np.asarray(cells["count"][:n], np.uint32)
        self.rough = np.asarray(cells["rough"][:n], F32)
        self.mean = np.asarray(cells["mean"][:n], F32).reshape(n, 3)
        self.normal = np.asarray(cells["normal"][:n], F32).reshape(n, 3)
        self.cov = np.asarray(cells["cov"][:n], F32).reshape(n, 6)
        self.lin = np.stack([np.where(v > 0, v - 1, v) for v in (self.sx, self.sy, self.sz)], 1)

    def candidates(self, R, box=None):
        ok = (self.flags & 1) != 0
        if R["candidates"] == SLOPES:
            ok &= (self.flags & 2) != 0
        if box is not None:
            ok &= (self.sx >= box[0]) & (self.sx <= box[1]) & (self.sy >= box[2]) & (self.sy <= box[3])
        room = F32(R["max_var"]) * self.count.astype(F32)
        assert room.dtype == F32
        return ok & (self.rough <= room)


class Map(Rows):
    """The exported rows with their key dict"""

    def __init__(self, cells):
        super().__init__(cells)
        self.key = {tuple(int(v) for v in self.lin[r]): r for r in range(self.n)}

    def adjacent_pairs(self, cand, connectivity):
        """every adjacent pair (a, b) of candidates with a < b"""
        A, B = [], []
        for a in np.flatnonzero(cand):
            x, y, z = (int(v) for v in self.lin[a])
            for dx, dy, dz in OFFSETS:
                if (dx != 0) + (dy != 0) + (dz != 0) > connectivity:
                    continue
                b = self.key.get((x + dx, y + dy, z + dz))
                if b is not None and b > a and cand[b]:
                    A.append(a)
                    B.append(b)
        return np.asarray(A, np.int64), np.asarray(B, np.int64)

    def links(self, R, A, B):
        """-> (linked [pairs], passes the angle, passes the offset); the rule is asserted symmetric to the bit"""
        if not len(A):
            z = np.zeros(0, bool)
            return z, z, z
        c, ea, eb = link_terms(self.normal[A], self.normal[B], self.mean[A], self.mean[B])
        c2, eb2, ea2 = link_terms(self.normal[B], self.normal[A], self.mean[B], self.mean[A])
        for u, v in ((c, c2), (ea, ea2), (eb, eb2)):
            assert u.dtype == F32 and u.tobytes() == v.tobytes(), "the link rule is not symmetric to the bit"
        angle = c >= R["cos_min"]
        offset = (ea <= R["max_offset"]) & (eb <= R["max_offset"])
        return angle & offset, angle, offset

    def patches(self, R, box=None):
        """-> dict(label [n] uint32, patches: RECORD array of EVERY patch in ascending label, rows: the candidates, pairs: (A, B,
        linked, angle, offset) of the adjacent candidate pairs, cand, posed: well_posed's answer for every patch)"""
        n = self.n
        conn = int(R["connectivity"]) or 3
        cand = self.candidates(R, box)
        A, B = self.adjacent_pairs(cand, conn)
        linked, angle, offset = self.links(R, A, B)
        nbrs = [[] for _ in range(n)]
        for a, b in zip(A[linked].tolist(), B[linked].tolist()):
            nbrs[a].append(b)
            nbrs[b].append(a)
        label = np.full(n, NO_ROW, np.uint32)
        recs, posed = [], []
        for r0 in np.flatnonzero(cand).tolist():            # ascending: a component is found from its smallest row
            if label[r0] != NO_ROW:
                continue
            members, queue = [], deque([r0])
            label[r0] = r0
            while queue:
                a = queue.popleft()
                members.append(a)
                for t in nbrs[a]:
                    if label[t] == NO_ROW:
                        label[t] = r0
                        queue.append(t)
            recs.append(self.record(R, r0, sorted(members)))
            posed.append(self.last_posed())
        records = np.zeros(len(recs), RECORD)
        for i, rec in enumerate(recs):
            records[i] = rec
        return dict(label=label, patches=records, rows=int(cand.sum()), pairs=(A, B, linked, angle, offset), cand=cand, posed=posed)

    def last_posed(self):
        """of the patch record() saw last: (well posed, spread) — see well_posed"""
        w = self.last_eigenvalues
        return bool(w[0] > 0.0 and w[1] >= 100.0 * w[0]), self.last_spread

    def record(self, R, r0, members):
        rec = np.zeros((), RECORD)
        m = np.asarray(members, np.int64)
        rec["label"], rec["nodes"], rec["points"] = r0, len(m), int(self.count[m].astype(np.int64).sum())
        for k, v in (("sx", self.sx), ("sy", self.sy), ("sz", self.sz)):
            rec[k + "_min"], rec[k + "_max"] = v[m].min(), v[m].max()
        rec["sum_px"], rec["sum_py"], rec["sum_pz"] = (int(self.lin[m, a].sum()) for a in range(3))
        # the members merged as Gaussians about the label row's mean, in ascending row
        ref = self.mean[r0].astype(np.float64)
        N, S1, S2 = 0.0, np.zeros(3), np.zeros((3, 3))
        for r in members:
            cnt = float(self.count[r])
            d = self.mean[r].astype(np.float64) - ref
            cv = self.cov[r].astype(np.float64)
            scatter = np.array([[cv[0], cv[1], cv[2]], [cv[1], cv[3], cv[4]], [cv[2], cv[4], cv[5]]])
            N += cnt
            S1 += cnt * d
            S2 += scatter + cnt * np.outer(d, d)
        Cm = S2 - np.outer(S1, S1) / N
        w, v = np.linalg.eigh(Cm)
        nrm = v[:, 0] / np.linalg.norm(v[:, 0])
        for a in (2, 1, 0):
            if nrm[a] != 0.0:
                if nrm[a] < 0.0:
                    nrm = -nrm
                break
        w[0] = least_eigenvalue(Cm, w[0])
        rec["centroid"], rec["normal"], rec["var"] = ref + S1 / N, nrm, max(w[0], 0.0) / N
        az = abs(nrm[2])
        kind = HORIZONTAL if az >= float(R["cos_level"]) else VERTICAL if az <= float(R["sin_level"]) else INCLINED
        if all(int(self.flags[r]) & 2 for r in members):
            kind |= SLOPES_ONLY
        rec["kind"] = kind
        self.last_eigenvalues, self.last_spread = w, float(np.trace(S2)) / N
        return rec


def least_eigenvalue(Cm, x0):
    """eigh's least eigenvalue of the symmetric 3 x 3 Cm polished by Newton steps on det(Cm - x I) in long double: eigh leaves it with
    an absolute error of a few ulps of the LARGEST eigenvalue, which on a flat patch (a ratio of 10^5 and more) is 1e-10 of the least and
    would be taken for the library's deviation"""
    L = np.longdouble
    a, b, c, d, e, f = (L(Cm[0, 0]), L(Cm[0, 1]), L(Cm[0, 2]), L(Cm[1, 1]), L(Cm[1, 2]), L(Cm[2, 2]))
    x = L(x0)
    for _ in range(4):
        A, D, F = a - x, d - x, f - x
        p = A * (D * F - e * e) - b * (b * F - e * c) + c * (b * e - D * c)
        dp = -((D * F - e * e) + (A * F - c * c) + (A * D - b * b))
        if dp == 0:
            break
        x = x - p / dp
    return float(x)


def least_eigenvalues(C6, x0):
    """least_eigenvalue for arrays: C6 [P, 6] = (xx, xy, xz, yy, yz, zz), x0 [P] -> [P] float64; the same long-double operations in
    the same order, an element whose derivative vanishes stays where it is from then on"""
    L = np.longdouble
    a, b, c, d, e, f = (C6[:, k].astype(L) for k in range(6))
    x = np.asarray(x0).astype(L)
    live = np.ones(len(x), bool)
    for _ in range(4):
        A, D, F = a - x, d - x, f - x
        p = A * (D * F - e * e) - b * (b * F - e * c) + c * (b * e - D * c)
        dp = -((D * F - e * e) + (A * F - c * c) + (A * D - b * b))
        live &= dp != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.where(live, x - p / dp, x)
    return x.astype(np.float64)


KEY_BITS, KEY_BIAS = 21, 1 << 20       # a linear index of +-65 536 and a level of the codec's range fit 21 bits with room for +-1


def patches_fast(cells, R, box=None):
    """Map.patches without the key dict and the search, for maps of a million rows: sorted 64-bit keys and searchsorted for the
    neighbours, link_terms on the pairs, components by hooking the larger root under the smaller and pointer jumping, the fields by
    ufunc.at in ascending row, one batched eigh.  cells: an export, or the Rows of one.  -> dict(label, patches: RECORD array of EVERY
    patch in ascending label, rows, cand, eigenvalues [P, 3] (the least one polished), spread [P]: tr(S2) / N — what well_posed_fast
    reads)"""
    m = cells if isinstance(cells, Rows) else Rows(cells)
    n = m.n
    conn = int(R["connectivity"]) or 3
    cand = m.candidates(R, box)
    rows = np.flatnonzero(cand)
    assert n == 0 or (np.abs(m.lin).max() < KEY_BIAS - 1)
    key = ((m.lin[rows, 0] + KEY_BIAS) << (2 * KEY_BITS)) | ((m.lin[rows, 1] + KEY_BIAS) << KEY_BITS) | (m.lin[rows, 2] + KEY_BIAS)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    assert (ks[1:] != ks[:-1]).all(), "two rows of one key"
    A, B = [], []
    for dx, dy, dz in OFFSETS:
        if (dx != 0) + (dy != 0) + (dz != 0) > conn or not len(rows):
            continue
        want = key + ((dx << (2 * KEY_BITS)) + (dy << KEY_BITS) + dz)
        pos = np.minimum(np.searchsorted(ks, want), len(ks) - 1)
        b = rows[order[pos]]
        hit = (ks[pos] == want) & (b > rows)
        a, b = rows[hit], b[hit]
        c, ea, eb = link_terms(m.normal[a], m.normal[b], m.mean[a], m.mean[b])
        linked = (c >= R["cos_min"]) & (ea <= R["max_offset"]) & (eb <= R["max_offset"])
        A.append(a[linked])
        B.append(b[linked])
    A, B = (np.concatenate(v) if v else np.zeros(0, np.int64) for v in (A, B))
    # components: parent[x] <= x throughout, flat before every hooking, so what is hooked is a root and the root is the smallest row
    parent = np.arange(n, dtype=np.int64)
    rounds = 0
    while len(A):
        pa, pb = parent[A], parent[B]
        apart = pa != pb
        if not apart.any():
            break
        A, B, pa, pb = A[apart], B[apart], pa[apart], pb[apart]
        np.minimum.at(parent, np.maximum(pa, pb), np.minimum(pa, pb))
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
        rounds += 1
    label = np.where(cand, parent, NO_ROW).astype(np.uint32)
    roots = rows[parent[rows] == rows]
    at = np.searchsorted(roots, parent[rows])                      # the patch of every candidate, candidates in ascending row
    P_ = len(roots)
    rec = np.zeros(P_, RECORD)
    rec["label"] = roots
    rec["nodes"] = np.bincount(at, minlength=P_)
    i64 = lambda fill=0: np.full(P_, fill, np.int64)
    points = i64()
    np.add.at(points, at, m.count[rows].astype(np.int64))
    rec["points"] = points
    for k, v in (("sx", m.sx), ("sy", m.sy), ("sz", m.sz)):
        lo, hi = i64(np.iinfo(np.int64).max), i64(np.iinfo(np.int64).min)
        np.minimum.at(lo, at, v[rows])
        np.maximum.at(hi, at, v[rows])
        rec[k + "_min"], rec[k + "_max"] = lo, hi
    for axis, k in enumerate(("sum_px", "sum_py", "sum_pz")):
        tot = i64()
        np.add.at(tot, at, m.lin[rows, axis])
        rec[k] = tot
    slopes = i64()
    np.add.at(slopes, at, ((m.flags[rows] & 2) != 0).astype(np.int64))
    # the ten sums about the label row's mean: Map.record's terms, added in ascending row
    ref = m.mean[roots].astype(np.float64)
    cnt = m.count[rows].astype(np.float64)
    d = m.mean[rows].astype(np.float64) - ref[at]
    cv = m.cov[rows].astype(np.float64)
    N, S1, S2 = np.zeros(P_), np.zeros((P_, 3)), np.zeros((P_, 6))
    np.add.at(N, at, cnt)
    for j in range(3):
        np.add.at(S1[:, j], at, cnt * d[:, j])
    for j, (u, v) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        np.add.at(S2[:, j], at, cv[:, j] + cnt * (d[:, u] * d[:, v]))
    C6 = np.stack([S2[:, j] - (S1[:, u] * S1[:, v]) / N for j, (u, v) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)))], 1)
    Cm = C6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(P_, 3, 3)
    w, v = np.linalg.eigh(Cm) if P_ else (np.zeros((0, 3)), np.zeros((0, 3, 3)))
    v0 = v[:, :, 0]
    nrm = v0 / np.array([np.linalg.norm(x) for x in v0]).reshape(P_, 1)      # (norm's own dot product, vector by vector: the same bits)
    # the sign: the last non-zero component among z, y, x is positive
    lead = np.where(nrm[:, 2] != 0.0, nrm[:, 2], np.where(nrm[:, 1] != 0.0, nrm[:, 1], nrm[:, 0]))
    nrm = np.where((lead < 0.0)[:, None], -nrm, nrm)
    w = w.copy()
    w[:, 0] = least_eigenvalues(C6, w[:, 0])
    rec["centroid"], rec["normal"], rec["var"] = ref + S1 / N[:, None], nrm, np.maximum(w[:, 0], 0.0) / N
    az = np.abs(nrm[:, 2])
    kind = np.where(az >= float(R["cos_level"]), HORIZONTAL, np.where(az <= float(R["sin_level"]), VERTICAL, INCLINED))
    rec["kind"] = kind | np.where(slopes == rec["nodes"], SLOPES_ONLY, 0)
    spread = ((S2[:, 0] + S2[:, 3]) + S2[:, 5]) / N
    return dict(label=label, patches=rec, rows=len(rows), cand=cand, eigenvalues=w, spread=spread, rounds=rounds)


def well_posed_fast(ref, want):
    """well_posed for the records `want` (any of ref's patches) from what patches_fast kept -> (posed [len(want)] bool, spread)"""
    at = np.searchsorted(ref["patches"]["label"], want["label"])
    assert np.array_equal(ref["patches"]["label"][at], want["label"])
    w = ref["eigenvalues"][at]
    return (w[:, 0] > 0.0) & (w[:, 1] >= 100.0 * w[:, 0]), ref["spread"][at]


def listed(ref, min_size=1):
    """the patches of `ref` the call lists, and its four counts"""
    keep = ref["patches"][ref["patches"]["nodes"] >= max(int(min_size), 1)]
    return keep, np.array([len(keep), ref["rows"], len(ref["patches"]), 0], np.uint32)


def same_integers(got, want):
    """every integer field and kind's SLOPES_ONLY bit, for equality"""
    return got.shape == want.shape and all(np.array_equal(got[k], want[k]) for k in INTEGER_FIELDS) and \
        np.array_equal(got["kind"] & SLOPES_ONLY, want["kind"] & SLOPES_ONLY) and (got["reserved"] == 0).all()


def diff_integers(got, want):
    if got.shape != want.shape:
        return f"{got.shape[0]} records, want {want.shape[0]}"
    for k in INTEGER_FIELDS + ("kind",):
        bad = np.flatnonzero(got[k] != want[k])
        if len(bad):
            return f"{k}: records {bad[:5]} got {got[k][bad[:5]]} want {want[k][bad[:5]]}"
    return ""


PLANE_ABS = 1e-10       # centroid (m) and normal (component-wise, after orientation): the footprints' bound
VAR_REL = 1e-10         # var: times its value


def plane_deviation(got, want, var_slack=None):
    """-> (worst |centroid| deviation, worst |normal| deviation, worst var deviation — what exceeds var_slack, where given — over var)
    over the records"""
    if not len(want):
        return 0.0, 0.0, 0.0
    dc = float(np.abs(got["centroid"] - want["centroid"]).max())
    dn = float(np.abs(got["normal"] - want["normal"]).max())
    excess = np.maximum(np.abs(got["var"] - want["var"]) - (0.0 if var_slack is None else var_slack), 0.0)
    dv = float((excess / np.maximum(want["var"], 1e-300)).max())
    return dc, dn, dv


def well_posed(m, R, ref, rec):
    """-> (the two larger eigenvalues of the patch's C are at least 100 x the least, and the least is positive: the record's plane is
    compared with the restatement's only then; the patch's mean squared distance from its label row's mean, tr(S2) / N)"""
    members = np.flatnonzero(ref["label"] == rec["label"]).tolist()
    m.record(R, int(rec["label"]), members)
    return m.last_posed()


def planes_agree(m, R, ref, got, want, what="", spread_slack=False):
    """the plane fields of the well-posed records within the bounds, kind's orientation bits equal there -> how many were compared;
    prints the worst deviations before it asserts.  spread_slack (maps that were not drawn for this comparison: the oracle's, where a
    synthetic ground is flat to the last bit over tens of metres): var may first deviate by (2 nodes + 8) 2^-53 tr(S2) / N —
    C = S2 - S1 S1^T / N cancels the patch's spread about its label row, so each of the `nodes` roundings of either side's sums, up to
    2^-53 tr(S2) a term, can land on the least eigenvalue whole, and a backward-stable solver answers for a matrix a few (8) ulps of
    the LARGEST eigenvalue (<= tr(S2)) away; a patch far thinner than its spread holds no ten digits of var in fp64, whoever sums it."""
    if "eigenvalues" in ref:                 # patches_fast's answer: m may be None
        keep, spread = well_posed_fast(ref, want)
    else:
        posed = [well_posed(m, R, ref, rec) for rec in want]
        keep, spread = np.array([p[0] for p in posed], bool), np.array([p[1] for p in posed], np.float64)
    g, w = got[keep], want[keep]
    slack = (2.0 * w["nodes"] + 8.0) * 2.0 ** -53 * spread[keep] if spread_slack else None
    dc, dn, dv = plane_deviation(g, w, slack)
    print(f"patch planes {what}: {int(keep.sum())} of {len(want)} compared, centroid {dc:.3e} m, normal {dn:.3e}, var rel {dv:.3e}")
    ref["deviation"] = (dc, dn, dv)
    assert dc <= PLANE_ABS and dn <= PLANE_ABS and dv <= VAR_REL, (what, dc, dn, dv)
    assert np.array_equal(g["kind"], w["kind"]), (what, g["kind"], w["kind"])
    return int(keep.sum())


# ---- clouds -----------------------------------------------------------------------------------------------------------------------
GL, ZL, IV = 0.5, 0.25, 0.08
P = dict(grid_len=GL, z_len=ZL, slope_interval=IV, demand="slope")
# demand "true": every node with statistics is a slope and carries a normal.  Under "slope" a node below another one of its column has
# none (normal 0, rough 0): a candidate under NODES that links to nothing, so a wall would be a stack of single nodes.
P_HAND = dict(P, demand="true")
ORIGIN = np.float32([0.0, 0.0, 0.0])
Z_FLOOR = 0.11           # inside level lin 0; a storey k levels higher: Z_FLOOR + k * ZL
FLAT3 = (0.12, 0.25, 0.38)
FINE5 = (0.05, 0.15, 0.25, 0.35, 0.45)


def ripple(u, v):
    return 0.002 * np.sin(7 * u) * np.cos(5 * v)


def flat_cell(ix, iy, z, gx=0.0, gy=0.0, at=FLAT3):
    """points of cell (ix, iy) on the plane z + gx (x - x0) + gy (y - y0) about the cell's corner, with the frontiers' ripple"""
    return [[ix * GL + a, iy * GL + b, z + gx * a + gy * b + ripple(ix * GL + a, iy * GL + b)] for a in at for b in at]


def wall_node(ix, iy, level, x_in=0.25):
    """points of the node of column (ix, iy) at level lin `level` on the vertical plane x = ix GL + x_in"""
    return [[ix * GL + x_in + ripple(iy * GL + b, level * ZL + c), iy * GL + b, level * ZL + c] for b in FLAT3 for c in (0.06, 0.125, 0.19)]


def rough_cell(ix, iy, z_mid):
    """a node whose least eigenvalue is about 0.008 m^2 a point, along z: z alternates by 0.09 m about z_mid over the 3 x 3 points"""
    return [[ix * GL + a, iy * GL + b, z_mid + (0.09 if (i + j) % 2 == 0 else -0.09)] for i, a in enumerate(FLAT3) for j, b in enumerate(FLAT3)]


def cloud_of(points):
    return np.ascontiguousarray(np.float32([ORIGIN] + list(points)))


FLOOR_N, WALL_H, DECK = 8, 4, (1, 4)
ROUGH_CELL, BARE_CELL = (6, 5), (7, 0)


def hand_scene():
    """-> (cloud, groups): a floor of 8 x 8 cells at level 0 with a rough node at (6, 5) and a node of two points at (7, 0); a wall of
    four levels on the columns ix = 8; a ramp of gradient 0.5 (26.6 degrees) over the columns ix = -1, -2, two levels high and two nodes
    a column; a deck of 3 x 3 cells one level above the floor.  groups: {name: [(lin x, lin y, lin z) of its nodes]} — the answer under
    NODES and the default thresholds is one patch a group, written out here by hand:
      floor   62 nodes: the rough node is no candidate (its neighbours link round it), the node of two points has no statistics
      wall    32 nodes: perpendicular to the floor it meets (the angle refuses)
      ramp    32 nodes: 26.6 degrees from the floor it meets (the angle refuses)
      deck     9 nodes: parallel to the floor one level below (the angle passes), 0.25 m off its plane (the offset refuses)"""
    pts, groups = [], dict(floor=[], wall=[], ramp=[], deck=[], rough=[], bare=[])
    for ix in range(FLOOR_N):
        for iy in range(FLOOR_N):
            if (ix, iy) == ROUGH_CELL:
                pts += rough_cell(ix, iy, 0.125)
                groups["rough"].append((ix, iy, 0))
            elif (ix, iy) == BARE_CELL:
                pts += flat_cell(ix, iy, Z_FLOOR)[:2]
                groups["bare"].append((ix, iy, 0))
            else:
                pts += flat_cell(ix, iy, Z_FLOOR)
                groups["floor"].append((ix, iy, 0))
    for iy in range(FLOOR_N):
        for level in range(WALL_H):
            pts += wall_node(FLOOR_N, iy, level)
            groups["wall"].append((FLOOR_N, iy, level))
    for ix, levels in ((-1, (0, 1)), (-2, (1, 2))):
        for iy in range(FLOOR_N):
            # z = Z_FLOOR - 0.5 x: the cell's corner is at x = ix GL, where the ramp stands at Z_FLOOR - 0.5 ix GL
            pts += flat_cell(ix, iy, Z_FLOOR - 0.5 * ix * GL, gx=-0.5, at=FINE5)
            groups["ramp"] += [(ix, iy, lv) for lv in levels]
    for ix in range(*DECK):
        for iy in range(*DECK):
            pts += flat_cell(ix, iy, Z_FLOOR + ZL)
            groups["deck"].append((ix, iy, 1))
    return cloud_of(pts), groups


def hand_labels(m, groups):
    """the labels the hand scene's groups give on the rows of Map m: a patch's label is its smallest member row"""
    label = np.full(m.n, NO_ROW, np.uint32)
    for name in ("floor", "wall", "ramp", "deck"):
        rows = [m.key[k] for k in groups[name]]
        label[rows] = min(rows)
    assert sum(len(v) for v in groups.values()) == m.n
    return label


def spiral(turns=44):
    """-> the (ix, iy) cells of a one-cell-wide square spiral from the origin outwards, a free cell between its arms: one chain of about
    4 k cells (turns 44: 3 961), the union-find's long path"""
    cells, x, y = [(0, 0)], 0, 0
    dirs = ((1, 0), (0, 1), (-1, 0), (0, -1))
    for k in range(2 * turns):
        dx, dy = dirs[k % 4]
        for _ in range(2 * (k // 2 + 1)):
            x, y = x + dx, y + dy
            cells.append((x, y))
    return cells


def flat_cloud(cells, seed=None):
    """flat cells at the floor's height, in a shuffled order with a seed: row order follows first sight"""
    cells = list(cells)
    if seed is not None:
        cells = [cells[i] for i in np.random.default_rng(seed).permutation(len(cells))]
    return cloud_of(p for ix, iy in cells for p in flat_cell(ix, iy, Z_FLOOR))


CHECKER_N = 12


def checkerboard(n=CHECKER_N):
    """n x n cells tilted by +-0.2 along x about their own corner, alternating like a chessboard: 6-neighbours are 22.6 degrees apart
    (the angle refuses: every node its own patch), diagonal neighbours parallel and 0.098 m off each other's plane (below the default
    0.125: the two colours are two patches under 18 and 26)"""
    return cloud_of(p for ix in range(n) for iy in range(n)
                    for p in flat_cell(ix, iy, Z_FLOOR if (ix + iy) % 2 == 0 else Z_FLOOR + 0.076, gx=0.2 if (ix + iy) % 2 == 0 else -0.2))


def two_storeys():
    """-> (cloud, nodes a group): a floor of 8 x 8 cells at level 0, a deck of 4 x 8 cells four levels up from ix = 12 on, and between them
    a stair two cells wide of gradient 0.5 over the columns ix = 8 .. 11, two nodes a column (build with P_HAND)"""
    pts = [p for ix in range(8) for iy in range(8) for p in flat_cell(ix, iy, Z_FLOOR)]
    pts += [p for ix in range(8, 12) for iy in (2, 3) for p in flat_cell(ix, iy, Z_FLOOR + 0.5 * (ix - 8) * GL, gx=0.5, at=FINE5)]
    pts += [p for ix in range(12, 16) for iy in range(8) for p in flat_cell(ix, iy, Z_FLOOR + 4 * ZL)]
    return cloud_of(pts), dict(floor=64, stair=16, deck=32)


def u_shape():
    """two arms of six cells on ix = 0 and ix = 4 joined by a base along iy = 0: one patch, two when a box leaves the base out"""
    cells = [(ix, 0) for ix in range(5)] + [(ix, iy) for ix in (0, 4) for iy in range(1, 6)]
    return flat_cloud(cells)
