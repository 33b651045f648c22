"""Plain numpy answers to the footprint poses of include/gndt.h (gndt_footprint_poses*), written from the header's definition and
nothing else: the centre through the query's restatement (tests/query_ref.py), the box of non-zero signed indices, the inside test
in fp64, the support of every column under the vehicle, the merged Gaussian summed sequentially in box order in plain fp64 (the
library folds 64 partial sums: the two differ by reordering, which tests/test_footprint_host.py bounds), numpy's eigh for the plane,
then step, bump, headroom and the verdict bits.  Shared by the CPU tier and the GPU tier.  Test infrastructure only."""
import numpy as np

from tests import query_ref as qr

NO_ROW = 0xFFFFFFFF
OK, BAD_POSE, NO_GROUND, SPARSE = 0, 1, 2, 3
TILT, STEP, COVER, LOW = 1, 2, 4, 8
CELL, COUNT = 0, 1
MAX_N = 15
FLT_MAX = np.float32(np.finfo(np.float32).max)
ROBOT = dict(radius=0.25, reachable_height=0.15, max_rough=100.0, max_angle_deg=30.0)
INFO_DTYPE = np.dtype([("status", np.int32), ("flags", np.uint32), ("centre_row", np.uint32), ("cells", np.uint16), ("support", np.uint16),
                       ("gaps", np.uint16), ("unknown", np.uint16), ("z", np.float32), ("normal", np.float32, 3), ("along", np.float32),
                       ("across", np.float32), ("rms", np.float32), ("step_max", np.float32), ("bump_max", np.float32),
                       ("headroom", np.float32), ("reserved", np.uint32)])
INTS = ("status", "flags", "centre_row", "cells", "support", "gaps", "unknown", "reserved")
FLOATS = ("z", "normal", "along", "across", "rms", "step_max", "bump_max", "headroom")
assert INFO_DTYPE.itemsize == 64


def box_n(half_length, half_width, grid_len):
    """step 3's n, from the floats widened"""
    hl, hw, g = float(np.float32(half_length)), float(np.float32(half_width)), float(np.float32(grid_len))
    return max(int(np.ceil(np.sqrt(hl * hl + hw * hw) / g)), 1)


def rule(half_length, half_width, robot=None, min_cover=0.0):
    """what the host forms once in fp64: half_length^2, half_width^2, cos(max_angle_deg), min_cover"""
    rb = dict(ROBOT)
    rb.update(robot or {})
    hl, hw = float(np.float32(half_length)), float(np.float32(half_width))
    return np.array([hl * hl, hw * hw, np.cos(float(np.float32(rb["max_angle_deg"])) * (np.pi / 180.0)), float(np.float32(min_cover))], np.float64)


def axis(c, n):
    """the 2n + 1 non-zero signed indices around c, ascending"""
    out, s = [c], c
    for _ in range(n):
        s = s - 1 if s - 1 != 0 else -1
        out.insert(0, s)
    s = c
    for _ in range(n):
        s = s + 1 if s + 1 != 0 else 1
        out.append(s)
    return out


def centre(s, o, g):
    """a column's centre on an axis, fp64"""
    return float(o) + ((s - 0.5) if s > 0 else (s + 0.5)) * float(g)


class Footprinter:
    def __init__(self, cells, origin, grid_len, z_len, robot=None):
        self.cells, self.origin = cells, np.asarray(origin, np.float32)[:3]
        self.grid_len, self.z_len = np.float32(grid_len), np.float32(z_len)
        self.robot = dict(ROBOT)
        self.robot.update(robot or {})
        n = int(cells["num_nodes"]) if "num_nodes" in cells else len(cells["sx"])
        self.sx, self.sy, self.sz = (np.asarray(cells[k])[:n].astype(np.int64) for k in ("sx", "sy", "sz"))
        self.flags = np.asarray(cells["flags"])[:n].astype(np.int64)
        self.mean = np.asarray(cells["mean"], np.float32)[:n]
        self.count = np.asarray(cells["count"])[:n].astype(np.float64)
        self.cov = np.asarray(cells["cov"], np.float32)[:n].astype(np.float64)
        self.columns = {}
        for r in range(n):
            self.columns.setdefault((int(self.sx[r]), int(self.sy[r])), []).append(r)

    def support(self, col, z0, max_dz):
        """step 5 for a column in the map -> row or None"""
        best = None
        for t in self.columns[col]:
            if not self.flags[t] & 2:
                continue
            d = np.abs(np.float32(self.mean[t, 2] - z0))
            if max_dz != 0 and not d <= max_dz:
                continue
            if best is None or d < best[0] or (d == best[0] and self.sz[t] < best[1]):
                best = (d, self.sz[t], t)
        return None if best is None else best[2]

    def footprints(self, poses, half_length, half_width, max_dz=0.0, height=0.0, min_cells=0, min_cover=0.0, weight=CELL, row_cap=0):
        """-> (info [K] INFO_DTYPE, rows [K, row_cap] uint32, close [K] bool: the two smallest eigenvalues of S lie closer than 1e-6 of
        the largest, so the plane's direction is not determined to working precision)"""
        poses = np.asarray(poses, np.float32)
        K = len(poses)
        info = np.zeros(K, INFO_DTYPE)
        info["centre_row"] = NO_ROW
        rows = np.full((K, row_cap), NO_ROW, np.uint32)
        close = np.zeros(K, bool)
        n = box_n(half_length, half_width, self.grid_len)
        assert n <= MAX_N
        len2, wid2, cos_max, cover = rule(half_length, half_width, self.robot, min_cover)
        max_dz, height = np.float32(max_dz), np.float32(height)
        reach = np.float32(self.robot["reachable_height"])
        min_cells = min_cells or 3
        ox, oy = self.origin[0], self.origin[1]
        finite = np.isfinite(poses[:, :5]).all(1) if K else np.zeros(0, bool)
        crow = qr.nearest_slope_rows(self.cells, poses[:, :3], self.origin, self.grid_len, self.z_len) if K else []
        for k in range(K):
            x, y, z, hx, hy = (float(v) for v in poses[k, :5])
            if not finite[k] or (hx == 0.0 and hy == 0.0):
                info["status"][k] = BAD_POSE
                continue
            if crow[k] == qr.NO_ROW:
                info["status"][k] = NO_GROUND
                continue
            c = int(crow[k])
            info["centre_row"][k] = c
            z0 = self.mean[c, 2]
            ax, ay = axis(int(self.sx[c]), n), axis(int(self.sy[c]), n)
            hh = hx * hx + hy * hy
            cells = gaps = unknown = 0
            sup = {}                                           # (i, j) -> row, filled in box order
            for j, sy in enumerate(ay):
                for i, sx in enumerate(ax):
                    dx, dy = centre(sx, ox, self.grid_len) - x, centre(sy, oy, self.grid_len) - y
                    u, v = dx * hx + dy * hy, dy * hx - dx * hy
                    if not ((u * u <= len2 * hh and v * v <= wid2 * hh) or (i == n and j == n)):
                        continue
                    cells += 1
                    if abs(sx) > qr.MAX_XY or abs(sy) > qr.MAX_XY or (sx, sy) not in self.columns:
                        unknown += 1
                        continue
                    r = c if (i == n and j == n) else self.support((sx, sy), z0, max_dz)
                    if r is None:
                        gaps += 1
                    else:
                        sup[(i, j)] = (r, dx, dy)
            got = [v[0] for v in sup.values()]
            rows[k, :min(len(got), row_cap)] = got[:row_cap]
            info["cells"][k], info["support"][k], info["gaps"][k], info["unknown"][k] = cells, len(got), gaps, unknown
            if len(got) < min_cells:
                info["status"][k] = SPARSE
                continue
            W, M, Q = 0.0, np.zeros(3), np.zeros((3, 3))
            at = np.array([x, y, float(z0)])
            for r, _, _ in sup.values():
                d = self.mean[r].astype(np.float64) - at
                w = self.count[r] if weight == COUNT else 1.0
                s = w / self.count[r]
                cv = self.cov[r]
                W += w
                M += w * d
                Q += np.outer(w * d, d) + s * np.array([[cv[0], cv[1], cv[2]], [cv[1], cv[3], cv[4]], [cv[2], cv[4], cv[5]]])
            dbar = M / W
            S = Q - np.outer(W * dbar, dbar)
            S = (S + S.T) / 2
            ev, vec = np.linalg.eigh(S)
            close[k] = ev[1] - ev[0] < 1e-6 * ev[2]
            lam, nrm = ev[0], vec[:, 0]
            if nrm[2] < 0:
                nrm = -nrm
            zc = float(z0) + dbar[2]

            def plane(ex, ey):
                return zc if nrm[2] == 0 else zc - (nrm[0] * (ex - dbar[0]) + nrm[1] * (ey - dbar[1])) / nrm[2]

            flags = 0
            info["rms"][k] = np.sqrt(max(lam, 0.0) / W)
            info["normal"][k] = nrm
            info["z"][k] = plane(0.0, 0.0)
            if nrm[2] != 0:
                rh = np.sqrt(hh)
                fx, fy = hx / rh, hy / rh
                info["along"][k] = -(nrm[0] * fx + nrm[1] * fy) / nrm[2]
                info["across"][k] = -(nrm[1] * fx - nrm[0] * fy) / nrm[2]
            step, bump, head = np.float32(0), 0.0, None
            for (i, j), (r, dx, dy) in sup.items():
                for nb in ((i + 1, j), (i, j + 1)):
                    if nb in sup:
                        step = max(step, np.abs(np.float32(self.mean[sup[nb][0], 2] - self.mean[r, 2])))
                bump = max(bump, abs(nrm @ (self.mean[r].astype(np.float64) - at - dbar)))
                over = np.float32(self.mean[r, 2] + reach)
                zp = plane(dx, dy)
                for t in self.columns[(int(self.sx[r]), int(self.sy[r]))]:
                    if self.flags[t] & 1 and self.mean[t, 2] > over:
                        h = float(self.mean[t, 2]) - zp
                        head = h if head is None or h < head else head
            info["step_max"][k], info["bump_max"][k] = step, bump
            info["headroom"][k] = FLT_MAX if head is None else head
            if nrm[2] < cos_max:
                flags |= TILT
            if info["step_max"][k] > reach:
                flags |= STEP
            if float(len(got)) < cover * float(cells):
                flags |= COVER
            if height > 0 and info["headroom"][k] < height:
                flags |= LOW
            info["flags"][k] = flags
        return info, rows, close


def same_ints(got_info, got_rows, want_info, want_rows, what=""):
    for f in INTS:
        assert np.array_equal(got_info[f], want_info[f]), (what, f, np.flatnonzero(got_info[f] != want_info[f])[:8], got_info[f][:8], want_info[f][:8])
    if want_rows is not None:
        assert np.array_equal(got_rows, want_rows), (what, "rows", np.argwhere(got_rows != want_rows)[:8])


def float_diffs(got, want, keep=None):
    """{field: largest |got - want|} over the poses of `keep` (all by default); FLT_MAX headrooms must agree as they are"""
    out = {}
    for f in FLOATS:
        a, b = got[f].astype(np.float64), want[f].astype(np.float64)
        if keep is not None and f in ("z", "normal", "along", "across"):
            a, b = a[keep], b[keep]
        if f == "headroom":
            none = b == float(FLT_MAX)
            assert np.array_equal(a == float(FLT_MAX), none), "headroom: FLT_MAX"
            a, b = a[~none], b[~none]
        out[f] = float(np.abs(a - b).max()) if a.size else 0.0
    return out


def same_bits(got_info, got_rows, want_info, want_rows, what=""):
    """two runs of the library's own code: every word of every record, every row"""
    a, b = got_info.view(np.uint32).reshape(len(got_info), 16), want_info.view(np.uint32).reshape(len(want_info), 16)
    assert np.array_equal(a, b), (what, np.argwhere(a != b)[:8], got_info[:2], want_info[:2])
    if want_rows is not None:
        assert np.array_equal(np.asarray(got_rows).view(np.uint32), np.asarray(want_rows).view(np.uint32)), (what, "rows")
