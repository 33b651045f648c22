"""CPU tier: the surface patches' per-row code (grid_ndt_amd/csrc/gndt_patch.hpp: the candidate test, the link rule, the union-find over
13 of the 26 neighbour keys, the integer reduction, the moment match and the plane fit), compiled with g++ into tests/_patch_shim.so
and run one row after another, against the restatement from the rows (tests/patch_ref.py: a key dict, a breadth-first search, the link
rule in numpy float32) — on a hand-drawn scene whose labels are written out, on maps the oracle builds and on 200 random lattices:
every label, every integer field, every count for equality; the plane fields of the well-posed patches within the footprints' bound;
parent[x] <= x after every union; and the product entry points refuse to run without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import patch_ref as pr
from tests.host_emulation import MAP, HostMap, MapRows, load_shim

_shim = None


def shim():
    global _shim
    if _shim is None:
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        _shim = load_shim("patch_shim.cpp", "_patch_shim.so", {
            "pshim_links": ([vp, vp, MAP, vp, vp, u64, vp], None),
            "pshim_patches": ([vp, vp, u32, vp, MAP, vp, vp, u32, vp], C.c_int64),
        })
    return _shim


def _rule_args(R, box):
    ints = np.array([R["candidates"], int(R["connectivity"]) or 3, int(box is not None)] + list(box if box is not None else (0, 0, 0, 0)), np.int32)
    floats = np.array([R[k] for k in ("cos_min", "max_offset", "max_var", "cos_level", "sin_level")], np.float32)
    return ints, floats


def run(m, R, box=None, min_size=1, order=None, cap=None):
    """the passes on map m (a HostMap or a Lattice) -> dict(label, patches [min(listed, cap)], counts, tail)"""
    n = m.n
    ints, floats = _rule_args(R, box)
    cap = n if cap is None else cap
    label = np.full(max(n, 1), 0xDEADBEEF, np.uint32)
    patches = np.full(max(cap, 1) * 32, 0xA5A5A5A5, np.uint32).view(pr.RECORD)
    counts = np.full(4, 0xDEADBEEF, np.uint32)
    o = None if order is None else np.ascontiguousarray(order, np.uint32)
    rc = shim().pshim_patches(ints.ctypes.data, floats.ctypes.data, max(min_size, 1), None if o is None else o.ctypes.data, m.shim_map(),
                              label.ctypes.data, patches.ctypes.data, cap, counts.ctypes.data)
    assert rc == 0, f"parent[x] <= x failed at row {rc - 1}"
    k = min(int(counts[0]), cap)
    return dict(label=label[:n], patches=patches[:k], counts=counts, tail=patches[k:])


def check(m, ref_map, R, box=None, min_size=1, order=None, what="", planes=True, spread_slack=False):
    got = run(m, R, box, min_size, order)
    ref = ref_map.patches(R, box)
    recs, counts = pr.listed(ref, min_size)
    assert np.array_equal(got["counts"], counts), (what, got["counts"], counts)
    assert np.array_equal(got["label"], ref["label"]), what
    assert pr.same_integers(got["patches"], recs), (what, pr.diff_integers(got["patches"], recs))
    if planes:
        ref["compared"] = pr.planes_agree(ref_map, R, ref, got["patches"], recs, what, spread_slack)
    return got, ref


def links_both_ways(m, ref_map, R, ref, what=""):
    """the header's link rule over every adjacent candidate pair, in both orders, against the restatement's"""
    A, B, linked, _, _ = ref["pairs"]
    if not len(A):
        return
    ints, floats = _rule_args(R, None)
    a, b = np.ascontiguousarray(A, np.uint32), np.ascontiguousarray(B, np.uint32)
    for x, y in ((a, b), (b, a)):
        out = np.full(len(a), 7, np.uint8)
        shim().pshim_links(ints.ctypes.data, floats.ctypes.data, m.shim_map(), x.ctypes.data, y.ctypes.data, len(a), out.ctypes.data)
        assert np.array_equal(out.astype(bool), linked), what


# ---- the hand scene ------------------------------------------------------------------------------------------------------------------

_hand = []


def hand():
    if not _hand:
        cloud, groups = pr.hand_scene()
        m = HostMap(cloud, pr.P_HAND)
        _hand.append((m, pr.Map(m.cells), groups))
    return _hand[0]


def test_the_hand_scene_has_the_labels_written_out():
    m, ref_map, groups = hand()
    assert m.n == 64 + 32 + 32 + 9
    want = pr.hand_labels(ref_map, groups)
    R = pr.rule()
    got, ref = check(m, ref_map, R, what="hand")
    assert np.array_equal(got["label"], want)
    rec = got["patches"]
    floor, deck, wall, ramp = (int(want[ref_map.key[groups[k][0]]]) for k in ("floor", "deck", "wall", "ramp"))
    assert sorted(rec["label"].tolist()) == sorted([floor, deck, wall, ramp]) and tuple(got["counts"]) == (4, 135, 4, 0)
    by = {int(r["label"]): r for r in rec}
    assert [int(by[k]["nodes"]) for k in (floor, deck, wall, ramp)] == [62, 9, 32, 32]
    assert [int(by[k]["kind"]) & 7 for k in (floor, deck, wall, ramp)] == [pr.HORIZONTAL, pr.HORIZONTAL, pr.VERTICAL, pr.INCLINED]
    # the rough node and the node of two points are no candidates; the floor's bounds reach round them
    for k in ("rough", "bare"):
        assert want[ref_map.key[groups[k][0]]] == pr.NO_ROW
    f = by[floor]
    assert (int(f["sx_min"]), int(f["sx_max"]), int(f["sy_min"]), int(f["sy_max"]), int(f["sz_min"]), int(f["sz_max"])) == (1, 8, 1, 8, 1, 1)
    w = by[wall]
    assert (int(w["sx_min"]), int(w["sx_max"]), int(w["sz_min"]), int(w["sz_max"])) == (9, 9, 1, 4) and int(w["sum_pz"]) == 8 * (0 + 1 + 2 + 3)
    r = by[ramp]
    assert (int(r["sx_min"]), int(r["sx_max"]), int(r["sz_min"]), int(r["sz_max"])) == (-2, -1, 1, 3) and int(r["sum_px"]) == -16 - 32
    # the ramp's plane: gradient 0.5 along -x; the deck a quarter of a metre above the floor
    assert abs(r["normal"][0] / r["normal"][2] - 0.5) < 1e-3 and abs(by[deck]["centroid"][2] - f["centroid"][2] - 0.25) < 1e-3
    assert ref["compared"] == 4
    # what refuses: the angle between floor and wall / ramp, the offset between floor and deck
    A, B, linked, angle, offset = ref["pairs"]
    assert (~angle).sum() > 0 and (angle & ~offset).sum() > 0
    links_both_ways(m, ref_map, R, ref, "hand")


def test_the_hand_scene_under_every_connectivity_order_and_list_length():
    m, ref_map, groups = hand()
    for conn in (1, 2, 3, 0):
        for cand in (pr.NODES, pr.SLOPES):
            got, _ = check(m, ref_map, pr.rule(cand, conn), what=("hand", conn, cand))
            assert tuple(got["counts"]) == (4, 135, 4, 0)
    R = pr.rule()
    first = run(m, R)
    rng = np.random.default_rng(5)
    for order in (np.arange(m.n)[::-1], rng.permutation(m.n), rng.permutation(m.n)):
        got = run(m, R, order=order)
        assert got["label"].tobytes() == first["label"].tobytes() and np.array_equal(got["counts"], first["counts"])
        assert pr.same_integers(got["patches"], first["patches"])
    for cap in (0, 1, 3, 4, 7):
        got = run(m, R, cap=cap)
        assert np.array_equal(got["counts"], first["counts"]) and pr.same_integers(got["patches"], first["patches"][:cap])
        assert (got["tail"].view(np.uint32) == 0xA5A5A5A5).all()
    for ms in (0, 2, 10, 33, 63):
        got, _ = check(m, ref_map, R, min_size=ms, what=("min_size", ms))
        assert np.array_equal(got["label"], first["label"]) and got["counts"][2] == 4
    # a box through the floor's middle cuts it in two; the wall and the ramp lie outside
    got, _ = check(m, ref_map, R, box=(1, 8, 1, 8), what="floor and deck only")
    assert tuple(got["counts"]) == (2, 71, 2, 0)
    # tighter thresholds: an offset below the ripple leaves single nodes, an angle of 30 degrees joins the ramp to the floor
    check(m, ref_map, pr.rule(max_offset=1e-4), what="tight offset")
    got, _ = check(m, ref_map, pr.rule(max_angle_deg=30.0), what="wide angle")
    assert got["counts"][0] == 3
    got, _ = check(m, ref_map, pr.rule(max_var=0.02), what="the rough node joins")
    assert got["counts"][1] == 136 and int(got["patches"]["nodes"][0]) == 63


# ---- oracle-built maps ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bridge_ground", "site_two_storey"])
def test_oracle_maps_both_candidate_modes_all_connectivities(name):
    from tests.test_frontier_host import _map
    m, _ = _map(name)
    ref_map = pr.Map(m.cells)
    zl = m.P["z_len"]
    some = 0
    for cand in (pr.NODES, pr.SLOPES):
        for conn in (1, 2, 3):
            R = pr.rule(cand, conn, max_offset=0.5 * zl, max_var=(0.25 * zl) ** 2)
            got, ref = check(m, ref_map, R, what=(name, cand, conn), planes=conn == 3, spread_slack=True)
            some += int((got["patches"]["nodes"] >= 2).sum())
            if conn == 3:
                links_both_ways(m, ref_map, R, ref, (name, cand))
    assert some > 0
    x0, x1, y0, y1 = m.box()
    check(m, ref_map, pr.rule(pr.SLOPES, 3, max_offset=0.5 * zl, max_var=(0.25 * zl) ** 2), box=(x0, (x0 + x1) // 2 or 1, y0, y1), min_size=3,
          order=np.random.default_rng(3).permutation(m.n), what=(name, "box"), planes=False)


# ---- random lattices ---------------------------------------------------------------------------------------------------------------

def random_unit(rng, k, lo_deg, hi_deg):
    """k unit vectors lo_deg .. hi_deg from +z, at random azimuths"""
    t, a = np.deg2rad(rng.uniform(lo_deg, hi_deg, k)), rng.uniform(0.0, 2.0 * np.pi, k)
    return np.stack([np.sin(t) * np.cos(a), np.sin(t) * np.sin(a), np.cos(t)], 1)


class Lattice(MapRows):
    """side x side columns across the origin in a shuffled order, one to three levels each out of four neighbouring ones, random unit
    normals anywhere on the sphere — a third of the rows within 4 degrees of one shared, nearly upright normal, their means on its plane
    through their cell's centre, so that patches form, the stacked ones among them a level apart (the offset refuses) — counts of 3 to 40,
    roughness on both sides of max_var x count, random scatters, a few rows without statistics or without a slope.  No cloud, no build."""

    def __init__(self, rng, side=10):
        fill = rng.uniform(0.6, 0.95)
        cols = [(ix, iy) for ix in range(-side // 2, side // 2) for iy in range(-side // 2, side // 2) if rng.random() < fill]
        cols = [cols[i] for i in rng.permutation(len(cols))]
        pool = np.array([-2, -1, 1, 2])
        sx, sy, sz, ncol = [], [], [], []
        for ix, iy in cols:
            zs = rng.choice(pool, size=rng.choice([1, 1, 1, 2, 2, 3]), replace=False)
            if rng.random() < 0.8 and 1 not in zs:           # most columns share a ground level
                zs[rng.integers(0, len(zs))] = 1
            for j, z in enumerate(zs):
                sx.append(ix + 1 if ix >= 0 else ix); sy.append(iy + 1 if iy >= 0 else iy); sz.append(int(z))
                ncol.append(len(zs) if j == 0 else 0)
        n = len(sx)
        lin = np.stack([np.where(np.array(v) > 0, np.array(v) - 1, np.array(v)) for v in (sx, sy, sz)], 1)
        centre = (lin + 0.5) * np.array([0.5, 0.5, 0.25])
        shared = random_unit(rng, 1, 2.0, 9.0)[0]
        near = rng.random(n) < 1.0 / 3.0
        normal = random_unit(rng, n, 0.0, 180.0)
        tilt = random_unit(rng, n, 0.0, 4.0)
        normal[near] = shared + (tilt[near] - np.array([0.0, 0.0, 1.0]))
        normal /= np.linalg.norm(normal, axis=1, keepdims=True)
        mean = centre + rng.uniform(-0.1, 0.1, (n, 3)) * np.array([1.0, 1.0, 0.5])
        # the shared rows' means on the shared plane through the level's middle over the origin: z from x and y
        mean[near, 2] = centre[near, 2] - (shared[0] * mean[near, 0] + shared[1] * mean[near, 1]) / shared[2]
        count = rng.integers(3, 41, n)
        rough = np.where(rng.random(n) < 0.12, rng.uniform(1.0, 3.0, n), rng.uniform(0.0, 0.9, n)) * 0.004 * count
        g = rng.normal(0.0, 0.05, (n, 3, 3))
        S = np.einsum("nij,nkj->nik", g, g) * count[:, None, None]
        cov = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)
        flags = np.where(rng.random(n) < 0.9, 3, np.where(rng.random(n) < 0.5, 1, 0))
        cells = dict(sx=sx, sy=sy, sz=sz, mean=mean, normal=normal, rough=rough, flags=flags, count=count, cov=cov)
        super().__init__(cells, ncol, table=1024)
        self.cells = dict(num_nodes=self.n, **{k: getattr(self, k) for k, _ in self.ROWS})


FUZZ_RULE = dict(max_offset=0.125, max_var=0.004)


def scene_is_rich(ref):
    """on the restatement alone: at least two patches of two or more members, an adjacent candidate pair the angle refuses, one the
    offset refuses, a row max_var refuses"""
    A, B, linked, angle, offset = ref["pairs"]
    return bool((ref["patches"]["nodes"] >= 2).sum() >= 2 and (~angle).any() and (angle & ~offset).any() and ref["var_refused"] > 0)


def fuzz_reference(g, R):
    ref_map = pr.Map(g.cells)
    ref = ref_map.patches(R)
    stats = (ref_map.flags & 1) != 0
    ref["var_refused"] = int((stats & ~ref["cand"]).sum())
    return ref_map, ref


def test_fuzz_200_random_lattices():
    rng = np.random.default_rng(20241021)
    redraws = 0
    for k in range(200):
        R = pr.rule(pr.NODES, 3, **FUZZ_RULE)
        while True:
            g = Lattice(rng)
            ref_map, ref = fuzz_reference(g, R)
            if scene_is_rich(ref):
                break
            redraws += 1
            assert redraws <= 20, "more than 10 % of the scenes redrawn"
        got, _ = check(g, ref_map, R, what=(k, "base"), spread_slack=True)
        links_both_ways(g, ref_map, R, ref, k)
        R2 = pr.rule(int(rng.integers(0, 2)), int(rng.integers(0, 4)), max_angle_deg=float(rng.choice([5.0, 15.0, 40.0])),
                     max_offset=float(rng.choice([0.02, 0.125, 0.3])), max_var=float(rng.choice([0.001, 0.004, 0.02])),
                     level_deg=float(rng.choice([5.0, 10.0, 30.0])))
        box = None if rng.random() < 0.5 else tuple(int(v) for v in (rng.integers(-6, 0), rng.integers(1, 7), rng.integers(-6, 0), rng.integers(1, 7)))
        check(g, ref_map, R2, box=box, min_size=int(rng.integers(0, 4)), order=rng.permutation(g.n), what=(k, R2, box), spread_slack=True)
    print(f"patch fuzz: {redraws} scenes redrawn for 200 kept")
    assert redraws <= 20


def test_the_patch_record_dtype_matches_the_header_and_decodes_as_its_fields(tmp_path):
    """gndt_patch as tests/test_abi_layout_host.py holds the records of _lib.RECORDS: sizeof and every offsetof from a C program that
    includes the header, then record_views against the numpy fields on random bytes"""
    import os
    import shutil
    import subprocess
    import torch
    from grid_ndt_amd import _lib
    (cname, dt), = _lib.PATCH_RECORD.items()
    assert cname not in _lib.RECORDS and dt.itemsize == pr.RECORD.itemsize == 128
    assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, pr.RECORD.fields[n][1]) for n in pr.RECORD.names]
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no host C compiler"
    src = ["#include <stddef.h>", "#include <stdio.h>", '#include "gndt.h"', "int main(void) {", f'    printf("%zu", sizeof({cname}));']
    src += [f'    printf(" %zu", offsetof({cname}, {f}));' for f in dt.names] + ["    return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(src) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([cc, "-std=c99", "-I", os.path.join(root, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    assert [int(x) for x in out.split()] == [dt.itemsize] + [dt.fields[f][1] for f in dt.names]
    for K in (0, 1, 5):
        raw = np.random.default_rng(K).integers(0, 256, (K, dt.itemsize), dtype=np.uint8)
        host = raw.view(dt).reshape(K)
        views = _lib.record_views(torch.from_numpy(raw.view(np.int32).copy()), dt)
        assert list(views) == [n for n in dt.names if n != "reserved"]
        for name, t in views.items():
            got = t.numpy()
            assert got.shape == host[name].shape, name
            assert (np.ascontiguousarray(got).view(np.uint8) == np.ascontiguousarray(host[name]).view(np.uint8)).all(), name


def test_no_cpu_fallback_for_patches(native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import grid_ndt_amd as g
    m = g.TwoDmap(0.5, 0.5)
    m.setCloudFirst((0, 0, 0))
    for host in (False, True):
        with pytest.raises(g.GndtError) as e:
            m.patches(host=host)
        assert e.value.code == 2   # GNDT_ERR_NO_DEVICE
