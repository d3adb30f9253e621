#!/usr/bin/env python3
"""Fixtures of the exact trajectory-against-voxel-map test, made on the CPU by this project's own multiprecision reference
(tests/traj_voxel_hit_mp.py).  Writes data only: tests/golden/traj_voxel_hit_cases.npz.

    python tests/golden/make_traj_voxel_hit_golden.py [--check]

Grids: 0 the 16 x 12 x 8 map (origin (-2, -1.5, 0), scale 0.25) filled at random to about 3 % with the start cell cleared; 1 the
same grid, empty; 2 the same grid with the one voxel (8, 6, 4) set; 3 a 1 x 1 x 1 grid (origin 0, scale 1), empty.
Families, for each order s = 2, 3, 4: free, hit_low / hit_high (the blocked voxel entered with the crossed coordinate rising /
falling), exit_x0 .. exit_z1 (the six map faces), start_blocked, cell0 (the -1 < q < 1 cell of truncation toward zero), cheb
(Chebyshev-like components), long (more than 30 planes crossed), unit (the 1 x 1 x 1 grid), graze_in / graze_out (a tangency to
a blocked face that penetrates by +1e-3 / -1e-3 voxels: must hit / must not).
A candidate is rejected and redrawn when an extremum or an end value of a component lies within 1e-6 voxels of a plane of its
axis, or when two crossings on different axes, neither later than t* + 1e-6, lie within 1e-6 (normalised time) of each other:
every case in the file is then compared by the tests and none is left out at test time.  Fewer than 5 % are rejected (asserted).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import traj_voxel_hit_mp as hm  # noqa: E402

OUT = os.path.join(HERE, "traj_voxel_hit_cases.npz")
SIZE, ORIGIN, SCALE = (16, 12, 8), (-2.0, -1.5, 0.0), 0.25
START_CELL = (8, 6, 4)                     # of grid 0; cleared
SEP = 1e-6
PER_FAMILY = 4


def grids():
    rng = np.random.default_rng(20261019)
    n = SIZE[0] * SIZE[1] * SIZE[2]
    main = (rng.random(n) < 0.03).astype(np.uint8) * rng.integers(1, 3, n).astype(np.uint8)      # values 1 and 2
    lin = lambda c: c[0] + SIZE[0] * (c[1] + SIZE[1] * c[2])
    main[lin(START_CELL)] = 0
    one = np.zeros(n, dtype=np.uint8)
    one[lin(START_CELL)] = 1
    g = hm.Grid(SIZE, ORIGIN, SCALE)
    return [(g, main), (g, np.zeros(n, dtype=np.uint8)), (g, one), (hm.Grid((1, 1, 1), (0.0, 0.0, 0.0), 1.0), np.zeros(1, dtype=np.uint8))]


def from_control_points(bq, T, grid):
    """Bernstein control points in voxel coordinates (3, D) -> coefficient matrix in metres and local time, highest power first"""
    from math import comb
    D = bq.shape[1]
    n = D - 1
    cm = np.zeros((3, D))
    for ax in range(3):
        for k in range(D):        # ascending coefficient k in normalised time
            u = sum(comb(n, k) * comb(k, i) * (-1) ** (k - i) * bq[ax, i] for i in range(k + 1))
            if k == 0:
                cm[ax, n] = u * grid.scale + grid.origin[ax]
            else:
                cm[ax, n - k] = u * grid.scale / T ** k
    return cm


def draw(family, s, rng, G):
    """-> (grid id, cm, T) of a candidate; the family is verified on the reference afterwards"""
    D = 2 * s
    T = float(rng.uniform(0.4, 3.0))
    centre = np.array(START_CELL) + 0.5
    gid = 0
    if family == "unit":
        gid = 3
        bq = rng.uniform(-0.9, 0.9, (3, D))
        if rng.random() < 0.5:
            bq[rng.integers(3), -1] = rng.choice([-1.8, 1.7])
        return gid, from_control_points(bq, T, G[gid][0]), T
    if family in ("graze_in", "graze_out"):
        # q_x = 8 + pen - 2 (tau - 1/2)^2 from below the voxel (8, 6, 4) of grid 2 (its face q_x = 8), or mirrored from above its
        # face q_x = 9; y and z move inside their cells
        gid = 2
        pen = 1e-3 if family == "graze_in" else -1e-3
        above = rng.random() < 0.5
        cm = np.zeros((3, D))
        g = G[gid][0]
        sgn = -1.0 if above else 1.0
        face = 9.0 if above else 8.0
        qx = [face + sgn * (pen - 0.5), sgn * 2.0, -sgn * 2.0]       # ascending in tau
        qy = [6.3 + 0.2 * rng.random(), 0.3 * rng.random()]
        qz = [4.3 + 0.2 * rng.random(), 0.3 * rng.random()]
        for ax, qa in enumerate((qx, qy, qz)):
            for k, u in enumerate(qa):
                cm[ax, D - 1 - k] = u * g.scale / T ** k + (g.origin[ax] if k == 0 else 0.0)
        return gid, cm, T
    if family == "cheb":
        gid = int(rng.choice([0, 1]))
        cm = np.zeros((3, D))
        g = G[gid][0]
        for ax in range(3):
            amp = rng.uniform(0.5, 3.0)
            qa = amp * hm.cheb_coeffs(D - 1 - int(rng.integers(0, 2)))
            qa[0] += centre[ax] + rng.uniform(-0.3, 0.3)
            for k, u in enumerate(qa):
                cm[ax, D - 1 - k] = u * g.scale / T ** k + (g.origin[ax] if k == 0 else 0.0)
        return gid, cm, T
    if family == "long":
        # on the empty grid, from one corner of the map to the opposite one: 15 + 11 + 7 planes
        gid = 1
        lo, hi = rng.uniform(0.1, 0.6, 3), np.array(SIZE) - rng.uniform(0.1, 0.6, 3)
        flip = rng.random(3) < 0.5
        lo, hi = np.where(flip, hi, lo), np.where(flip, lo, hi)
        w = np.linspace(0.0, 1.0, D)[None]
        bq = lo[:, None] * (1.0 - w) + hi[:, None] * w + np.c_[np.zeros((3, 1)), rng.uniform(-0.5, 0.5, (3, D - 2)), np.zeros((3, 1))]
        return gid, from_control_points(bq, T, G[gid][0]), T
    bq = centre[:, None] + rng.uniform(-0.45, 0.45, (3, D))
    if family == "free":
        gid = int(rng.choice([0, 1]))
        bq += rng.uniform(-1.5, 1.5, (3, D)) * rng.random()
    elif family in ("hit_low", "hit_high"):
        gid = int(rng.choice([0, 2]))
        if gid == 2:       # start somewhere else and end in the one voxel
            a = centre + rng.uniform(1.5, 4.0, 3) * rng.choice([-1.0, 1.0], 3)
            e = centre + rng.uniform(-0.3, 0.3, 3)
        else:              # start in the cleared cell and end in some blocked voxel
            ids = np.flatnonzero(G[0][1])
            i = int(ids[rng.integers(len(ids))])
            a = centre + rng.uniform(-0.4, 0.4, 3)
            e = np.array([i % SIZE[0], (i // SIZE[0]) % SIZE[1], i // (SIZE[0] * SIZE[1])]) + rng.uniform(0.2, 0.8, 3)
        w = np.linspace(0.0, 1.0, D)[None]
        bq = a[:, None] * (1.0 - w) + e[:, None] * w + np.c_[np.zeros((3, 1)), rng.uniform(-0.4, 0.4, (3, D - 2)), np.zeros((3, 1))]
    elif family.startswith("exit_"):
        gid = 1
        ax, hi = "xyz".index(family[5]), family[6] == "1"
        bq += rng.uniform(-1.0, 1.0, (3, D))
        bq[:, 0] = centre + rng.uniform(-0.4, 0.4, 3)
        far = SIZE[ax] + rng.uniform(0.3, 3.0) if hi else -1.0 - rng.uniform(0.3, 3.0)
        bq[ax] = np.linspace(bq[ax, 0], far, D) + np.r_[0.0, rng.uniform(-0.8, 0.8, D - 1)]
    elif family == "start_blocked":
        gid = int(rng.choice([0, 2]))
        if gid == 0 and rng.random() < 0.5:     # outside the map
            bq[int(rng.integers(3)), 0] = rng.choice([-1.0 - rng.uniform(0.01, 2.0), 30.0])
        else:
            g, vox = G[gid]
            ids = np.flatnonzero(vox)
            i = int(ids[rng.integers(len(ids))])
            cell = np.array([i % SIZE[0], (i // SIZE[0]) % SIZE[1], i // (SIZE[0] * SIZE[1])])
            bq[:, 0] = cell + rng.uniform(0.05, 0.95, 3)
    elif family == "cell0":
        # on grid 1: a coordinate dips below the origin, -1 < q < 0, where truncation still gives cell 0; half of them go on to
        # q <= -1 and leave the map there (not at q = 0)
        gid = 1
        ax = int(rng.integers(3))
        bq[ax] = np.linspace(rng.uniform(0.2, 1.8), rng.uniform(-0.9, -0.1), D) + np.r_[0.0, rng.uniform(-0.05, 0.05, D - 1)]
        if rng.random() < 0.5:
            bq[ax, -1] = -1.0 - rng.uniform(0.2, 1.0)
    else:
        raise ValueError(family)
    return gid, from_control_points(bq, T, G[gid][0]), T


def classify(family, ref, cr, grid):
    """does the reference's answer make the candidate a member of the family?"""
    v, ax = ref["voxel"], ref["axis"]
    if family in ("free", "graze_out"):
        return v == hm.HIT_FREE
    if family == "start_blocked":
        return ref["tau"] == 0
    if family in ("hit_low", "hit_high", "graze_in"):
        if v < 0 or ax < 0:
            return False
        rising = ref["plane"] == (v // [1, grid.size[0], grid.size[0] * grid.size[1]][ax]) % grid.size[ax]
        return family == "graze_in" or rising == (family == "hit_low")
    if family.startswith("exit_"):
        want_ax, hi = "xyz".index(family[5]), family[6] == "1"
        return v == hm.HIT_OUTSIDE and ax == want_ax and ref["plane"] == (grid.size[ax] if hi else -1)
    if family == "cell0":
        return v == hm.HIT_FREE or (v == hm.HIT_OUTSIDE and ref["plane"] == -1)
    if family == "long":
        n = len(cr) if ref["tau"] is None else sum(1 for c in cr if c[0] <= ref["tau"])
        return n > 30
    return True        # cheb, unit: whatever they give


def accept(q, ref, grid):
    """the two rejection rules"""
    if hm.extrema_clearance_mp(q, grid) <= SEP:
        return False
    cr = ref["crossings"]
    if ref["tau"] is not None:
        cr = [c for c in cr if c[0] <= ref["tau"] + SEP]
    return all(b[0] - a[0] > SEP or a[1] == b[1] for a, b in zip(cr, cr[1:]))


def build():
    G = grids()
    families = ["free", "hit_low", "hit_high"] + ["exit_%s%d" % (a, h) for a in "xyz" for h in (0, 1)] + \
        ["start_blocked", "cell0", "cheb", "long", "unit", "graze_in", "graze_out"]
    rows = []
    drawn = rejected = 0
    for s in (2, 3, 4):
        for fi, fam in enumerate(families):
            rng = np.random.default_rng(1000 * s + fi)
            got = tries = 0
            while got < PER_FAMILY:
                tries += 1
                assert tries < 400, (fam, s)
                gid, cm, T = draw(fam, s, rng, G)
                grid, vox = G[gid]
                ref = hm.piece_hit_mp(cm, T, grid, vox)
                if not classify(fam, ref, ref["crossings"], grid):
                    continue           # not a member of the family: not a rejection, the draw is aimed, not exact
                drawn += 1
                q = hm.q_exact(cm, T, grid)
                if not accept(q, ref, grid):
                    rejected += 1
                    continue
                got += 1
                hit = ref["tau"] is not None
                A = hm.axis_scales(cm, T, grid)
                ax = ref["axis"]
                rows.append(dict(
                    family=fam, s=s, grid=gid, T=T, cm=np.pad(cm, ((0, 0), (0, 8 - cm.shape[1]))),
                    tau=float(ref["tau"]) if hit else np.inf, t=float(ref["tau"] * hm.mpmath.mpf(T)) if hit else np.inf,
                    voxel=ref["voxel"], axis=ax, plane=ref["plane"],
                    dq=float(ref["dq"]) if ax >= 0 else np.inf, scale=float(A[ax] + abs(ref["plane"])) if ax >= 0 else 0.0,
                    n_cross=len(ref["crossings"])))
    assert rejected < 0.05 * drawn, (rejected, drawn)
    out = {k: np.array([r[k] for r in rows]) for k in rows[0]}
    out["vox0"], out["vox2"] = G[0][1], G[2][1]
    out["rejected"] = np.array([rejected, drawn])
    return out


def main():
    data = build()
    if "--check" in sys.argv:
        old = np.load(OUT)
        for k in data:
            assert np.array_equal(old[k], data[k]), k
        print("fixture reproduced:", len(data["T"]), "cases")
        return
    np.savez_compressed(OUT, **data)
    fam, cnt = np.unique(data["family"], return_counts=True)
    print("wrote", OUT, len(data["T"]), "cases; rejected %d of %d" % tuple(data["rejected"]), dict(zip(fam, cnt)))


if __name__ == "__main__":
    main()
