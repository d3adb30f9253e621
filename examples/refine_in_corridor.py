#!/usr/bin/env python3
"""A corridor from the map, then the spatial-temporal optimisation INSIDE it:

    synthetic PointCloud2 -> VoxelMap -> convexCover(route, map) -> shortCut -> planner form
    -> lbfgs_minco_sfc: overlap vertices, backward_p of the start waypoints, L-BFGS over (xi, tau)

Every waypoint is a convex combination of the vertices of the overlap of the two polytopes it joins, so the junctions of the
result are inside the corridor by construction; the largest row violation at the junctions is printed (at most the enumeration's
epsilon, 1e-6), next to that of the plain lbfgs_minco run from the same start, whose waypoints only the soft penalty holds.

    python examples/refine_in_corridor.py        # needs a GPU
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import allocnet_amd as aa  # noqa: E402
from allocnet_amd.synth import forest_cloud, forest_route  # noqa: E402


def junction_violation(hp, wps):
    """Largest a.p - b over the rows of both polytopes at every junction (rows are unit normals: metres)."""
    worst = -np.inf
    for w, p in enumerate(wps):
        for poly in (hp[w], hp[w + 1]):
            rows = poly[np.any(poly[:, :3] != 0.0, axis=1)]
            worst = max(worst, float((rows[:, :3] @ p - rows[:, 3]).max()))
    return worst


def main():
    route = forest_route()[:4]
    cloud = forest_cloud(np.random.default_rng(17), n_points=1_000_000, clear_route=forest_route())
    vm = aa.VoxelMap((400, 400, 50), (-20.0, -20.0, 0.0), 0.1)
    vm.setOccupiedCloud(cloud.tobytes(), 16)
    vm.dilate(2)
    polys = aa.short_cut(aa.convex_cover(route, vm, vm.getOrigin(), vm.getCorner(), progress=7.0, rng_range=3.0, max_rows=50))
    N = len(polys)
    rows = [len(p) for p in polys]
    M = max(rows)
    raw = np.zeros((N, M, 4))
    for i, p in enumerate(polys):
        raw[i, :len(p)] = p
    hp = aa.to_planner_form(raw, rows)[None]                                     # (1, N, M, 4), rows a.x <= b
    head = np.zeros((1, 3, 3)); tail = np.zeros((1, 3, 3))
    head[0, :, 0] = route[0]; tail[0, :, 0] = route[-1]
    # start waypoints: the deepest common point of consecutive polytopes (geo_utils::overlapPt), equal durations
    wps = np.array([[aa.overlap_pt(polys[i], polys[i + 1])[1] for i in range(N - 1)]])
    length = np.linalg.norm(np.diff(route, axis=0), axis=1).sum()
    T = np.full((1, N), length / N / 2.0)
    pen = aa.make_penalty(rho=50.0, w_corridor=1e4, w_vel=1e3, w_acc=1e3, smooth_mu=1e-2, max_vel=4.0, max_acc=6.0, res=20, poly_rows=M)
    t0 = time.perf_counter()
    res = aa.lbfgs_minco_sfc(head, tail, hp, T, 3, wps=wps, penalty=pen, max_evals=2000)
    t1 = time.perf_counter()
    free = aa.lbfgs_minco(head, tail, wps, T, 3, hpolys=hp, penalty=pen, max_evals=2000, opt=aa.lbfgs.OPT_WAYPOINTS |
                          aa.lbfgs.OPT_TIMES | aa.lbfgs.OPT_LOCKSTEP)
    print(f"{N} polytopes of up to {M} rows, {res['max_verts']} vertex slots per overlap, overlap status {res['overlap_status'][0].tolist()}")
    print(f"lbfgs_minco_sfc: {1e3 * (t1 - t0):.2f} ms, status {int(res['status'][0])} ({aa.lbfgs_strerror(res['status'][0])}), "
          f"{int(res['evals'][0])} evaluations, cost {res['cost'][0]:.4f}, durations {np.round(res['T'][0], 3).tolist()}")
    print(f"largest row violation at a junction: {junction_violation(hp[0], res['wps'][0]):.3e} m (vertex weights) against "
          f"{junction_violation(hp[0], free['wps'][0]):.3e} m (free waypoints, cost {free['cost'][0]:.4f})")
    return 0 if res["status"][0] != aa.SFC_NO_OVERLAP else 1


if __name__ == "__main__":
    sys.exit(main())
