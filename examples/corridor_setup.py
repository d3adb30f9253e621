#!/usr/bin/env python3
"""What upstream GCOPTER's setup() does before its optimisation, on the device, and what it buys:

    synthetic PointCloud2 -> VoxelMap -> convexCover(route, map) -> shortCut -> planner form
    (a) lbfgs_minco_sfc from the mean of every overlap's vertices, equal durations
    (b) sfc_setup: shortest route through the corridor (one point per overlap), pieces per polytope by length_per_piece, inner
        waypoints evenly spaced, durations from the leg lengths -> lbfgs_minco_sfc from there

and prints evaluations and final cost of both.

    python examples/corridor_setup.py        # needs a GPU
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import allocnet_amd as aa  # noqa: E402
from allocnet_amd.synth import forest_cloud, forest_route  # noqa: E402


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
    pen = aa.make_penalty(rho=50.0, w_corridor=1e4, w_vel=1e3, w_acc=1e3, smooth_mu=1e-2, max_vel=4.0, max_acc=6.0, res=20, poly_rows=M)
    length = np.linalg.norm(np.diff(route, axis=0), axis=1).sum()

    # (a) the start lbfgs_minco_sfc has on its own
    T = np.full((1, N), length / N / 2.0)
    a = aa.lbfgs_minco_sfc(head, tail, hp, T, 3, penalty=pen, max_evals=2000)
    print(f"{N} polytopes of up to {M} rows")
    print(f"(a) vertex-mean start, {N} pieces:  status {int(a['status'][0])} ({aa.lbfgs_strerror(a['status'][0])}), "
          f"{int(a['evals'][0])} evaluations, cost {a['cost'][0]:.4f}, total time {a['T'][0].sum():.3f} s")

    # (b) the setup
    sp = aa.sfc_shortest_path(head[:, :, 0], tail[:, :, 0], hp)
    mean = aa.sfc_overlap_vertices(hp, max_verts=sp["max_verts"])
    k = np.maximum(mean["count"][0], 1)[:, None]
    mean_len = np.linalg.norm(np.diff(np.vstack([route[0], mean["verts"][0].sum(1) / k, route[-1]]), axis=0), axis=1).sum()
    print(f"    shortest route {sp['length'][0]:.3f} m after {int(sp['evals'][0])} evaluations "
          f"({aa.lbfgs_strerror(sp['status'][0])}); through the vertex means {mean_len:.3f} m")
    groups = aa.sfc_setup(head[:, :, 0], tail[:, :, 0], hp, length_per_piece=4.0, speed=2.0, min_duration=0.1)
    if not groups:
        print("the corridor has a pair of polytopes without an overlap")
        return 1
    g = groups[0]
    b = aa.lbfgs_minco_sfc(head[g["index"]], tail[g["index"]], g["hpolys"], g["T"], 3, wps=g["wps"], penalty=pen, max_evals=2000)
    print(f"(b) sfc_setup, pieces {g['pieces'][0].tolist()}:  status {int(b['status'][0])} ({aa.lbfgs_strerror(b['status'][0])}), "
          f"{int(b['evals'][0])} evaluations, cost {b['cost'][0]:.4f}, total time {b['T'][0].sum():.3f} s")
    return 0 if b["status"][0] != aa.SFC_NO_OVERLAP else 1


if __name__ == "__main__":
    sys.exit(main())
