#!/usr/bin/env python3
"""The online flow from a point cloud, all of its map and corridor work on the MI355X:

    synthetic PointCloud2 -> VoxelMap fill (mapCallBack) -> dilate(2) -> convexCover(route, map) -> shortCut
    -> planner form -> [network: segment times] -> QPSolver::solve -> Trajectory

The map is the launch file's (40 x 40 x 5 m at 0.1 m, inflate_radius 0.2 -> r = 2).  By default a fixed route stands in
for the path search; with --plan the route comes from plan_path(start, goal) on the map, as LearningPlanner::plan does
when it is handed an empty route (sfc_gen::planPath).  That route spans the whole map, so its corridor usually needs more
than the model's five polytopes and the run stops there, as plan() does.

    python examples/plan_from_cloud.py [--plan]   # needs a GPU; prints the stages and their wall times
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import allocnet_amd as aa  # noqa: E402
from allocnet_amd.synth import forest_cloud, forest_route  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", action="store_true", help="plan the route from forest_route()[0] to [-1] on the map")
    args = ap.parse_args()
    route = forest_route()[:3]                                                   # two legs: a corridor the model takes
    cloud = forest_cloud(np.random.default_rng(17), n_points=1_000_000, clear_route=forest_route())    # float32 records, 16 B each
    buf = cloud.tobytes()
    # warm-up: module load and first launches
    w = aa.VoxelMap((40, 40, 5), (-20.0, -20.0, 0.0), 1.0)
    w.setOccupiedCloud(buf, 16); w.dilate(1); aa.convex_cover(route[:2], w, w.getOrigin(), w.getCorner(), 7.0, 3.0)
    if args.plan:
        aa.plan_path(route[0], route[1], w.getOrigin(), w.getCorner(), w)
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    vm = aa.VoxelMap((400, 400, 50), (-20.0, -20.0, 0.0), 0.1)                  # learning_planning.cpp: the map
    vm.setOccupiedCloud(buf, 16)                                                 # mapCallBack's fill
    torch.cuda.synchronize(); t1 = time.perf_counter()
    vm.dilate(2)                                                                 # inflate_radius 0.2 / 0.1
    t2 = tc = time.perf_counter()
    if args.plan:                                                                # learning_planner.hpp:251-262
        s, g = forest_route()[0], forest_route()[-1]
        costs, paths, status, rounds = aa.plan_paths(s[None], g[None], vm, vm.getOrigin(), vm.getCorner(), with_rounds=True)
        route = paths[0]
        tc = time.perf_counter()
        print(f"planPath {1e3 * (tc - t2):.2f} ms ({rounds} rounds, status {int(status[0])}): {len(route)} points, "
              f"length {costs[0]:.2f} m")
        if len(route) == 0:
            return 1
    polys = aa.convex_cover(route, vm, vm.getOrigin(), vm.getCorner(), progress=7.0, rng_range=3.0)   # learning_planner.hpp:274-280
    t3 = time.perf_counter()
    polys = aa.short_cut(polys)                                                  # :282
    t4 = time.perf_counter()
    seg = len(polys)
    print(f"fill {1e3 * (t1 - t0):.2f} ms ({len(cloud)} records) -> dilate(2) + surface {1e3 * (t2 - t1):.2f} ms "
          f"({vm.surf_ids_dev.numel()} surface voxels) -> convexCover {1e3 * (t3 - tc):.2f} ms -> shortCut "
          f"{1e3 * (t4 - t3):.2f} ms -> {seg} polytopes")
    if seg > 5:
        print("give up this try, long corridor")                                # :286-290 (modelMaxSeg)
        return 1
    rows = [len(p) for p in polys]
    raw = np.zeros((seg, max(rows), 4))
    for i, p in enumerate(polys):
        raw[i, :len(p)] = p
    hp = aa.to_planner_form(raw, rows)                                           # :293-299
    ini = np.zeros((3, 3)); fin = np.zeros((3, 3))
    ini[:, 0] = route[0]; fin[:, 0] = route[-1]
    length = np.linalg.norm(np.diff(route, axis=0), axis=1).sum()
    times = np.full(seg, length / seg / 2.0, dtype=np.float32)                   # <- the network's segment times
    t5 = time.perf_counter()
    solver = aa.QPSolver(aa.QPConfig(MaxVelBox=4.0, MaxAccBox=6.0, ConstRes=20))
    solver.setOrder(4)
    ok, flat = solver.solve(ini, fin, [hp[i, :rows[i]] for i in range(seg)], times)
    t6 = time.perf_counter()
    print(f"QP {1e3 * (t6 - t5):.2f} ms, solved {ok}")
    if not ok:
        return 1
    traj = aa.Trajectory()
    co = np.asarray(flat).reshape(seg, 3, 8)
    for i in range(seg):
        traj.emplace_back(float(times[i]), co[i])
    T = traj.getTotalDuration()
    print(f"trajectory: {T:.2f} s, start {traj.getPos(0.0)}, end {traj.getPos(T)}, max |v| {traj.getMaxVelRate():.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
