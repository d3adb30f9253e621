#!/usr/bin/env python3
"""A trajectory towards space nobody has seen, timed so that the vehicle can always stop inside what it knows -- the setting of
examples/explore_forest.py (the same synthetic forest, map and sensor), which plans a route and then "flies" the polyline by
interpolation:

    first scans -> OccupancyMap.to_voxel_map(unknown="blocked") -> next_view -> plan_path to the chosen pose
    -> the route's corners (legs longer than 2 m split evenly) as the waypoints of a rest-to-rest jerk trajectory
    -> lbfgs_optimize_dev, once on
    obstacle_objective_dev (keep `clearance` from occupied and unknown space) and once on stop_objective_dev (keep the reaction
    and braking distance plus `clearance` inside known free space), with the same clearance, weight and rho

Printed for the start and both results: the total duration, the peak speed, the worst ball margin (traj_stop_margin: a SAMPLED
check) and the number of samples the directional check traj_stop_check calls unsafe.

    python examples/fly_into_unknown.py [--scans N]   # needs a GPU
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allocnet_amd as aa  # noqa: E402
from allocnet_amd.synth import forest_cloud, forest_route  # noqa: E402
from explore_forest import MIN_SIZE, Sensor  # noqa: E402
from map_from_scans import SIZE, ORIGIN, SCALE, MAX_RANGE, poses_along  # noqa: E402

A_BRAKE, T_REACT = 5.0, 0.1          # m/s^2, s
CLEARANCE, WEIGHT, MU, RHO, RES = 0.3, 5000.0, 0.05, 500.0, 20   # rho: time is dear, so that the energy alone does not slow the flight
CRUISE = 4.0                         # m/s: the first durations are the segment lengths at this speed
PIECE_LENGTH = 2.0                   # m: longer legs of the route are split into pieces of at most this length


def report(name, co, T, vm):
    margin = aa.traj_stop_margin(co, T, vm, A_BRAKE, T_REACT, CLEARANCE, RES)[0].min()
    unsafe = int(aa.traj_stop_check(co, T, vm, A_BRAKE, T_REACT, RES)[0][0])
    print(f"{name:9s} duration {T.sum():6.2f} s, peak speed {aa.traj_max_rate(co, T, 1).max():5.2f} m/s, worst ball margin "
          f"{margin:+.3f} m, unsafe samples {unsafe} of {T.shape[1] * (RES + 1)}")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=3)
    args = ap.parse_args()
    route = forest_route()
    truth = aa.VoxelMap(SIZE, ORIGIN, SCALE)
    truth.setOccupiedCloud(forest_cloud(np.random.default_rng(17), n_points=1_000_000, clear_route=route).tobytes(), 16)
    om = aa.OccupancyMap(SIZE, ORIGIN, SCALE, aa.occupancy_params(max_range=MAX_RANGE))
    sensor = Sensor(truth, om)
    first = poses_along(route, 24)[:args.scans]
    for p in first:
        sensor.scan(p)
    pose = first[-1]
    vm = aa.VoxelMap(SIZE, ORIGIN, SCALE)
    om.to_voxel_map(occ=0, unknown="blocked", out=vm)
    nv = aa.next_view(om, vm, pose, sensor.template, occ=0, min_size=MIN_SIZE, connectivity=26, radii=(1.0, 2.5), n_yaw=8, height=pose[2],
                      lam=0.15)
    if len(nv["order"]) == 0:
        print("no reachable frontier cluster")
        return 1
    goal = nv["t"][int(nv["order"][0])]
    cost, path = aa.plan_path(pose, goal, None, None, vm)
    if len(path) < 2:
        print("the chosen pose has no route")
        return 1
    # the route's corners, and evenly spaced points between them so that no piece is longer than PIECE_LENGTH
    pts = [path[0]]
    for a, b in zip(path[:-1], path[1:]):
        n = max(1, int(np.ceil(np.linalg.norm(b - a) / PIECE_LENGTH)))
        pts += [a + (b - a) * k / n for k in range(1, n + 1)]
    corners, path = len(path), np.asarray(pts)
    if len(path) > 17:
        print(f"a route of {len(path)} points cannot be the waypoints of one trajectory")
        return 1
    print(f"{args.scans} scans, {100 * om.known_fraction():.2f} % known; route of {corners} corners, {cost:.2f} m, {len(path) - 1} pieces, from "
          f"{np.round(pose, 2).tolist()} to {np.round(goal, 2).tolist()}")
    s, c, N, B, ld = 3, 3, len(path) - 1, 1, 1
    head, tail = np.zeros((B, 3, c)), np.zeros((B, 3, c))
    head[0, :, 0], tail[0, :, 0] = path[0], path[-1]
    wps = path[None, 1:-1]
    T = (np.linalg.norm(np.diff(path, axis=0), axis=1) / CRUISE + 0.2)[None]
    field = (vm, vm.distance_field(walls=True, refresh=True))

    def dev(a):                      # (B, fields) -> batch-minor (fields, ld)
        t = torch.zeros(a.size // B, ld, dtype=torch.float64)
        t[:, :B] = torch.from_numpy(a.reshape(B, -1)).T
        return t.to(vm.device)
    pen = aa.make_penalty(rho=RHO, res=RES)
    terms = {
        "obstacle": aa.obstacle_objective_dev(dev(head), dev(tail), s, c, N, B, field,
                                              aa.make_obstacle_penalty(w=WEIGHT, smooth_mu=MU, clearance=CLEARANCE, res=RES), penalty=pen),
        "stop": aa.stop_objective_dev(dev(head), dev(tail), s, c, N, B, field,
                                      aa.make_stop_penalty(w=WEIGHT, smooth_mu=MU, clearance=CLEARANCE, a_brake=A_BRAKE, t_react=T_REACT,
                                                           speed_eps=1e-2, res=RES), penalty=pen),
    }
    co, _ = aa.minco_solve(head, tail, wps, T, s)
    report("start", co, T, vm)
    nw = 3 * (N - 1)
    for name, ev in terms.items():
        x = torch.zeros(nw + N, ld, dtype=torch.float64, device=vm.device)
        if nw:
            x[:nw] = dev(wps)
        x[nw:] = dev(np.log(T))
        out = aa.lbfgs_optimize_dev(x, ev, batch=B, param=aa.lbfgs_parameter_t(past=3, delta=1e-5), max_evals=600)
        torch.cuda.synchronize()
        w1 = x[:nw, :B].T.cpu().numpy().reshape(B, N - 1, 3)
        T1 = np.exp(x[nw:, :B].T.cpu().numpy())
        co1, _ = aa.minco_solve(head, tail, w1, T1, s)
        print(f"{name}: status {out['status'].cpu().numpy().tolist()}, {out['evals'].cpu().numpy().tolist()} evaluations")
        report(name, co1, T1, vm)
    return 0


if __name__ == "__main__":
    sys.exit(main())
