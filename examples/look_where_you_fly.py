#!/usr/bin/env python3
"""A trajectory towards space nobody has seen that keeps its direction of travel inside the camera's field of view -- the forest,
map and sensor of examples/fly_into_unknown.py, with a route that has at least one corner:

    first scans -> OccupancyMap.to_voxel_map(unknown="blocked") -> next_view -> plan_path to the first candidate pose whose route
    has a corner (if every route is straight: the way already flown, from the first scan pose to the current one, is put in front)
    -> the route's corners (legs longer than 2 m split evenly) as the waypoints of a rest-to-rest jerk trajectory, the yaw as a
    one-axis MINCO of order 2 over the same pieces, from the heading of the first leg to the heading of the last
    -> lbfgs_optimize_dev on yaw_objective_dev: position, yaw and durations jointly, the stop term of fly_into_unknown.py riding
    along as an extra accumulate = 1 term

Printed before and after, and once for the optimised position trajectory with the yaw HELD at the unconstrained tangent heading
(the waypoint headings of heading_waypoints, no rate limit seen): the worst look margin (traj_yaw_margin: a SAMPLED check, samples
slower than V_MIN not counted), the peak sampled yaw rate, the total duration and the worst stop margin.

    python examples/look_where_you_fly.py [--scans N]   # needs a GPU
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allocnet_amd as aa  # noqa: E402
from allocnet_amd.synth import forest_cloud, forest_route  # noqa: E402
from explore_forest import MIN_SIZE, Sensor  # noqa: E402
from fly_into_unknown import A_BRAKE, CLEARANCE, CRUISE, MU, PIECE_LENGTH, RES, RHO, T_REACT, WEIGHT  # noqa: E402
from map_from_scans import SIZE, ORIGIN, SCALE, MAX_RANGE, poses_along  # noqa: E402

HALF_FOV, MAX_RATE, V_MIN = math.radians(35.0), 1.0, 0.2     # rad, rad/s, m/s
SY = 2                                                       # the yaw minimises its angular acceleration


def report(name, co, cy, T, vm):
    m, _, r = aa.traj_yaw_margin(co, cy, T, HALF_FOV, V_MIN, RES)
    stop = aa.traj_stop_margin(co, T, vm, A_BRAKE, T_REACT, CLEARANCE, RES)[0].min()
    print(f"{name:9s} worst look margin {m.min():+.3f} rad, peak yaw rate {r.max():5.2f} rad/s, duration {T.sum():6.2f} s, worst stop "
          f"margin {stop:+.3f} m")


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
    path, cost, how, straight = None, 0.0, "", None
    for rank, k in enumerate(nv["order"]):
        cst, pth = aa.plan_path(pose, nv["t"][int(k)], None, None, vm)
        if len(pth) >= 3:
            path, cost, how = [np.asarray(q) for q in pth], cst, f"candidate {rank} of next_view"
            break
        if rank == 0 and len(pth) == 2:
            straight = (cst, [np.asarray(q) for q in pth])
    if path is None:
        if straight is None:
            print("the chosen pose has no route")
            return 1
        start = np.asarray(first[0], dtype=np.float64)
        path = [start] + straight[1]
        cost, how = straight[0] + float(np.linalg.norm(straight[1][0] - start)), "the way flown so far, then the first candidate"
    pts = [path[0]]
    for a, b in zip(path[:-1], path[1:]):
        n = max(1, int(np.ceil(np.linalg.norm(b - a) / PIECE_LENGTH)))
        pts += [a + (b - a) * k / n for k in range(1, n + 1)]
    corners, path = len(path), np.asarray(pts)
    if len(path) > 17:
        print(f"a route of {len(path)} points cannot be the waypoints of one trajectory")
        return 1
    print(f"{args.scans} scans, {100 * om.known_fraction():.2f} % known; route ({how}) of {corners} corners, {cost:.2f} m, "
          f"{len(path) - 1} pieces, from {np.round(path[0], 2).tolist()} to {np.round(path[-1], 2).tolist()}")
    s, c, N, B, ld = 3, 3, len(path) - 1, 1, 1
    head, tail = np.zeros((B, 3, c)), np.zeros((B, 3, c))
    head[0, :, 0], tail[0, :, 0] = path[0], path[-1]
    wps = path[None, 1:-1]
    T = (np.linalg.norm(np.diff(path, axis=0), axis=1) / CRUISE + 0.2)[None]
    h0, hw, h1 = aa.heading_waypoints(wps[0], path[0], path[-1])
    yhead, ytail = np.zeros((B, SY)), np.zeros((B, SY))
    yhead[0, 0], ytail[0, 0] = h0, h1
    ywps = np.full((B, N - 1), h0)                           # the start of the optimisation: the camera keeps looking where it looked
    field = (vm, vm.distance_field(walls=True, refresh=True))

    def dev(a):                      # (B, fields) -> batch-minor (fields, ld)
        t = torch.zeros(a.size // B, ld, dtype=torch.float64)
        t[:, :B] = torch.from_numpy(a.reshape(B, -1)).T
        return t.to(vm.device)
    pen = aa.make_penalty(rho=RHO, res=RES)
    stop = aa.make_stop_penalty(w=WEIGHT, smooth_mu=MU, clearance=CLEARANCE, a_brake=A_BRAKE, t_react=T_REACT, speed_eps=1e-2, res=RES)
    yaw = aa.make_yaw_penalty(w_look=WEIGHT, mu_look=MU, half_fov=HALF_FOV, speed_eps=1e-2, w_rate=WEIGHT, mu_rate=MU, max_rate=MAX_RATE,
                              w_energy=1.0, res=RES)
    ride = lambda coeffs, T_, gdC, gdT, pc, stream: aa.minco_stop_partial_grads_dev(stop, s, N, B, coeffs, T_, field, gdC, gdT, pc,
                                                                                   accumulate=True, stream=stream)
    ev = aa.yaw_objective_dev(dev(head), dev(tail), dev(yhead), dev(ytail), s, c, SY, SY, N, B, yaw, penalty=pen, extra_terms=(ride,))
    co, _ = aa.minco_solve(head, tail, wps, T, s)
    cy, _ = aa.minco_solve_scalar(yhead, ytail, ywps, T, SY)
    report("start", co, cy, T, vm)
    nw, ny = 3 * (N - 1), N - 1
    x = torch.zeros(nw + ny + N, ld, dtype=torch.float64, device=vm.device)
    x[:nw] = dev(wps)
    x[nw:nw + ny] = dev(ywps)
    x[nw + ny:] = dev(np.log(T))
    out = aa.lbfgs_optimize_dev(x, ev, batch=B, param=aa.lbfgs_parameter_t(past=3, delta=1e-5), max_evals=1500)
    torch.cuda.synchronize()
    xs = x[:, :B].T.cpu().numpy()
    w1, y1, T1 = xs[:, :nw].reshape(B, N - 1, 3), xs[:, nw:nw + ny], np.exp(xs[:, nw + ny:])
    co1, _ = aa.minco_solve(head, tail, w1, T1, s)
    cy1, _ = aa.minco_solve_scalar(yhead, ytail, y1, T1, SY)
    print(f"joint: status {out['status'].cpu().numpy().tolist()}, {out['evals'].cpu().numpy().tolist()} evaluations")
    report("joint", co1, cy1, T1, vm)
    # the same position trajectory with the yaw held at the tangent headings of its waypoints
    t0, tw, t1 = aa.heading_waypoints(w1[0], path[0], path[-1])
    th, tt = yhead.copy(), ytail.copy()
    th[0, 0], tt[0, 0] = t0, t1
    cyt, _ = aa.minco_solve_scalar(th, tt, tw[None], T1, SY)
    report("tangent", co1, cyt, T1, vm)
    return 0


if __name__ == "__main__":
    sys.exit(main())
