#!/usr/bin/env python3
"""A map from sensor scans instead of a finished cloud, all of it on the MI355X:

    truth forest (VoxelMap) -> per pose: a fan of rays, VoxelMap.raycast = the sensor's returns
    -> OccupancyMap.integrate (ray carving: free, occupied, unknown) -> to_voxel_map(unknown="blocked", dilate)
    -> plan_path(pose, goal) on what is known so far

A robot has no world cloud (examples/plan_from_cloud.py starts from one): it has scans taken from a pose.  Here the sensor is
flown along forest_route(); each pose casts 128 x 96 segments of 1.5 x max_range over the whole sphere against the truth map.  A
segment that hits gives the entry point, nudged 1e-6 voxels along the ray so that it lies in the voxel it entered; one that does not
gives its far end, which the scan truncates at max_range and only carves.  After each scan the route to the goal is planned with
unknown space blocked: it ends where the known space does, as a receding-horizon planner's would.  Per scan: the known fraction,
the truly occupied voxels the map holds as free, the truly free ones it holds as occupied, the route's length.  Every route, and
at the end the route from the first pose to the goal on the map of the last scan, is checked against the TRUTH map with query.

    python examples/map_from_scans.py [--poses N]   # needs a GPU
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import allocnet_amd as aa  # noqa: E402
from allocnet_amd.synth import forest_cloud, forest_route  # noqa: E402

SIZE, ORIGIN, SCALE = (200, 200, 25), (-20.0, -20.0, 0.0), 0.2
MAX_RANGE = 6.0
FAN = (128, 96)


def fan_directions():
    """128 azimuths x 96 elevations over the sphere (the poles left out), unit vectors (n, 3)."""
    az = (np.arange(FAN[0]) + 0.5) * (2.0 * np.pi / FAN[0])
    el = -0.5 * np.pi + (np.arange(FAN[1]) + 0.5) * (np.pi / FAN[1])
    a, e = np.meshgrid(az, el, indexing="ij")
    return np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=-1).reshape(-1, 3)


def poses_along(route, n):
    seg = np.linalg.norm(np.diff(route, axis=0), axis=1)
    s = np.concatenate([[0.0], np.cumsum(seg)])
    at = np.linspace(0.0, s[-1], n)
    return np.stack([np.interp(at, s, route[:, c]) for c in range(3)], axis=1)


def collisions(truth, path):
    """(samples of the polyline `path` in an occupied voxel of `truth`, samples): one every quarter voxel."""
    seg = np.diff(path, axis=0)
    n = np.maximum(1, np.ceil(np.linalg.norm(seg, axis=1) / (0.25 * SCALE)).astype(int))
    samples = np.concatenate([path[i] + np.linspace(0.0, 1.0, n[i] + 1)[:, None] * seg[i] for i in range(len(seg))])
    return int(truth.query(samples).sum()), len(samples)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=24)
    args = ap.parse_args()
    route = forest_route()
    goal = route[-1]
    truth = aa.VoxelMap(SIZE, ORIGIN, SCALE)
    truth.setOccupiedCloud(forest_cloud(np.random.default_rng(17), n_points=1_000_000, clear_route=route).tobytes(), 16)
    truth_occ = truth.voxels_dev != 0
    om = aa.OccupancyMap(SIZE, ORIGIN, SCALE, aa.occupancy_params(max_range=MAX_RANGE))
    vm = aa.VoxelMap(SIZE, ORIGIN, SCALE)
    dirs = torch.from_numpy(fan_directions()).to(om.device)
    reach = 1.5 * MAX_RANGE
    bad_all = n_all = 0
    print(f"{int(truth_occ.sum().item())} occupied voxels in the truth map; {dirs.shape[0]} rays per scan, max_range {MAX_RANGE} m")
    for k, pose in enumerate(poses_along(route, args.poses)):
        t0 = time.perf_counter()
        o = torch.from_numpy(pose).to(om.device).expand(dirs.shape[0], 3).contiguous()
        q = o + reach * dirs
        voxel, t = aa.voxel_raycast_dev(truth, truth.voxels_dev, o, q)
        hit = voxel >= 0
        # the return: the entry point of the blocked voxel, nudged into it; no return: the far end (truncated, carves only)
        t = torch.where(hit, t + 1e-6 * SCALE / reach, torch.ones_like(t))
        om.integrate(o + t[:, None] * (q - o), pose)
        om.to_voxel_map(occ=0, unknown="blocked", dilate=1, out=vm)
        cost, path = aa.plan_path(pose, goal, None, None, vm)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if len(path) > 1:
            b, n = collisions(truth, path)
            bad_all, n_all = bad_all + b, n_all + n
        L = om.logodds_dev()
        known = L != aa.occupancy.UNKNOWN
        held_free = int((truth_occ & known & (L < 0)).sum().item())
        held_occ = int((~truth_occ & known & (L >= 0)).sum().item())
        length = float(np.linalg.norm(np.diff(path, axis=0), axis=1).sum()) if len(path) > 1 else 0.0
        to_goal = float(np.linalg.norm(path[-1] - goal)) if len(path) else float("nan")
        print(f"scan {k:2d} at ({pose[0]:6.2f}, {pose[1]:6.2f}, {pose[2]:4.2f}): known {100.0 * om.known_fraction():5.2f} %, "
              f"{int(hit.sum().item()):5d} returns, occupied held free {held_free}, free held occupied {held_occ}, "
              f"route {length:6.2f} m in {len(path)} points, ends {to_goal:5.2f} m from the goal, {1e3 * dt:.1f} ms")
    # the map of the last scan: the route from the first pose to the goal through what the flight has seen, against the TRUTH
    cost, path = aa.plan_path(route[0], goal, None, None, vm)
    if len(path) < 2:
        print("no route from the first pose on the last map")
        return 1
    bad, n = collisions(truth, path)
    length = float(np.linalg.norm(np.diff(path, axis=0), axis=1).sum())
    print(f"last map: route from the first pose {length:.2f} m in {len(path)} points, ends {np.linalg.norm(path[-1] - goal):.2f} m from the "
          f"goal; {n} samples against the truth map, {bad} in an occupied voxel; the routes of all scans: {bad_all} of {n_all}")
    return 0 if bad == 0 and bad_all == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
