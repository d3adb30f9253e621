#!/usr/bin/env python3
"""Exploration that chooses its own route, all of it on the MI355X -- the setting of examples/map_from_scans.py (the same synthetic
forest, map and sensor), but nobody hands the sensor a route:

    scan -> OccupancyMap.to_voxel_map(unknown="blocked") -> frontier_clusters (frontier mask, components, table)
    -> candidate_views (rings around the clusters, reachable by the component label of the free bytes) -> view_gain
    -> utility gain * exp(-lambda * route length) -> plan_path to the best pose -> fly it, scanning at intervals

until no cluster of min_size can be reached or the pose budget is spent.  Printed per pose: the known fraction next to what the
preset route of map_from_scans.py had reached after as many scans, the number of clusters and candidates, the gain the winner
promised and what the scan from there revealed; at the end the number of poses and that no truly occupied voxel is held free.

    python examples/explore_forest.py [--poses N]   # needs a GPU
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import allocnet_amd as aa  # noqa: E402
from allocnet_amd.synth import forest_cloud, forest_route  # noqa: E402
from map_from_scans import SIZE, ORIGIN, SCALE, MAX_RANGE, fan_directions, poses_along  # noqa: E402

MIN_SIZE = 12        # frontier voxels a cluster needs to count
SCAN_EVERY = 3.0     # metres of route between two scans on the way to a goal


class Sensor:
    """The sensor of map_from_scans.py: a fan of segments of 1.5 max_range against the truth map."""

    def __init__(self, truth, om):
        import torch
        self.truth, self.om = truth, om
        self.dirs = torch.from_numpy(fan_directions()).to(om.device)
        self.reach = 1.5 * MAX_RANGE
        self.template = self.reach * self.dirs          # the same fan in the sensor frame: what view_gain walks

    def scan(self, pose):
        import torch
        o = torch.from_numpy(np.ascontiguousarray(pose)).to(self.om.device).expand(self.dirs.shape[0], 3).contiguous()
        q = o + self.reach * self.dirs
        voxel, t = aa.voxel_raycast_dev(self.truth, self.truth.voxels_dev, o, q)
        t = torch.where(voxel >= 0, t + 1e-6 * SCALE / self.reach, torch.ones_like(t))
        self.om.integrate(o + t[:, None] * (q - o), pose)


def explore(truth, om, start, budget, sensor=None, log=print):
    """-> (poses scanned from, known fraction after each)."""
    sensor = sensor or Sensor(truth, om)
    vm = aa.VoxelMap(SIZE, ORIGIN, SCALE)
    pose = np.asarray(start, dtype=np.float64)
    poses, known = [], []

    def scan(p, note):
        before = om.known_fraction()
        sensor.scan(p)
        poses.append(p.copy()); known.append(om.known_fraction())
        log(f"pose {len(poses):2d} at ({p[0]:6.2f}, {p[1]:6.2f}, {p[2]:4.2f}): known {100 * known[-1]:5.2f} % "
            f"(+{round((known[-1] - before) * om._n):6d} voxels) {note}")

    scan(pose, "start")
    while len(poses) < budget:
        om.to_voxel_map(occ=0, unknown="blocked", out=vm)
        nv = aa.next_view(om, vm, pose, sensor.template, occ=0, min_size=MIN_SIZE, connectivity=26, radii=(1.0, 2.5), n_yaw=8,
                          height=pose[2], lam=0.15)
        if len(nv["order"]) == 0 or nv["utility"][nv["order"][0]] <= 0.0:
            log(f"no reachable frontier cluster of {MIN_SIZE} voxels is left ({len(nv['clusters']['root'])} clusters in all)")
            break
        best = int(nv["order"][0])
        goal = nv["t"][best]
        cost, path = aa.plan_path(pose, goal, None, None, vm)
        if len(path) < 2:
            log("the best pose has no route: stopping")
            break
        note = (f"{len(nv['clusters']['root'])} clusters, {len(nv['t'])} candidates, promised {int(nv['gain'][best])} voxels, "
                f"route {cost:.2f} m")
        # fly the route, scanning every SCAN_EVERY metres and at its end
        seg = np.linalg.norm(np.diff(path, axis=0), axis=1)
        s = np.concatenate([[0.0], np.cumsum(seg)])
        stops = list(np.arange(SCAN_EVERY, s[-1] - 0.5 * SCAN_EVERY, SCAN_EVERY)) + [s[-1]]
        for k, at in enumerate(stops):
            if len(poses) >= budget:
                break
            pose = np.array([np.interp(at, s, path[:, c]) for c in range(3)])
            scan(pose, note if k == len(stops) - 1 else "on the way")
    return np.asarray(poses), np.asarray(known)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=24)
    args = ap.parse_args()
    route = forest_route()
    truth = aa.VoxelMap(SIZE, ORIGIN, SCALE)
    truth.setOccupiedCloud(forest_cloud(np.random.default_rng(17), n_points=1_000_000, clear_route=route).tobytes(), 16)
    truth_occ = truth.voxels_dev != 0
    prm = aa.occupancy_params(max_range=MAX_RANGE)
    # the preset route of map_from_scans.py, for comparison
    preset = aa.OccupancyMap(SIZE, ORIGIN, SCALE, prm)
    sensor = Sensor(truth, preset)
    preset_known = []
    for p in poses_along(route, args.poses):
        sensor.scan(p)
        preset_known.append(preset.known_fraction())
    om = aa.OccupancyMap(SIZE, ORIGIN, SCALE, prm)
    poses, known = explore(truth, om, route[0], args.poses, Sensor(truth, om))
    print("\nposes  explored  preset route")
    for k in range(len(known)):
        print(f"{k + 1:5d}  {100 * known[k]:7.2f} %  {100 * preset_known[k]:7.2f} %")
    L = om.logodds_dev()
    held_free = int((truth_occ & (L != aa.occupancy.UNKNOWN) & (L < 0)).sum().item())
    print(f"{len(poses)} poses; truly occupied voxels held free: {held_free}")
    return 0 if held_free == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
