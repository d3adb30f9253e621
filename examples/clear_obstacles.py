#!/usr/bin/env python3
"""A batch of straight trajectories pushed out of a forest by the map's own distance field -- no route search, no corridor.

    python examples/clear_obstacles.py [--batch 64] [--clearance 0.4] [--trees 40] [--rounds 3]     # needs a GPU

A synthetic forest of solid trunks is set into a VoxelMap voxel by voxel and dilated by one voxel (solid: a scan fills only the
shell of a trunk, and a field has a free pocket inside a shell).  Every trajectory starts as a straight rest-to-rest line across
it.  The exact distance field of the map (VoxelMap.distance_field) then enters the MINCO objective as a penalty
(allocnet_amd.obstacle_objective_dev), and the lockstep L-BFGS (allocnet_amd.lbfgs_optimize_dev) moves the waypoints and log
durations of ALL trajectories at once, restarted a few times.  Before and after, the exact tools answer: the first collision with the map
(allocnet_amd.traj_first_collision) and the clearance to its surface points (allocnet_amd.traj_clearance).  The penalty is sampled
and soft, the checks are exact.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import allocnet_amd as aa  # noqa: E402


def report(tag, co, T, vm):
    t, _, _ = aa.traj_first_collision(co, T, vm)
    cl = aa.traj_clearance(co, T, vm)[0].min(axis=1)
    free = ~np.isfinite(t)
    rest = f"smallest {cl[free].min():.3f} m, median {np.median(cl[free]):.3f} m" if free.any() else "none is free"
    print(f"{tag}: {int((~free).sum())} of {len(t)} trajectories collide with the map; clearance to its surface over the free ones: {rest}")
    return int((~free).sum())


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--clearance", type=float, default=0.4)
    ap.add_argument("--trees", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    B, N, s, c = args.batch, 8, 3, 3
    size, origin, scale = (200, 200, 40), (-10.0, -10.0, 0.0), 0.1
    rng = np.random.default_rng(3)
    vm = aa.VoxelMap(size, origin, scale)
    # trunks of radius 0.2 .. 0.5 m over the full height, between the start and the goal lines
    centre, radius = rng.uniform(-7.5, 7.5, (args.trees, 2)), rng.uniform(0.2, 0.5, args.trees)
    xy = np.stack(np.meshgrid(np.arange(size[0]), np.arange(size[1]), indexing="ij"), -1).reshape(-1, 2)
    pos = np.array(origin[:2]) + (xy + 0.5) * scale
    inside = (np.linalg.norm(pos[:, None, :] - centre[None, :, :], axis=2) <= radius[None, :]).any(1)
    cols = xy[inside]
    ids = np.concatenate([np.repeat(cols, size[2], axis=0), np.tile(np.arange(size[2]), len(cols))[:, None]], axis=1)
    vm.setOccupied(ids.astype(np.int32))
    vm.dilate(1)
    field = vm.distance_field(walls=True)
    print(f"map {size} at {scale} m: {int((field < 0).sum())} blocked voxels, deepest {scale * float(-field.min()) ** 0.5:.2f} m inside, "
          f"farthest free voxel {scale * float(field.max()) ** 0.5:.2f} m from an obstacle")

    # straight lines west to east at random heights, rest to rest; ends that sit in an obstacle are moved along y until they are free
    y = rng.uniform(-8.5, 8.5, (B, 2))
    z = rng.uniform(1.0, 3.0, (B, 2))
    ends = np.stack([np.stack([np.full(B, -9.0), y[:, 0], z[:, 0]], 1), np.stack([np.full(B, 9.0), y[:, 1], z[:, 1]], 1)], 1)
    for _ in range(50):
        bad = vm.getDistance(ends.reshape(-1, 3)).reshape(B, 2) < args.clearance + 0.2
        if not bad.any():
            break
        ends[..., 1][bad] = rng.uniform(-8.5, 8.5, int(bad.sum()))
    frac = np.linspace(0.0, 1.0, N + 1)[None, :, None]
    pts = ends[:, :1] * (1.0 - frac) + ends[:, 1:] * frac
    head, tail = np.zeros((B, 3, c)), np.zeros((B, 3, c))
    head[:, :, 0], tail[:, :, 0] = pts[:, 0], pts[:, -1]
    wps = pts[:, 1:-1].copy()
    T = np.linalg.norm(np.diff(pts, axis=1), axis=2) / 2.0 + 0.3

    co, _ = aa.minco_solve(head, tail, wps, T, s)
    n0 = report("before", co, T, vm)

    open_ = aa.make_obstacle_penalty(w=2000.0, smooth_mu=0.05, clearance=args.clearance, res=24)
    pen = aa.make_penalty(rho=20.0, res=24)                          # energy + rho * time: no corridor, no limits
    ld = aa.recommended_ld(B)
    dev = vm.device
    nw = 3 * (N - 1)

    def up(a):
        t = torch.zeros(a.shape[1], ld, device=dev, dtype=torch.float64)
        t[:, :B] = torch.from_numpy(np.ascontiguousarray(a)).to(dev).T
        return t
    x = up(np.concatenate([wps.reshape(B, -1), np.log(T)], axis=1))
    objective = aa.obstacle_objective_dev(up(head.reshape(B, -1)), up(tail.reshape(B, -1)), s, c, N, B, vm, open_, penalty=pen)
    n1 = n0
    for rnd in range(args.rounds):                                   # the interpolant has kinks: a restart takes up a stalled search
        res = aa.lbfgs_optimize_dev(x, objective, batch=B, param=aa.lbfgs_parameter_t(past=3, delta=1e-6), max_evals=600)
        torch.cuda.synchronize()
        status = res["status"].cpu().numpy()
        wps = x[:nw, :B].T.cpu().numpy().reshape(B, N - 1, 3)
        T = np.exp(x[nw:, :B].T.cpu().numpy())
        co, _ = aa.minco_solve(head, tail, wps, T, s)
        print(f"round {rnd + 1}: {int(res['evals'].max())} evaluations at most, {int((status >= 0).sum())} of {B} with a status >= 0")
        n1 = report(f"after round {rnd + 1}", co, T, vm)
        if n1 == 0:
            break
    return 0 if n1 < n0 or n0 == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
