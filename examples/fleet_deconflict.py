#!/usr/bin/env python3
"""The fleet of examples/fleet_check.py taken one step further: the pairs that come too close are not only listed but removed.

    python examples/fleet_deconflict.py [--fleet 64] [--min-dist 0.6] [--rounds 5]     # needs a GPU

Each round selects the pairs whose exact separation (allocnet_amd.traj_separation) is below a radius, builds the neighbour lists
from them, freezes every vehicle at its current trajectory as an obstacle for the others, and runs the lockstep L-BFGS
(allocnet_amd.lbfgs_optimize_dev) on the waypoints and log durations of ALL vehicles at once, with the trajectory-avoidance
penalty (allocnet_amd.minco_avoid_cost_grad_dev) in the objective.  Start offsets stay as planned.  The penalty keeps a margin
above --min-dist: it is sampled and soft, the check afterwards is exact.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import allocnet_amd as aa  # noqa: E402


def conflicts(co, T, t0, min_dist):
    sep, _, _, pairs = aa.traj_separation(co, T, t0=t0)
    return sep, pairs, int((~(sep >= min_dist)).sum())


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleet", type=int, default=64)
    ap.add_argument("--min-dist", type=float, default=0.6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--margin", type=float, default=1.4, help="the penalty's distance as a multiple of --min-dist")
    args = ap.parse_args()
    B, N, s, c = args.fleet, 4, 3, 3
    rng = np.random.default_rng(5)                                  # the fleet of fleet_check.py
    ang = rng.uniform(0.0, 2.0 * np.pi, B)
    start = np.stack([10.0 * np.cos(ang), 10.0 * np.sin(ang), rng.uniform(1.0, 3.0, B)], axis=1)
    goal = -start * np.array([1.0, 1.0, -1.0]) + rng.normal(size=(B, 3)) * 0.5
    frac = np.linspace(0.0, 1.0, N + 1)[None, :, None]
    pts = start[:, None] * (1.0 - frac) + goal[:, None] * frac + rng.normal(size=(B, N + 1, 3)) * np.array([0.8, 0.8, 0.2]) * (frac * (1 - frac) > 0)
    head, tail = np.zeros((B, 3, c)), np.zeros((B, 3, c))
    head[:, :, 0], tail[:, :, 0] = pts[:, 0], pts[:, -1]
    wps = pts[:, 1:-1].copy()
    T = np.linalg.norm(np.diff(pts, axis=1), axis=2) / 2.0 + 0.3
    t0 = rng.uniform(0.0, 4.0, B)

    co, _ = aa.minco_solve(head, tail, wps, T, s)
    sep, pairs, n0 = conflicts(co, T, t0, args.min_dist)
    print(f"{B} vehicles, {len(pairs)} pairs; before: {n0} pairs closer than {args.min_dist} m, smallest separation {sep.min():.4f} m")

    keep_out = args.margin * args.min_dist
    apen = aa.make_avoid_penalty(w=2000.0, smooth_mu=0.1 * keep_out ** 2, min_dist=keep_out, z_scale=1.0, res=20)
    pen = aa.make_penalty(rho=60.0, res=20)                          # energy + rho * time: no corridor, no limits
    ld = aa.recommended_ld(B)
    dev = torch.device("cuda", 0)
    nw = 3 * (N - 1)

    def up(a):
        t = torch.zeros(a.shape[1], ld, device=dev, dtype=torch.float64)
        t[:, :B] = torch.from_numpy(np.ascontiguousarray(a)).to(dev).T
        return t
    d_head, d_tail, d_t0 = up(head.reshape(B, -1)), up(tail.reshape(B, -1)), torch.from_numpy(t0).to(dev)
    x = up(np.concatenate([wps.reshape(B, -1), np.log(T)], axis=1))
    n = n0
    for rnd in range(args.rounds):
        nbr = aa.neighbours_from_pairs(pairs, B, keep=~(sep >= 2.0 * keep_out))
        if nbr[1].size == 0:
            break
        others = aa.upload_others(co, T, t0)                         # every vehicle where it is now, frozen for this round
        objective = aa.avoid_objective_dev(d_head, d_tail, s, c, N, B, others, apen, nbr, t0=d_t0, penalty=pen)
        res = aa.lbfgs_optimize_dev(x, objective, batch=B, param=aa.lbfgs_parameter_t(past=3, delta=1e-5), max_evals=400)
        torch.cuda.synchronize()
        wps = x[:nw, :B].T.cpu().numpy().reshape(B, N - 1, 3)
        T = np.exp(x[nw:, :B].T.cpu().numpy())
        co, _ = aa.minco_solve(head, tail, wps, T, s)
        sep, pairs, n = conflicts(co, T, t0, args.min_dist)
        status = res["status"].cpu().numpy()
        print(f"round {rnd + 1}: {nbr[1].size // 2} pairs in the lists, {int(res['evals'].max())} evaluations, "
              f"{int((status >= 0).sum())} of {B} converged; {n} pairs closer than {args.min_dist} m, smallest separation {sep.min():.4f} m")
    print(f"after: {n} pairs closer than {args.min_dist} m (before: {n0}), smallest separation {sep.min():.4f} m")
    return 0 if n < n0 or n0 == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
