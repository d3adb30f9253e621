#!/usr/bin/env python3
"""A fleet planned in one batch, checked against itself: every pair of trajectories, the exact smallest distance over the time
both are flying (allocnet_amd.traj_separation), beside what sampling both on a time grid reports.

    python examples/fleet_check.py [--fleet 64] [--min-dist 0.6]     # needs a GPU

Vehicles cross a 20 m square at staggered start times.  A vehicle that has not started, or has landed, is not there: to keep it
as an obstacle at its start or goal, prepend or append a constant piece (see the `hold` option below).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import allocnet_amd as aa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleet", type=int, default=64)
    ap.add_argument("--min-dist", type=float, default=0.6)
    ap.add_argument("--hold", type=float, default=0.0, help="seconds a vehicle stays at its goal after arriving")
    args = ap.parse_args()
    B, N, s = args.fleet, 4, 3
    rng = np.random.default_rng(5)
    ang = rng.uniform(0.0, 2.0 * np.pi, B)
    start = np.stack([10.0 * np.cos(ang), 10.0 * np.sin(ang), rng.uniform(1.0, 3.0, B)], axis=1)
    goal = -start * np.array([1.0, 1.0, -1.0]) + rng.normal(size=(B, 3)) * 0.5
    frac = np.linspace(0.0, 1.0, N + 1)[None, :, None]
    pts = start[:, None] * (1.0 - frac) + goal[:, None] * frac + rng.normal(size=(B, N + 1, 3)) * np.array([0.8, 0.8, 0.2]) * (frac * (1 - frac) > 0)
    head, tail = np.zeros((B, 3, 3)), np.zeros((B, 3, 3))
    head[:, :, 0], tail[:, :, 0] = pts[:, 0], pts[:, -1]
    T = np.linalg.norm(np.diff(pts, axis=1), axis=2) / 2.0 + 0.3
    co, _ = aa.minco_solve(head, tail, pts[:, 1:-1], T, s)
    t0 = rng.uniform(0.0, 4.0, B)
    if args.hold > 0.0:                                   # a constant piece at the goal
        rest = np.zeros((B, 1, 3, 2 * s))
        rest[:, 0, :, -1] = pts[:, -1]
        co, T = np.concatenate([co, rest], axis=1), np.concatenate([T, np.full((B, 1), args.hold)], axis=1)
    sep, t, pieces, pairs = aa.traj_separation(co, T, t0=t0)                                 # every a < b, cutoff off
    near, _, _, _ = aa.traj_separation(co, T, t0=t0, cutoff=np.nextafter(args.min_dist, np.inf))
    bad = np.flatnonzero(~(near >= args.min_dist))
    assert np.array_equal(bad, np.flatnonzero(~(sep >= args.min_dist)))
    print(f"{B} vehicles, {len(pairs)} pairs, {np.isfinite(sep).sum()} share some time; closest approach {sep.min():.4f} m")
    print(f"{len(bad)} pairs come closer than {args.min_dist} m:")
    for p in bad[np.argsort(sep[bad])][:10]:
        a, b = pairs[p]
        print(f"  vehicles {a} and {b}: {sep[p]:.4f} m at t = {t[p]:.3f} s (pieces {pieces[p, 0]} and {pieces[p, 1]})")
    # what sampling reports: both on a grid of 0.1 s
    grid = np.arange(0.0, float((t0 + T.sum(axis=1)).max()), 0.1)
    local = grid[None] - t0[:, None]
    live = (local >= 0.0) & (local <= T.sum(axis=1)[:, None])
    pos = aa.traj_eval(co, T, np.clip(local, 0.0, T.sum(axis=1)[:, None]), 0)
    worst = 0.0
    for p in bad:
        a, b = pairs[p]
        both = live[a] & live[b]
        if both.any():
            worst = max(worst, float(np.linalg.norm(pos[a, both] - pos[b, both], axis=1).min()) - sep[p])
    print(f"sampled every 0.1 s, the closest approach of those pairs is overestimated by up to {worst:.4f} m")
    return 0


if __name__ == "__main__":
    sys.exit(main())
