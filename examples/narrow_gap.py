#!/usr/bin/env python3
"""A plate through a slot narrower than its span: the whole-body corridor penalty lets the vehicle roll to pass.

    python examples/narrow_gap.py [--rounds 4] [--weight 2e4]     # needs a GPU

The corridor is three polytopes along x.  The middle one is a slab tilted about x by 40 degrees with half-width 0.12 m; the body is a
plate with half extents 0.25 x 0.25 x 0.05 m.  Along the slab's normal the plate reaches 0.25 sin 40 + 0.05 cos 40 = 0.20 m when it
is level and 0.05 m when it is rolled to 40 degrees, so a level plate does not fit and a rolled one does -- and a vehicle only
rolls by accelerating sideways, so the trajectory has to swing through the slot (sliding down the incline at g sin 40 keeps the
thrust along the slab's normal).  No dilation of the map expresses this.

First the point solution: the body is one vertex at the origin, which is the point-corridor penalty.  From there the plate:
allocnet_amd.body_objective_dev (energy + rho * time + J_body, gradients through the flatness map's adjoint) under the lockstep
L-BFGS allocnet_amd.lbfgs_optimize_dev on the waypoints and log durations, restarted a few times.  Printed: the worst sampled body
margin (allocnet_amd.traj_body_margin; positive = outside) before and after, and the largest tilt reached.  The penalty is soft and
sampled; this is a demonstration and checks no number.  With one snap piece per polytope the optimiser has nine variables: on an
MI355X it lowers J_body and raises the tilt in the slot (13 -> 23 degrees) but leaves the plate 0.11 m outside at its worst sample
(0.12 m before); more pieces per polytope, or a start that already swings, are what a planner would add.
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import allocnet_amd as aa  # noqa: E402


def box(lo, hi):
    """rows a.x <= b of the axis-aligned box [lo, hi]"""
    r = np.zeros((6, 4))
    for ax in range(3):
        r[2 * ax, ax], r[2 * ax, 3] = 1.0, hi[ax]
        r[2 * ax + 1, ax], r[2 * ax + 1, 3] = -1.0, -lo[ax]
    return r


def slab(x_lo, x_hi, centre, angle, half_width, half_span):
    """x in [x_lo, x_hi], |n.(x - c)| <= half_width, |u.(x - c)| <= half_span with n = Rx(angle) e3, u = Rx(angle) e2"""
    n = np.array([0.0, -math.sin(angle), math.cos(angle)])
    u = np.array([0.0, math.cos(angle), math.sin(angle)])
    r = np.zeros((6, 4))
    r[0, 0], r[0, 3] = 1.0, x_hi
    r[1, 0], r[1, 3] = -1.0, -x_lo
    for k, (d, w) in enumerate(((n, half_width), (u, half_span))):
        r[2 + 2 * k, :3], r[2 + 2 * k, 3] = d, d @ centre + w
        r[3 + 2 * k, :3], r[3 + 2 * k, 3] = -d, -(d @ centre) + w
    return r


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--weight", type=float, default=2e4)
    args = ap.parse_args()
    B, N, s, c, res = 1, 3, 4, 3, 40
    angle = math.radians(40.0)
    centre = np.array([3.0, 0.0, 1.5])
    # consecutive polytopes overlap by 1.2 m, more than the plate's reach: a sample of piece i is tested against polytope i only
    hp = np.stack([box((-0.6, -1.5, 0.3), (2.6, 1.5, 2.7)), slab(1.4, 4.6, centre, angle, 0.12, 1.5),
                   box((3.4, -1.5, 0.3), (6.6, 1.5, 2.7))])[None]                           # (1, 3, 6, 4)
    plate = aa.box_body((0.25, 0.25, 0.05))
    point = np.zeros((1, 3))
    fm = aa.FlatnessMap()
    head, tail = np.zeros((B, 3, c)), np.zeros((B, 3, c))
    head[0, :, 0], tail[0, :, 0] = (0.0, 0.0, 1.5), (6.0, 0.0, 1.5)
    wps = np.array([[[2.0, 0.0, 1.5], [4.0, 0.0, 1.5]]])
    T = np.full((B, N), 1.5)
    pen = aa.make_penalty(rho=10.0, res=res)                                               # energy + rho * time; the corridor is J_body's
    dev = torch.device("cuda", aa.default_context().device)
    ld, nw = 1, 3 * (N - 1)

    def up(a):     # (B, fields) -> batch-minor (fields, ld)
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(B, -1)
        t = torch.zeros(a.shape[1], ld, device=dev, dtype=torch.float64)
        t[:, :B] = torch.from_numpy(a).to(dev).T
        return t

    def report(tag, w, t):
        co, _ = aa.minco_solve(head, tail, w, t, s)
        mp = aa.traj_body_margin(fm, point, co, t, hp, res)[0].max()
        mb, tt, row, vert = aa.traj_body_margin(fm, plate, co, t, hp, res)
        i = int(np.argmax(mb[0]))
        tilt = aa.traj_flat_extrema(fm, co, t, res)[0, 2]
        print(f"{tag}: worst margin of the point {mp:+.3f} m, of the plate {mb.max():+.3f} m (piece {i}, t = {tt[0, i]:.2f} s, row "
              f"{row[0, i]}, vertex {vert[0, i]}); largest tilt {math.degrees(tilt):.1f} deg; durations {np.round(t[0], 2).tolist()}")
        return mb.max()

    def optimise(body, w, t, rounds, tag):
        bpen = aa.make_body_penalty(body, w=args.weight, smooth_mu=0.02, res=res, poly_rows=hp.shape[2])
        x = up(np.concatenate([w.reshape(B, -1), np.log(t)], axis=1))
        objective = aa.body_objective_dev(up(head), up(tail), s, c, N, B, fm, bpen, up(hp), penalty=pen)
        for rnd in range(rounds):
            out = aa.lbfgs_optimize_dev(x, objective, batch=B, param=aa.lbfgs_parameter_t(past=3, delta=1e-7), max_evals=800)
            torch.cuda.synchronize()
            w = x[:nw, :B].T.cpu().numpy().reshape(B, N - 1, 3)
            t = np.exp(x[nw:, :B].T.cpu().numpy())
            print(f"  {tag} round {rnd + 1}: status {int(out['status'][0])}, {int(out['evals'][0])} evaluations, J = {float(out['f'][0]):.4g}")
        return w, t

    report("start (straight line)", wps, T)
    wps, T = optimise(point, wps, T, 1, "point")
    before = report("point-corridor solution", wps, T)
    wps, T = optimise(plate, wps, T, args.rounds, "plate")
    after = report("with the whole-body penalty", wps, T)
    print(f"worst body margin {before:+.3f} m -> {after:+.3f} m")
    return 0


if __name__ == "__main__":
    sys.exit(main())
