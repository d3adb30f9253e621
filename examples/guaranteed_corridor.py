#!/usr/bin/env python3
"""The same corridor problems solved with the rows at samples (the reference's form) and on Bernstein control values
(rows="control_points"), with the EXACT margins of both: how far each solution leaves its corridor or exceeds a box for some t.

A sample-form solution is only held at its samples and typically bulges out between them; a control-point solution cannot (the
piece lies in the hull of its control values), at the price of a smaller feasible set -- a somewhat higher cost, and a few more
problems reported infeasible.  More segments per piece (segments=2) give part of that back.

    python examples/guaranteed_corridor.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import allocnet_amd as aa  # noqa: E402
from allocnet_amd.synth import qp_corridor_problem  # noqa: E402


def main():
    order, N, M, B = 4, 5, 12, 8
    vmax, amax = 3.0, 4.0
    rng = np.random.default_rng(3)
    probs = [qp_corridor_problem(rng, N, M) for _ in range(B)]
    ini, fin, hp, T = (np.array([p[q] for p in probs]) for q in range(4))
    forms = [("samples, res 20", dict(res=20)),
             ("samples, res 8", dict(res=8)),
             ("control points, 1 segment", dict(res=aa.qp.control_point_res(order, 1), rows="control_points")),
             ("control points, 2 segments", dict(res=aa.qp.control_point_res(order, 2), rows="control_points"))]
    print(f"{B} problems, {N} snap pieces, {M} corridor rows per piece, |v| <= {vmax}, |a| <= {amax} per axis")
    print(f"{'form':28s} {'rows':>6s} {'solved':>6s} {'steps':>6s} {'cost (median)':>14s} {'corridor':>10s} {'vel box':>10s} {'acc box':>10s}")
    for name, kw in forms:
        out = aa.qp_solve(order, ini, fin, hp, T, max_vel=vmax, max_acc=amax, **kw)
        ok = out["status"] == 1
        corridor, vel, acc = (m[ok].max() if ok.any() else float("nan") for m in aa.traj_qp_margins(out["coeffs"], T, hp, vmax, amax))
        print(f"{name:28s} {N * kw['res'] * (M + 12):6d} {int(ok.sum()):6d} {out['iters'][ok].mean():6.1f} {np.median(out['obj'][ok]):14.4f} "
              f"{corridor:10.2e} {vel:10.2e} {acc:10.2e}")
    print("margins: the worst over the solved problems, all pieces and ALL t of  a.p(t) - b,  |v_axis(t)| - max_vel,  |a_axis(t)| - max_acc;")
    print("positive = outside.  The control-point rows keep every margin at or below the solver's primal residual.")


if __name__ == "__main__":
    main()
