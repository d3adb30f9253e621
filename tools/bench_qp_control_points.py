#!/usr/bin/env python3
"""The control-point row form of the inequality QP (ANET_QP_ROWS_CONTROL_POINTS) against the sample form at
res = 20 on the same inputs: 4096 x 8-piece snap and 4096 x 5-piece jerk, interior point, device tensors in and out
(qp_solve_dev: no PCIe in the times).  Per form: device-event time (median of --reps launches after --warmup), Newton steps, share
solved, objective ratio to the sample form (problems both solve), and the EXACT margins of the solved problems (traj_qp_margins:
per problem the largest of corridor / velocity box / acceleration box over its pieces and over all t; positive = left the set).
Prints one JSON object."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import allocnet_amd as aa  # noqa: E402
from allocnet_amd.synth import corridor_problem  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    ctx = aa.Context(0)
    dev = torch.device("cuda", 0)
    vmax, amax, M = 4.0, 6.0, 16
    out = {}
    for (s, N) in [(4, 8), (3, 5)]:
        B = args.batch
        head, tail, wps, T, hp = corridor_problem(np.random.default_rng(1), B, N, 3, M)
        T = T * 1.5
        state = torch.from_numpy(np.ascontiguousarray(np.stack([head, tail], axis=1))).to(dev)
        tT, thp = torch.from_numpy(T.copy()).to(dev), torch.from_numpy(np.ascontiguousarray(hp)).to(dev)
        forms = [("samples_res20", 20, "samples")] + [(f"control_points_k{k}", aa.qp.control_point_res(s, k), "control_points")
                                                      for k in (1, 2)]
        base = None
        for name, res, rows in forms:
            kw = dict(res=res, max_vel=vmax, max_acc=amax, rows=rows, ctx=ctx)
            for _ in range(args.warmup):
                r = aa.qp_solve_dev(s, state, tT, thp, **kw)
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = aa.qp_solve_dev(s, state, tT, thp, **kw)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            status, iters = r["status"].cpu().numpy(), r["iters"].cpu().numpy()
            obj, coeffs = r["obj"].cpu().numpy(), r["coeffs"].cpu().numpy()
            ok = status == 1
            margin = np.max(aa.traj_qp_margins(coeffs, T, hp, vmax, amax, ctx=ctx), axis=(0, 2))      # (B,)
            rows_per_problem = N * res * (M + 12)
            rec = {"res": res, "rows_per_problem": rows_per_problem, "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)),
                   "newton_steps_mean": float(iters.mean()), "newton_steps_max": int(iters.max()), "solved_share": float(ok.mean()),
                   "ns_per_row_and_step": float(np.median(ms) * 1e6 / (rows_per_problem * float(iters.sum()))),
                   "margin_p99": float(np.percentile(margin[ok], 99)), "margin_worst": float(margin[ok].max()),
                   "share_outside_by_1e-6": float((margin[ok] > 1e-6).mean())}
            if base is None:
                base = (ok, obj)
            else:
                both = ok & base[0]
                ratio = obj[both] / base[1][both]
                rec.update(solved_of_sample_solved=float(ok[base[0]].mean()), obj_ratio_median=float(np.median(ratio)),
                           obj_ratio_worst=float(ratio.max()), obj_ratio_min=float(ratio.min()))
            out[f"s{s}_N{N}_B{B}_{name}"] = rec
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
