"""The yaw term on the MI355X (csrc/yaw_kernels.h) beside its sibling, the stop term (csrc/stop_kernels.h), on the trajectories of
tools/bench_stop_penalty.py (B x 8 snap pieces x 20 samples, random walks on the launch-file map) with a yaw of order 2 through the
tangent headings of the waypoints.  Steps:
  penalty_131072  anet_minco_yaw_partial_grads_dev (k_minco_yaw<4,2>) and, alternating with it in the same process,
  penalty_4096    anet_minco_stop_partial_grads_dev (k_minco_stop<4>) on the same position trajectories
  margin_131072   anet_traj_yaw_margin_dev on the same trajectories (21 samples per piece)
  scalar_131072   anet_minco_solve_scalar_dev and anet_minco_propagate_grad_scalar_dev (order 2, 8 pieces) beside the three-axis
                  anet_minco_solve_dev and anet_minco_propagate_grad_dev (order 4) of the same batch
Each step runs in a child process under its own `timeout -k 10`.  Device times are events around one call after 5 warm-ups; a step
repeats the whole measurement --runs times, alternating the kernels, and reports per kernel the median of the runs' medians and
the spread (max - min of the runs' medians) next to it.  Prints one JSON line.

    python tools/bench_yaw_penalty.py [--reps 20] [--runs 5] [--step NAME]
"""
import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_voxel_distance import RES, events_ms, forest_map  # noqa: E402
from bench_stop_penalty import A_BRAKE, SPEED_EPS, T_REACT, summary  # noqa: E402

STEPS = ["penalty_4096", "penalty_131072", "margin_131072", "scalar_131072"]
HALF_FOV, MAX_RATE, SY = math.radians(35.0), 1.0, 2


def problem(B, N=8, s=4):
    """the random walks of bench_stop_penalty.trajectories, solved to snap pieces, and the yaw through the tangent headings of their
    waypoints: batch-minor device tensors"""
    import torch
    import allocnet_amd as aa
    rng = np.random.default_rng(11)
    pts = np.empty((B, N + 1, 3))
    pts[:, 0] = rng.uniform([-18.0, -18.0, 0.5], [18.0, 18.0, 4.0], (B, 3))
    for i in range(N):
        step_ = rng.normal(size=(B, 3)) * np.array([1.0, 1.0, 0.2])
        pts[:, i + 1] = np.clip(pts[:, i] + 2.0 * step_ / np.linalg.norm(step_, axis=1, keepdims=True), [-19.5, -19.5, 0.3], [19.5, 19.5, 4.7])
    head, tail = np.zeros((B, 3, 3)), np.zeros((B, 3, 3))
    head[:, :, 0], tail[:, :, 0] = pts[:, 0], pts[:, -1]
    T = np.linalg.norm(np.diff(pts, axis=1), axis=2) / 1.5 + 0.4
    wps = pts[:, 1:-1]
    co, _ = aa.minco_solve(head, tail, wps, T, s)
    h0, hw, h1 = aa.heading_waypoints(wps, pts[:, 0], pts[:, -1])
    yhead, ytail = np.zeros((B, SY)), np.zeros((B, SY))
    yhead[:, 0], ytail[:, 0] = h0, h1
    cy, _ = aa.minco_solve_scalar(yhead, ytail, hw, T, SY)
    ld = aa.recommended_ld(B)

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a.reshape(B, -1).T)).cuda()
        return torch.cat([t, torch.ones(t.shape[0], ld - B, dtype=torch.float64, device="cuda")], 1).contiguous()
    dev = dict(co=up(co), cy=up(cy), T=up(T), head=up(head), tail=up(tail), wps=up(wps), yhead=up(yhead), ytail=up(ytail), ywps=up(hw))
    return dev, ld, N, s


def alternate(kernels, reps, runs):
    """the per-run medians of every kernel, the kernels alternating inside a run: a drift of the clocks meets all alike"""
    meds = {k: [] for k in kernels}
    for _ in range(runs):
        for k, fn in kernels.items():
            meds[k].append(events_ms(fn, reps)[0])
    return meds


def run_step(step, reps, runs):
    import torch
    import allocnet_amd as aa
    B = int(step.rsplit("_", 1)[1])
    d, ld, N, s = problem(B)
    D, DY = 2 * s, 2 * SY
    ctx = aa.default_context(0)
    new = lambda *shape: torch.zeros(*shape, device="cuda", dtype=torch.float64)
    yaw = aa.make_yaw_penalty(w_look=100.0, mu_look=0.05, half_fov=HALF_FOV, speed_eps=SPEED_EPS, w_rate=100.0, mu_rate=0.05,
                              max_rate=MAX_RATE, w_energy=0.01, res=RES)
    out = dict(trajectories=B, pieces=N, order=s, yaw_order=SY, res=RES, reps=reps, runs=runs)
    if step.startswith("margin"):
        m, t, r = new(N, ld), new(N, ld), new(N, ld)
        kernel = lambda: aa.traj_yaw_margin_dev(yaw, 0.2, s, SY, N, B, d["co"], d["cy"], d["T"], m, t, r, ctx=ctx)
        out["margin"] = summary([events_ms(kernel, reps)[0] for _ in range(runs)])
        out["samples"] = B * N * (RES + 1)
        out["margin"]["samples_per_s"] = out["samples"] / (out["margin"]["median_ms"] * 1e-3)
        torch.cuda.synchronize()
        out["negative_margins"] = int((m[:, :B] < 0.0).sum())
        return out
    if step.startswith("scalar"):
        cy, en, co3, en3 = new(N * DY, ld), new(ld), new(N * 3 * D, ld), new(ld)
        gdCy, gdC3, gdT = torch.ones(N * DY, ld, device="cuda", dtype=torch.float64), torch.ones(N * 3 * D, ld, device="cuda", dtype=torch.float64), new(N, ld)
        gPy, gTy, gP3, gT3 = new(N - 1, ld), new(N, ld), new(3 * (N - 1), ld), new(N, ld)
        p = lambda x: x.data_ptr()
        st = torch.cuda.current_stream().cuda_stream
        kernels = {
            "solve_scalar": lambda: aa.minco_solve_scalar_dev(d["yhead"], d["ytail"], d["ywps"], d["T"], SY, SY, N, B, cy, en, ctx=ctx),
            "solve_three_axes": lambda: aa.minco_solve_dev(d["head"], d["tail"], d["wps"], d["T"], s, 3, N, B, coeffs=co3, energy=en3, ctx=ctx),
            "propagate_scalar": lambda: aa.minco_propagate_grad_scalar_dev(d["T"], d["cy"], gdCy, None, SY, SY, N, B, gPy, gTy, ctx=ctx),
            "propagate_three_axes": lambda: ctx.check(ctx.lib.anet_minco_propagate_grad_dev(
                ctx.handle, s, 3, N, B, ld, p(d["T"]), p(d["co"]), p(gdC3), p(gdT), p(gP3), p(gT3), st)),
        }
        meds = alternate(kernels, reps, runs)
        torch.cuda.synchronize()
        for k in kernels:
            out[k] = summary(meds[k])
        return out
    vm = forest_map()
    sd2 = vm.distance_field()
    stop = aa.make_stop_penalty(w=100.0, smooth_mu=0.05, clearance=0.5, a_brake=A_BRAKE, t_react=T_REACT, speed_eps=SPEED_EPS, res=RES)
    ybuf = (new(N * 3 * D, ld), new(N * DY, ld), new(N, ld), new(N, ld))
    sbuf = (new(N * 3 * D, ld), new(N, ld), new(N, ld))
    kernels = {
        "yaw": lambda: aa.minco_yaw_partial_grads_dev(yaw, s, SY, N, B, d["co"], d["cy"], d["T"], *ybuf, ctx=ctx),
        "stop": lambda: aa.minco_stop_partial_grads_dev(stop, s, N, B, d["co"], d["T"], (vm, sd2), *sbuf, ctx=ctx),
    }
    meds = alternate(kernels, reps, runs)
    torch.cuda.synchronize()
    samples = B * N * RES
    for k, pc in (("yaw", ybuf[3]), ("stop", sbuf[2])):
        out[k] = summary(meds[k])
        out[k]["samples_per_s"] = samples / (out[k]["median_ms"] * 1e-3)
        out[k]["cost"] = float(pc[:, :B].sum())
        out[k]["active_pieces"] = int((pc[:, :B] > 0.0).sum())
    out["samples"] = samples
    out["yaw_over_stop"] = out["yaw"]["median_ms"] / out["stop"]["median_ms"]
    out["yaw_over_stop_per_run"] = [float(a / b) for a, b in zip(meds["yaw"], meds["stop"])]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--step", default=None, help="one of %s" % STEPS)
    args = ap.parse_args()
    if args.step:
        print(json.dumps(run_step(args.step, args.reps, args.runs)))
        return 0
    out = {}
    for step in STEPS:
        res = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--step", step, "--reps",
                              str(args.reps), "--runs", str(args.runs)], capture_output=True, text=True)
        if res.returncode != 0:                         # nothing more is started on the device after a step that hung or failed
            out[step] = dict(error=f"exit status {res.returncode}" + (" (time limit)" if res.returncode in (124, 137) else ""),
                             stderr=res.stderr[-800:])
            break
        out[step] = json.loads(res.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return 0 if all("error" not in v for v in out.values()) and len(out) == len(STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
