"""The stop-within-known-space term on the MI355X (csrc/stop_kernels.h) on the launch-file map of tools/bench_voxel_distance.py
(400 x 400 x 50 voxels of 0.1 m, a forest cloud of ~1e6 points, dilate(2)) and its trajectories (B x 8 snap pieces x 20 samples).
Steps:
  penalty_131072  anet_minco_stop_partial_grads_dev beside anet_minco_obstacle_partial_grads_dev on the same trajectories and field
  penalty_4096    in the same process: the obstacle kernel issues the same eight loads and square roots per sample, the stop term
                  adds the second Horner derivative, G and a second source per coefficient row
  margin_131072   anet_traj_stop_margin_dev on the same trajectories (21 samples per piece)
Each step runs in a child process under its own `timeout -k 10`.  Device times are events around one call after 5 warm-ups; a step
repeats the whole measurement --runs times, alternating the kernels, and reports per kernel the median of the runs' medians and
the spread (max - min of the runs' medians) next to it.  Prints one JSON line.

    python tools/bench_stop_penalty.py [--reps 20] [--runs 5] [--step NAME]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_voxel_distance import RES, events_ms, forest_map  # noqa: E402

STEPS = ["penalty_4096", "penalty_131072", "margin_131072"]
A_BRAKE, T_REACT, SPEED_EPS = 5.0, 0.1, 1e-2


def trajectories(B, N=8, s=4):
    """the random walks of bench_voxel_distance.run_penalty, solved to snap pieces: batch-minor device tensors"""
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
    co, _ = aa.minco_solve(head, tail, pts[:, 1:-1], T, s)
    ld = aa.recommended_ld(B)

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a.reshape(B, -1).T)).cuda()
        return torch.cat([t, torch.ones(t.shape[0], ld - B, dtype=torch.float64, device="cuda")], 1).contiguous()
    return up(co), up(T), ld, N, s


def summary(runs):
    """runs: the per-run medians in ms"""
    return dict(median_ms=float(np.median(runs)), spread_ms=float(np.max(runs) - np.min(runs)), runs_ms=[float(r) for r in runs])


def run_step(step, reps, runs):
    import torch
    import allocnet_amd as aa
    B = int(step.rsplit("_", 1)[1])
    vm = forest_map()
    sd2 = vm.distance_field()
    d_co, d_T, ld, N, s = trajectories(B)
    D = 2 * s
    ctx = aa.default_context(0)
    new = lambda *shape: torch.zeros(*shape, device="cuda", dtype=torch.float64)
    stop = aa.make_stop_penalty(w=100.0, smooth_mu=0.05, clearance=0.5, a_brake=A_BRAKE, t_react=T_REACT, speed_eps=SPEED_EPS, res=RES)
    out = dict(trajectories=B, pieces=N, order=s, res=RES, reps=reps, runs=runs)
    if step.startswith("margin"):
        m, t, sp, dd = new(N, ld), new(N, ld), new(N, ld), new(N, ld)
        kernel = lambda: aa.traj_stop_margin_dev(stop, s, N, B, d_co, d_T, (vm, sd2), m, t, sp, dd, ctx=ctx)
        out["margin"] = summary([events_ms(kernel, reps)[0] for _ in range(runs)])
        out["samples"] = B * N * (RES + 1)
        out["margin"]["samples_per_s"] = out["samples"] / (out["margin"]["median_ms"] * 1e-3)
        torch.cuda.synchronize()
        out["negative_margins"] = int((m[:, :B] < 0.0).sum())
        return out
    obs = aa.make_obstacle_penalty(w=100.0, smooth_mu=0.05, clearance=0.5, res=RES)
    bufs = {k: (new(N * 3 * D, ld), new(N, ld), new(N, ld)) for k in ("stop", "obstacle")}
    kernels = {
        "stop": lambda: aa.minco_stop_partial_grads_dev(stop, s, N, B, d_co, d_T, (vm, sd2), *bufs["stop"], ctx=ctx),
        "obstacle": lambda: aa.minco_obstacle_partial_grads_dev(obs, s, N, B, d_co, d_T, (vm, sd2), *bufs["obstacle"], ctx=ctx),
    }
    meds = {k: [] for k in kernels}
    for _ in range(runs):                                                # alternating: a drift of the clocks meets both alike
        for k, fn in kernels.items():
            meds[k].append(events_ms(fn, reps)[0])
    torch.cuda.synchronize()
    samples = B * N * RES
    for k in kernels:
        out[k] = summary(meds[k])
        out[k]["samples_per_s"] = samples / (out[k]["median_ms"] * 1e-3)
        out[k]["cost"] = float(bufs[k][2][:, :B].sum())
        out[k]["active_pieces"] = int((bufs[k][2][:, :B] > 0.0).sum())
    out["samples"] = samples
    out["stop_over_obstacle"] = out["stop"]["median_ms"] / out["obstacle"]["median_ms"]
    out["stop_over_obstacle_per_run"] = [float(a / b) for a, b in zip(meds["stop"], meds["obstacle"])]
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
