"""The corridor-constrained MINCO L-BFGS on the MI355X (allocnet_amd/sfc_opt.py), three measurements:

  (a) transform_K16 / transform_K32: k_sfc_forward_p and k_sfc_backward_grad alone at 131 072 problems of 8 pieces, device events,
      medians of --reps after 5 warm-up calls, and the rate against the compulsory bytes per (problem, waypoint):
      forward 8 (4 K) + 8 * 5, backward 8 (4 K + 7) + 8 K;
  (b) step_4096 / step_131072: one lockstep evaluation step of anet_lbfgs_minco_sfc_dev against one of anet_lbfgs_minco_dev with
      OPT_LOCKSTEP, 8-piece snap, the same corridors and penalty (tools/time_lbfgs_step.py's): wall time of a call of 200
      evaluations that ends in a synchronise, over 200, median of three calls after one warm-up call.  The difference is the price of
      the parametrisation plus the larger n in the update kernel;
  (c) plan_5_jerk: one plan (B = 1, 5 jerk pieces) end to end through lbfgs_minco_sfc (enumeration, backward_p, optimisation, host
      staging), wall time, median of --reps after 5 warm-up calls.

Every step runs in a child process of its own under its own time limit; the driver stops at the first step that fails.  Prints one
JSON line.

    python tools/bench_sfc_opt.py [--reps 30] [--step NAME]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ["transform_K16", "transform_K32", "step_4096", "step_131072", "plan_5_jerk"]
LIMIT_S = 420
PEN = dict(rho=50.0, w_corridor=1e4, w_vel=1e3, w_acc=1e3, smooth_mu=1e-2, max_vel=4.0, max_acc=6.0, res=20)


def events_ms(fn, reps, warm=5):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def transform_step(K, reps):
    import torch
    import allocnet_amd as aa
    B, N = 131072, 8
    ld = aa.recommended_ld(B)
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda rows: torch.randn(rows, ld, device="cuda", dtype=torch.float64, generator=g)
    xi, verts, gP = rnd((N - 1) * K) * 0.3, rnd((N - 1) * K * 3) * 5.0, rnd(3 * (N - 1))
    ctx = aa.default_context(0)
    fw = aa.sfc_forward_p_dev(xi, verts, N, B, K, 1.0, ctx=ctx)
    gxi = torch.zeros_like(xi)
    cost = torch.zeros(ld, device="cuda", dtype=torch.float64)
    f_med, f_min = events_ms(lambda: aa.sfc_forward_p_dev(xi, verts, N, B, K, 1.0, wps=fw["wps"], norm=fw["norm"], ctx=ctx), reps)
    b_med, b_min = events_ms(lambda: aa.sfc_backward_grad_p_dev(xi, verts, fw["wps"], fw["norm"], gP, N, B, K, grad_xi=gxi, cost=cost,
                                                                ctx=ctx), reps)
    lanes = B * (N - 1)
    f_bytes, b_bytes = lanes * (8 * 4 * K + 8 * 5), lanes * (8 * (4 * K + 7) + 8 * K)
    return dict(problems=B, pieces=N, max_verts=K, forward_median_ms=f_med, forward_min_ms=f_min, forward_compulsory_bytes=f_bytes,
                forward_GBps=f_bytes / (f_med * 1e-3) / 1e9, backward_median_ms=b_med, backward_min_ms=b_min,
                backward_compulsory_bytes=b_bytes, backward_GBps=b_bytes / (b_med * 1e-3) / 1e9)


def lockstep_step(B):
    import torch
    import allocnet_amd as aa
    from allocnet_amd.sfc_opt import _bm
    from allocnet_amd.synth import corridor_problem
    s, c, N, M, K, evals = 4, 3, 8, 16, 32, 200
    head, tail, wps, T, hp = corridor_problem(np.random.default_rng(2), B, N, c, M)
    pen = aa.make_penalty(poly_rows=M, **PEN)
    ctx = aa.default_context(0)
    th, tt, tw, tT, thp = (_bm(a, B) for a in (head, tail, wps, T, hp))
    ov = aa.sfc_overlap_vertices_dev(thp, N, B, M, K, ctx=ctx)
    bp = aa.sfc_backward_p_dev(ov["verts"], ov["count"], tw, N, B, K, ctx=ctx)
    lock = aa.lbfgs.OPT_WAYPOINTS | aa.lbfgs.OPT_TIMES | aa.lbfgs.OPT_LOCKSTEP

    def wall(fn):
        ts = []
        for rep in range(4):
            args = fn(None)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = fn(args)
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        return float(np.median(ts[1:])), out
    plain_s, plain = wall(lambda a: (tw.clone(), tT.clone()) if a is None else
                          aa.lbfgs_minco_dev(th, tt, a[0], a[1], s, c, N, B, hpolys=thp, penalty=pen, opt=lock, max_evals=evals, ctx=ctx))
    sfc_s, sfc = wall(lambda a: (bp["xi"].clone(), tT.clone()) if a is None else
                      aa.lbfgs_minco_sfc_dev(th, tt, a[0], a[1], ov["verts"], ov["count"], s, c, N, B, K, hpolys=thp, penalty=pen,
                                             max_evals=evals, overlap_status=ov["status"], ctx=ctx))
    ev_p, ev_s = plain["evals"].cpu().numpy(), sfc["evals"].cpu().numpy()
    return dict(problems=B, pieces=N, order=s, max_verts=K, evaluations=evals, plain_variables=3 * (N - 1) + N,
                sfc_variables=(N - 1) * K + N, plain_ms_per_step=plain_s / evals * 1e3, sfc_ms_per_step=sfc_s / evals * 1e3,
                difference_ms_per_step=(sfc_s - plain_s) / evals * 1e3, plain_still_running=float((ev_p == evals).mean()),
                sfc_still_running=float((ev_s == evals).mean()))


def plan_step(reps):
    import allocnet_amd as aa
    from allocnet_amd.synth import corridor_problem
    s, c, N, M = 3, 3, 5, 16
    head, tail, wps, T, hp = corridor_problem(np.random.default_rng(3), 1, N, c, M)
    pen = aa.make_penalty(poly_rows=M, **PEN)
    ctx = aa.default_context(0)
    run = lambda: aa.lbfgs_minco_sfc(head, tail, hp, T, s, wps=wps, penalty=pen, max_evals=2000, ctx=ctx)
    for _ in range(5):
        res = run()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); res = run(); ts.append(time.perf_counter() - t0)
    return dict(pieces=N, order=s, max_verts=res["max_verts"], median_ms=float(np.median(ts)) * 1e3, min_ms=float(np.min(ts)) * 1e3,
                evals=int(res["evals"][0]), iters=int(res["iters"][0]), status=int(res["status"][0]), cost=float(res["cost"][0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", default=None, help="one of %s" % STEPS)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.step:
        kind, arg = args.step.split("_", 1)
        res = transform_step(int(arg[1:]), args.reps) if kind == "transform" else \
            (lockstep_step(int(arg)) if kind == "step" else plan_step(args.reps))
        print(json.dumps(res))
        return 0
    out = {}
    for step in STEPS:
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)],
                                 capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            out[step] = dict(error=f"no result within {LIMIT_S} s")
            break                                       # nothing more is started on the device after a step that hung
        if res.returncode != 0:
            out[step] = dict(error=f"exit status {res.returncode}", stderr=res.stderr[-800:])
            break                                       # ... or failed
        out[step] = json.loads(res.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return 0 if all("error" not in v for v in out.values()) and len(out) == len(STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
