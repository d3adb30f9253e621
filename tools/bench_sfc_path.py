"""The shortest route through a corridor on the MI355X (allocnet_amd/sfc_opt.py, csrc/sfc_path_kernels.h), two measurements:

  (a) eval_K16 / eval_K32: k_sfc_path_eval alone (anet_sfc_path_cost_grad_dev) at 131 072 problems of 8 polytopes, device events,
      medians of --reps after 5 warm-up calls, and the rate against the compulsory bytes per problem, 8 ((N-1) 5 K + 7): every xi
      and vertex row once, every gradient row once, start, goal, cost.  The kernel requests 8 ((N-1) 9 K + 7): it reads a
      waypoint's rows a second time for the gradient;
  (b) solve_4096: a whole route solve (anet_sfc_shortest_path_dev from the vertex mean, defaults, 400 evaluations at most) of
      4096 random corridors of 8 polytopes, K = 32, device events around the call, median of --reps after 2 warm-up calls, with
      the evaluations the problems took.

Every step runs in a child process of its own under its own time limit; the driver stops at the first step that fails.  Prints one
JSON line.

    python tools/bench_sfc_path.py [--reps 30] [--step NAME]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ["eval_K16", "eval_K32", "solve_4096"]
LIMIT_S = 300


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


def eval_step(K, reps):
    import torch
    import allocnet_amd as aa
    B, N = 131072, 8
    ld = aa.recommended_ld(B)
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda rows: torch.randn(rows, ld, device="cuda", dtype=torch.float64, generator=g)
    xi, verts, start, goal = rnd((N - 1) * K) * 0.3, rnd((N - 1) * K * 3) * 5.0, rnd(3), rnd(3)
    ctx = aa.default_context(0)
    cost, grad = aa.sfc_path_cost_grad_dev(start, goal, xi, verts, N, B, K, ctx=ctx)
    med, best = events_ms(lambda: aa.sfc_path_cost_grad_dev(start, goal, xi, verts, N, B, K, cost=cost, grad_xi=grad, ctx=ctx), reps)
    compulsory, requested = B * 8 * ((N - 1) * 5 * K + 7), B * 8 * ((N - 1) * 9 * K + 7)
    return dict(problems=B, polytopes=N, max_verts=K, median_ms=med, min_ms=best, compulsory_bytes=compulsory, requested_bytes=requested,
                compulsory_GBps=compulsory / (med * 1e-3) / 1e9, requested_GBps=requested / (med * 1e-3) / 1e9)


def solve_step(B, reps):
    import torch
    import allocnet_amd as aa
    from allocnet_amd.sfc_opt import _bm
    from allocnet_amd.synth import corridor_problem
    N, M, K = 8, 16, 32
    head, tail, _, _, hp = corridor_problem(np.random.default_rng(2), B, N, 3, M)
    ctx = aa.default_context(0)
    ov = aa.sfc_overlap_vertices_dev(_bm(hp, B), N, B, M, K, ctx=ctx)
    start, goal = _bm(head[:, :, 0], B), _bm(tail[:, :, 0], B)
    out = {}

    def run():
        out.update(aa.sfc_shortest_path_dev(start, goal, ov["verts"], ov["count"], N, B, K, overlap_status=ov["status"],
                                            work=out.get("work"), ctx=ctx))
    med, best = events_ms(run, max(5, reps // 3), warm=2)
    ev, st = out["evals"].cpu().numpy(), out["status"].cpu().numpy()
    return dict(problems=B, polytopes=N, max_verts=K, variables=(N - 1) * K, median_ms=med, min_ms=best,
                evals_median=float(np.median(ev)), evals_max=int(ev.max()), ms_per_step=med / max(1, int(ev.max())),
                converged_or_stopped=float(np.isin(st, (0, 1)).mean()), still_running=float((st == aa.lbfgs.LBFGS_RUNNING).mean()),
                length_mean=float(out["length"].mean().item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", default=None, help="one of %s" % STEPS)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.step:
        kind, arg = args.step.split("_", 1)
        res = eval_step(int(arg[1:]), args.reps) if kind == "eval" else solve_step(int(arg), args.reps)
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
