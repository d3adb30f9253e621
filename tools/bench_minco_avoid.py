"""The trajectory-avoidance penalty on the MI355X (anet_minco_avoid_partial_grads_dev, csrc/avoid_kernels.h) beside the route a user
had before it: anet_traj_eval_dev of every neighbour at the ego's sample times (position and velocity), then torch operations for
the penalty and autograd for its gradient w.r.t. the ego's sampled positions.  The torch route stops there: it is NOT charged for
the contraction of those sample gradients to coefficient and duration gradients, nor for the suffix sums, which the kernel includes.
The fleet is that of tools/bench_traj_separation.py: 512 trajectories of eight snap pieces through random walks of 2 m segments in a
40 m x 40 m x 4 m volume, started at random offsets within 5 s; res = 20 samples per piece.  Steps:
  all_512     every other vehicle is a neighbour (511 per ego)
  near_512    the neighbours whose exact separation (anet_traj_separation) is below 2 m
Each step runs in a child process under its own `timeout -k 10`.  Times are device events around one call after 5 warm-ups, medians
of --reps (30).  Prints one JSON line.

    python tools/bench_minco_avoid.py [--reps 30] [--step NAME]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ["all_512", "near_512"]
RES = 20
NEAR = 2.0


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


def run(step, reps):
    import torch
    import allocnet_amd as aa
    kind, B = step.rsplit("_", 1)
    B = int(B)
    N, s = 8, 4
    rng = np.random.default_rng(11)
    pts = np.empty((B, N + 1, 3))
    pts[:, 0] = rng.uniform([-20.0, -20.0, 1.0], [20.0, 20.0, 5.0], (B, 3))
    for i in range(N):
        step_ = rng.normal(size=(B, 3)) * np.array([1.0, 1.0, 0.2])
        pts[:, i + 1] = pts[:, i] + 2.0 * step_ / np.linalg.norm(step_, axis=1, keepdims=True)
    head, tail = np.zeros((B, 3, 3)), np.zeros((B, 3, 3))
    head[:, :, 0], tail[:, :, 0] = pts[:, 0], pts[:, -1]
    T = np.linalg.norm(np.diff(pts, axis=1), axis=2) / 1.5 + 0.4
    t0 = rng.uniform(0.0, 5.0, B)
    co, _ = aa.minco_solve(head, tail, pts[:, 1:-1], T, s)
    if kind == "all":
        start, nbr = aa.neighbours_all(B, B, exclude_self=True)
    else:
        sep, _, _, pairs = aa.traj_separation(co, T, t0=t0)
        start, nbr = aa.neighbours_from_pairs(pairs, B, keep=sep < NEAR)
    pen = aa.make_avoid_penalty(w=100.0, smooth_mu=0.05, min_dist=1.0, z_scale=1.0, res=RES)
    ld = aa.recommended_ld(B)
    D = 2 * s

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a.reshape(B, -1).T)).cuda()
        return torch.cat([t, torch.ones(t.shape[0], ld - B, dtype=torch.float64, device="cuda")], 1).contiguous()
    d_co, d_T = up(co), up(T)
    d_t0 = torch.from_numpy(t0).cuda()
    others = aa.AvoidOthers(d_co, d_T, d_t0, N, B)                                  # the fleet against itself
    d_nbr = (torch.from_numpy(start).cuda(), torch.from_numpy(nbr).cuda())
    new = lambda *shape: torch.zeros(*shape, device="cuda", dtype=torch.float64)
    gC, gT, pc, g0 = new(N * 3 * D, ld), new(N, ld), new(N, ld), new(ld)
    ctx = aa.default_context(0)
    kernel = lambda: aa.minco_avoid_partial_grads_dev(pen, s, N, B, d_co, d_T, others, d_nbr, gC, gT, pc, g0, t0=d_t0, ctx=ctx)
    med, mn = events_ms(kernel, reps)
    kernel()
    torch.cuda.synchronize()
    cost = float(pc[:, :B].sum())

    # the torch route.  Other o is evaluated at the sample times of every ego that lists it (the lists are symmetric: its own list),
    # padded to the longest list: tq [(k, i, j)][o] = t_(nbr_o[k]),i,j - t0_o.
    counts = np.diff(start)
    kmax = int(counts.max())
    S = N * RES
    sigma = torch.arange(RES, device="cuda", dtype=torch.float64) / RES
    Te = d_T[:, :B].T                                                                  # (B, N)
    K = d_t0[:, None] + torch.cumsum(Te, 1) - Te
    tau = (sigma[None, None, :] * Te[:, :, None])                                      # (B, N, RES)
    t_s = (K[:, :, None] + tau).reshape(B, S)
    end = d_t0 + Te.sum(1)
    slot = torch.zeros(B, kmax, dtype=torch.long, device="cuda")                      # the k-th neighbour of o (0 where none)
    used = torch.zeros(B, kmax, dtype=torch.bool, device="cuda")
    rows = np.repeat(np.arange(B), counts)
    kk = np.arange(len(nbr)) - np.repeat(start[:-1], counts)
    slot[torch.from_numpy(rows).cuda(), torch.from_numpy(kk).cuda()] = torch.from_numpy(nbr.astype(np.int64)).cuda()
    used[torch.from_numpy(rows).cuda(), torch.from_numpy(kk).cuda()] = True
    nq = kmax * S
    t_at = t_s[slot]                                                                   # (B as o, kmax, S): global sample times
    there = used[:, :, None] & (t_at >= d_t0[:, None, None]) & (t_at < end[:, None, None])
    tq = new(nq, ld)
    tq[:, :B] = (t_at - d_t0[:, None, None]).clamp(min=0.0).reshape(B, nq).T
    pos, vel = new(nq * 3, ld), new(nq * 3, ld)
    q_ = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    # the ego's own sampled positions, by Horner in torch (a leaf for autograd)
    cb = d_co[:, :B].T.reshape(B, N, 3, D)
    p_b = cb[..., 0][:, :, None, :].expand(B, N, RES, 3)
    for col in range(1, D):
        p_b = p_b * tau[..., None] + cb[..., col][:, :, None, :]
    p_b = p_b.reshape(B, S, 3).contiguous()
    out = {}

    def ev():
        for d, buf in ((0, pos), (1, vel)):
            ctx.check(ctx.lib.anet_traj_eval_dev(ctx.handle, s, N, B, ld, q_(d_co), q_(d_T), nq, q_(tq), d, q_(buf), st))

    def penalty():
        pe = p_b.clone().requires_grad_(True)
        po = pos.view(kmax, S, 3, ld)[..., :B].permute(3, 0, 1, 2)                     # (o, k, S, 3)
        r = pe[slot] - po
        x = pen.min_dist ** 2 - (r * r).sum(-1)
        xd = (x / pen.smooth_mu).clamp(0.0, 1.0)
        f = torch.where(x > pen.smooth_mu, x - 0.5 * pen.smooth_mu, (pen.smooth_mu - 0.5 * xd * pen.smooth_mu) * xd ** 3)
        J = (pen.w * torch.where(there, f, torch.zeros_like(f)) * (Te[slot][:, :, :, None].expand(B, kmax, N, RES).reshape(B, kmax, S) / RES)).sum()
        J.backward()
        out["J"], out["F"] = J.detach(), pe.grad

    def route():
        ev(); penalty()
    parts = {name: events_ms(fn, reps)[0] for name, fn in (("traj_eval_ms", ev), ("penalty_autograd_ms", penalty))}
    med2, mn2 = events_ms(route, reps)
    route()
    torch.cuda.synchronize()
    terms = int(len(nbr)) * S
    return dict(trajectories=B, pieces=N, order=s, res=RES, neighbours=int(len(nbr)), neighbours_per_ego_max=kmax, terms=terms,
                kernel=dict(median_ms=med, min_ms=mn, terms_per_s=terms / (med * 1e-3)),
                torch_route=dict(median_ms=med2, min_ms=mn2, **parts, queries_per_trajectory=nq),
                kernel_over_torch_route=med / med2, cost=cost, torch_cost=float(out["J"]),
                cost_relative_difference=abs(float(out["J"]) - cost) / max(abs(cost), 1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", default=None, help="one of %s" % STEPS)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.step:
        print(json.dumps(run(args.step, args.reps)))
        return 0
    out = {}
    for step in STEPS:
        res = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--step", step, "--reps",
                              str(args.reps)], capture_output=True, text=True)
        if res.returncode != 0:                         # nothing more is started on the device after a step that hung or failed
            out[step] = dict(error=f"exit status {res.returncode}" + (" (time limit)" if res.returncode in (124, 137) else ""),
                             stderr=res.stderr[-800:])
            break
        out[step] = json.loads(res.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return 0 if all("error" not in v for v in out.values()) and len(out) == len(STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
