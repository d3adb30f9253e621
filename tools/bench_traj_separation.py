"""Exact minimum separation between pairs of trajectories on the MI355X (anet_traj_separation_dev, csrc/separation_kernels.h)
beside the route that existed before it: anet_traj_eval_dev of every trajectory on one global time grid, then torch norms of the
position differences of every pair and their minimum over the times both trajectories exist.  The grid's step is a twentieth of
the mean piece duration: 20 samples per piece.  The fleet is 512 trajectories of eight snap pieces from minco_solve through random
walks of 2 m segments in a 40 m x 40 m x 4 m volume, started at random offsets within 5 s; the pairs are all 130 816 with a < b,
sorted by a.  Steps:
  fleet_512      the exact route with the cutoff off and with the cutoff at 1 m, the sampled route, and by how much the sampled
                 separation exceeds the exact one (median, 99 %, worst)
The step runs in a child process under its own `timeout -k 10`.  Times are device events around one call after 5 warm-ups, medians
of --reps (30).  Prints one JSON line.

    python tools/bench_traj_separation.py [--reps 30] [--step NAME]
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

STEPS = ["fleet_512"]
RES = 20


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
    B = int(step.rsplit("_", 1)[1])
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
    pairs = aa.trajectory.all_pairs(B)
    P = len(pairs)
    ld = aa.recommended_ld(B)

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a.reshape(B, -1).T)).cuda()
        return torch.cat([t, torch.ones(t.shape[0], ld - B, dtype=torch.float64, device="cuda")], 1).contiguous()
    d_co, d_T = up(co), up(T)
    d_t0 = torch.from_numpy(t0).cuda()
    d_pa, d_pb = (torch.from_numpy(np.ascontiguousarray(pairs[:, k])).cuda() for k in (0, 1))
    ctx = aa.default_context(0)
    outs = dict(sep=torch.zeros(P, device="cuda", dtype=torch.float64), t=torch.zeros(P, device="cuda", dtype=torch.float64),
                piece_a=torch.zeros(P, device="cuda", dtype=torch.int32), piece_b=torch.zeros(P, device="cuda", dtype=torch.int32))
    exact = lambda cutoff: aa.traj_separation_dev(d_co, d_T, d_pa, d_pb, s, N, B, t0=d_t0, cutoff=cutoff, ctx=ctx, **outs)
    med_off, mn_off = events_ms(lambda: exact(float("inf")), reps)
    med_cut, mn_cut = events_ms(lambda: exact(1.0), reps)
    exact(1.0)
    torch.cuda.synchronize()
    sep_cut = outs["sep"].clone()
    exact(float("inf"))
    torch.cuda.synchronize()
    sep = outs["sep"].clone()
    # the sampled route: one global grid, every trajectory at (grid - t0) where it exists
    step_t = float(T.mean()) / RES
    end = t0 + T.sum(axis=1)
    grid = torch.arange(0.0, float(end.max()) + step_t, step_t, device="cuda", dtype=torch.float64)
    G = int(grid.numel())
    d_end = torch.from_numpy(end).cuda()
    local = grid[:, None] - d_t0[None, :]                                         # (G, B)
    live = (local >= 0.0) & (grid[:, None] <= d_end[None, :])
    tq = torch.zeros(G, ld, device="cuda", dtype=torch.float64)
    tq[:, :B] = local.clamp(min=0.0)
    pos = torch.zeros(G * 3, ld, device="cuda", dtype=torch.float64)
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_s = torch.zeros(P, device="cuda", dtype=torch.float64)
    chunk = max(1, (1 << 25) // G)                                                 # at most 0.75 GiB of differences at a time

    def ev():
        ctx.check(ctx.lib.anet_traj_eval_dev(ctx.handle, s, N, B, ld, q(d_co), q(d_T), G, q(tq), 0, q(pos), st))

    def dist():
        p3 = pos.view(G, 3, ld)[:, :, :B].permute(2, 0, 1)                        # (B, G, 3)
        for a in range(0, P, chunk):
            ia, ib = d_pa[a:a + chunk].long(), d_pb[a:a + chunk].long()
            d = torch.linalg.vector_norm(p3[ia] - p3[ib], dim=2)
            d = torch.where(live.T[ia] & live.T[ib], d, torch.full_like(d, float("inf")))
            d_s[a:a + chunk] = d.min(dim=1).values

    def sampled():
        ev(); dist()
    parts = {name: events_ms(fn, reps)[0] for name, fn in (("traj_eval_ms", ev), ("distance_ms", dist))}
    med2, mn2 = events_ms(sampled, reps)
    sampled()
    torch.cuda.synchronize()
    both = torch.isfinite(d_s) & torch.isfinite(sep)
    over = (d_s - sep)[both].cpu().numpy()
    close = (sep < 1.0)
    return dict(trajectories=B, pieces=N, order=s, pairs=P, res=RES, grid_points=G,
                exact=dict(median_ms=med_off, min_ms=mn_off, pairs_per_s=P / (med_off * 1e-3)),
                exact_cutoff_1m=dict(median_ms=med_cut, min_ms=mn_cut, pairs_per_s=P / (med_cut * 1e-3),
                                     same_bits_below_cutoff=bool(torch.equal(sep[close], sep_cut[close])),
                                     never_below_exact=bool((sep_cut >= sep).all())),
                sampled=dict(median_ms=med2, min_ms=mn2, pairs_per_s=P / (med2 * 1e-3), **parts),
                exact_over_sampled=med_off / med2, cutoff_over_sampled=med_cut / med2,
                pairs_with_common_time=int(torch.isfinite(sep).sum()), pairs_below_1m=int(close.sum()),
                separation_m=dict(min=float(sep.min()), median=float(sep[torch.isfinite(sep)].median())),
                sampled_minus_exact_m=dict(min=float(over.min()), median=float(np.median(over)), p99=float(np.quantile(over, 0.99)),
                                           worst=float(over.max())))


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
