"""Exact corridor margins on the MI355X (anet_traj_row_margin_dev, csrc/corridor_margin_kernels.h): 4096 and 131 072 trajectories of
eight snap pieces against M = 16 rows, d = 0, in four corridor variants -- the synthetic corridors as generated, the same with every
row pushed out by 100 m, with every fourth row slot made active (it passes through the curve at mid-piece, so it survives pruning and
has its roots isolated), and with padding rows only (the floor: the loads, the derivative and its Bernstein form).  Next to it, for orientation, the sampled version of the
same question on the same inputs: anet_minco_partial_grads_dev with the corridor rows at res = 20.  And the `res` study: qp_solve on
synthetic corridors at res = 10 and 20, the exact margins of its three inequality groups beside the sampled ones.

Every step runs in a child process of its own under its own `timeout -k 10`; the driver stops at the first step that fails.  Times
are device events around one call after 5 warm-ups, medians of --reps (30).  Achieved bytes/s are the COMPULSORY bytes of a call,
8 (3 2s N + N + 4 M N) in and 20 N out per trajectory (5856 B at this shape), over that time, as a share of the 6.29 TB/s copy
bandwidth measured on this part.  Prints one JSON line.

    python tools/bench_corridor_margin.py [--reps 30] [--step NAME]
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

COPY_BW = 6.29e12            # B/s, measured copy bandwidth of the MI355X
STEPS = ["margin_4096", "margin_131072", "res_study"]
LIMIT_S = {"margin_131072": 420, "res_study": 420}
BASE = 8192                  # distinct trajectories generated on the host; larger batches repeat them on the device


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


def margin(step, reps):
    import torch
    import allocnet_amd as aa
    from allocnet_amd.synth import corridor_problem
    B, N, s, M, res = int(step.rsplit("_", 1)[1]), 8, 4, 16, 20
    Bb = min(B, BASE)
    head, tail, wps, T, hp = corridor_problem(np.random.default_rng(7), Bb, N, 3, M)
    co, _ = aa.minco_solve(head, tail, wps, T, s)
    ld = aa.recommended_ld(B)

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a.reshape(Bb, -1).T)).cuda().repeat(1, B // Bb)
        return torch.cat([t, torch.ones(t.shape[0], ld - B, dtype=torch.float64, device="cuda")], 1).contiguous()
    variants = {"as_generated": hp, "all_slack": hp.copy(), "quarter_active": hp.copy()}
    variants["all_slack"][..., 3] += 100.0 * np.any(hp != 0.0, axis=3)
    variants["all_padding"] = np.zeros_like(hp)      # every row is skipped: the loads, the derivative and the Bernstein form alone
    mid = aa.traj_eval(co, T, np.cumsum(T, axis=1) - 0.5 * T, 0)                      # (Bb, N, 3): the curve at mid-piece
    q4 = variants["quarter_active"]
    for r in range(0, M, 4):
        a = q4[:, :, r, :3]
        a[np.linalg.norm(a, axis=2) == 0.0] = [0.0, 0.0, 1.0]
        q4[:, :, r, 3] = np.einsum("bnk,bnk->bn", a, mid)
    d_co, d_T = up(co), up(T)
    ctx = aa.default_context(0)
    new = lambda rows, dt=torch.float64: torch.zeros(rows, ld, device="cuda", dtype=dt)
    d_m, d_t, d_r = new(N), new(N), new(N, torch.int32)
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbytes = 8 * (3 * 2 * s * N + N + 4 * M * N) + 20 * N
    out = dict(batch=B, pieces=N, order=s, rows=M, deriv=0, bytes_per_trajectory=nbytes, distinct_trajectories=Bb)
    for name, h in variants.items():
        d_h = up(h)
        fn = lambda: ctx.check(ctx.lib.anet_traj_row_margin_dev(ctx.handle, s, N, B, ld, q(d_co), q(d_T), 0, M, q(d_h), q(d_m), q(d_r),
                                                                q(d_t), st))
        med, mn = events_ms(fn, reps)
        m = d_m[:, :B]
        out[name] = dict(median_ms=med, min_ms=mn, ns_per_row_maximum=med * 1e6 / (B * N * M), achieved_TBps=nbytes * B / (med * 1e-3) / 1e12,
                         share_of_copy_bandwidth=nbytes * B / (med * 1e-3) / COPY_BW, share_of_pieces_outside=float((m > 0).double().mean()),
                         median_margin=float(m.median()))
        if name == "as_generated":       # the sampled version of the same question on the same inputs
            pen = aa.make_penalty(rho=0.0, w_corridor=100.0, w_vel=0.0, w_acc=0.0, smooth_mu=0.01, res=res, poly_rows=M)
            gC, gT, pc = new(N * 3 * 2 * s), new(N), new(N)
            ref = ctypes.cast(ctypes.pointer(pen), ctypes.c_void_p)
            pg = lambda: ctx.check(ctx.lib.anet_minco_partial_grads_dev(ctx.handle, s, N, B, ld, q(d_co), q(d_T), q(d_h), ref, 0, q(gC),
                                                                        q(gT), q(pc), st))
            med2, mn2 = events_ms(pg, reps)
            out["partial_grads_res20_same_corridors"] = dict(median_ms=med2, min_ms=mn2, margin_over_partial_grads=med / med2)
    return out


def _sampled(co, T, rows, d, res):
    """max over the samples j T / res, j = 0 .. res - 1 (QPSolver::solve's), and over the rows, of a . p^(d) - b: (B, N)"""
    B, N, _, D = co.shape
    pw = np.arange(D - 1, -1, -1)
    ff = np.ones(D)
    for e in range(d):
        ff *= np.maximum(pw - e, 0)
    tau = (np.arange(res) / res)[None, None, :] * T[:, :, None]                          # (B, N, res)
    tp = tau[..., None] ** np.maximum(pw - d, 0)                                        # (B, N, res, D)
    val = np.einsum("bnad,bnrd->bnra", co * ff, tp)                                     # (B, N, res, 3)
    g = np.einsum("bnmk,bnrk->bnrm", rows[..., :3], val) - rows[:, :, None, :, 3]
    g = np.where(np.any(rows != 0.0, axis=3)[:, :, None, :], g, -np.inf)
    return g.max(axis=(2, 3))


def res_study(step, reps):
    import allocnet_amd as aa
    from allocnet_amd.synth import corridor_problem
    B, N, s, M, max_vel, max_acc = 1024, 8, 3, 16, 4.0, 6.0
    head, tail, wps, T, hp = corridor_problem(np.random.default_rng(5), B, N, 3, M)
    out = dict(batch=B, pieces=N, order=s, rows=M, max_vel=max_vel, max_acc=max_acc)
    pct = lambda x: dict(zip(("p50", "p90", "p99", "max"), (float(v) for v in np.percentile(x, [50, 90, 99, 100]))))
    for res in (10, 20):
        sol = aa.qp_solve(s, head, tail, hp, T, res=res, max_vel=max_vel, max_acc=max_acc)
        co = sol["coeffs"]
        exact = aa.traj_qp_margins(co, T, hp, max_vel, max_acc)
        boxes = [np.broadcast_to(aa.trajectory.box_rows(v), (B, N, 6, 4)) for v in (max_vel, max_acc)]
        sampled = [_sampled(co, T, hp, 0, res), _sampled(co, T, boxes[0], 1, res), _sampled(co, T, boxes[1], 2, res)]
        entry = dict(status_counts={str(k): int(v) for k, v in zip(*np.unique(np.asarray(sol["status"]), return_counts=True))})
        for name, e, sm in zip(("corridor", "vel_box", "acc_box"), exact, sampled):
            e, sm = e.max(axis=1), sm.max(axis=1)                                        # per trajectory
            entry[name] = dict(exact=pct(e), sampled=pct(sm), exact_minus_sampled=pct(e - sm),
                               share_exact_above_1e_3=float((e > 1e-3).mean()), share_sampled_above_1e_3=float((sm > 1e-3).mean()))
        m, _, t = aa.traj_row_margin(co, T, hp, 0)
        outside = m > 1e-3
        entry["pieces_outside_by_more_than_1e_3"] = float(outside.mean())
        entry["of_those_deepest_point_in_the_last_1_over_res_of_the_piece"] = float((t[outside] > T[outside] * (1.0 - 1.0 / res)).mean())
        entry["of_those_deepest_point_at_the_end_of_the_piece"] = float((t[outside] == T[outside]).mean())
        out["res_%d" % res] = entry
    return out


def run_step(step, reps):
    return res_study(step, reps) if step == "res_study" else margin(step, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", default=None, help="one of %s" % STEPS)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.step:
        print(json.dumps(run_step(args.step, args.reps)))
        return 0
    out = {}
    for step in STEPS:
        limit = LIMIT_S.get(step, 300)
        res = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--reps",
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
