"""Differential-flatness kernels on the MI355X: the pointwise map and adjoint at 2^24 elements, the sampled extrema at
131 072 x 8-piece snap, and the thrust / tilt / body-rate penalty gradients at 4096 and 131 072 x 8-piece snap next to the
existing penalty kernel with the box rows only (anet_minco_partial_grads_dev, hpolys = NULL) at the same shapes.

Every step runs in a child process of its own under its own time limit; the driver stops at the first step that fails.  Times are
device events around one call after warm-up, medians of --reps (>= 20).  Achieved bytes/s are the COUNTED bytes of each call
(below) over that time, as a share of the 6.29 TB/s copy bandwidth measured on this part.  Prints one JSON line.

    python tools/bench_flatness.py [--reps 30] [--step NAME]

For kernel times, one run of its own:  rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_flatness.py --step all_once
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
# counted doubles per element: forward reads vel, acc, jer (9) [+ psi, dpsi] and writes thr, quat, omg (8); backward reads the same
# inputs, pos_grad, vel_grad (6), thr_grad, quat_grad, omg_grad (8) and writes pos, vel, acc, jer totals (12) and two scalars
FWD_BYTES = {True: 8 * (11 + 8), False: 8 * (9 + 8)}
BWD_BYTES = {True: 8 * (11 + 14 + 14), False: 8 * (9 + 14 + 14)}
# floating-point operations per sample of k_flat_piece_grad, counted by hand from csrc/flatness_kernels.h (an estimate: FMA = 2,
# divide / square root = 1): four basis rows against c~ (2 * 4 * 3 * D), the snap row (2 D), the map (~120), four penalty rows
# (~60); on a sample with an active row also the adjoint (~250) and the gradient update (2 * 3 * 3 * D)
def piece_grad_flops(s, active):
    D = 2 * s
    return 2 * 4 * 3 * D + 2 * D + 120 + 60 + (250 + 2 * 3 * 3 * D if active else 0)


STEPS = ["forward_yaw", "forward", "backward_yaw", "backward", "extrema", "piece_grad_4096", "piece_grad_131072"]
LIMIT_S = {"extrema": 600, "piece_grad_131072": 600}


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


def pointwise(step, reps):
    import torch
    import allocnet_amd as aa
    yaw, back = step.endswith("_yaw"), step.startswith("backward")
    n = 1 << 24
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda rows, scale: (torch.rand(rows, n, generator=g, device="cuda", dtype=torch.float64) * 2.0 - 1.0) * scale
    vel, acc, jer = rnd(3, 4.0), rnd(3, 6.0), rnd(3, 5.0)
    psi, dpsi = (rnd(1, 3.0)[0], rnd(1, 1.0)[0]) if yaw else (None, None)
    par = aa.make_flat_params()
    if back:
        ups = (rnd(3, 1.0), rnd(3, 1.0), rnd(1, 1.0)[0], rnd(4, 1.0), rnd(3, 1.0))
        fn = lambda: aa.flat_backward_dev(par, vel, acc, jer, psi, dpsi, *ups)
        nbytes = BWD_BYTES[yaw]
    else:
        thr, quat, omg = aa.flat_forward_dev(par, vel, acc, jer, psi, dpsi)
        fn = lambda: aa.flat_forward_dev(par, vel, acc, jer, psi, dpsi, thr=thr, quat=quat, omg=omg)
        nbytes = FWD_BYTES[yaw]
    med, mn = events_ms(fn, reps)
    bw = nbytes * n / (med * 1e-3)
    return dict(elements=n, bytes_per_element=nbytes, median_ms=med, min_ms=mn, achieved_TBps=bw / 1e12,
                share_of_copy_bandwidth=bw / COPY_BW,
                note="backward timings include the allocation of its six outputs by the caching allocator" if back else "")


def snap_batch(B, N=8, s=4):
    """Rest-to-rest random-walk problems solved on the device, durations tripled (inside the planner's boxes for nearly all)."""
    import torch
    import allocnet_amd as aa
    from allocnet_amd.synth import random_problem
    head, tail, wps, T = random_problem(np.random.default_rng(7), B, N, 3, rest=True)
    T *= 3.0
    co, _ = aa.minco_solve(head, tail, wps, T, s)
    ld = aa.recommended_ld(B)
    up = lambda a, fill=0.0: torch.cat([torch.from_numpy(a.reshape(B, -1).T.copy()),
                                        torch.full((a.reshape(B, -1).shape[1], ld - B), fill, dtype=torch.float64)], 1).cuda()
    return up(co), up(T, 1.0), ld


def extrema(step, reps):
    import torch
    import allocnet_amd as aa
    B, N, s, res = 131072, 8, 4, 20
    co, T, ld = snap_batch(B, N, s)
    ctx = aa.default_context(0)
    par = aa.make_flat_params()
    out = torch.empty(4, ld, device="cuda", dtype=torch.float64)
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ref = ctypes.cast(ctypes.pointer(par), ctypes.c_void_p)
    fn = lambda: ctx.check(ctx.lib.anet_traj_flat_extrema_dev(ctx.handle, ref, s, N, B, ld, q(co), q(T), res, q(out), st))
    med, mn = events_ms(fn, reps)
    samples = B * N * (res + 1)
    return dict(batch=B, pieces=N, order=s, res=res, median_ms=med, min_ms=mn, samples=samples, ns_per_sample=med * 1e6 / samples,
                bytes_per_trajectory=8 * (N * 3 * 2 * s + N + 4))


def piece_grad(step, reps):
    import torch
    import allocnet_amd as aa
    B, N, s, res = int(step.rsplit("_", 1)[1]), 8, 4, 20
    co, T, ld = snap_batch(B, N, s)
    ctx = aa.default_context(0)
    par = aa.make_flat_params()
    new = lambda rows: torch.zeros(rows, ld, device="cuda", dtype=torch.float64)
    gC, gT, pc = new(N * 3 * 2 * s), new(N), new(N)
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    ref = lambda o: ctypes.cast(ctypes.pointer(o), ctypes.c_void_p)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = dict(batch=B, pieces=N, order=s, res=res)
    # limits that a share of the samples violates (the adjoint is skipped by waves none of whose lanes violates one)
    fpen = aa.make_flat_penalty(w_thrust=30.0, w_tilt=200.0, w_bdr=10.0, smooth_mu=0.01, min_thrust=9.6, max_thrust=10.2,
                                max_tilt=0.12, max_bdr=0.6, res=res)
    far = aa.make_flat_penalty(w_thrust=30.0, w_tilt=200.0, w_bdr=10.0, smooth_mu=0.01, min_thrust=-1e6, max_thrust=1e6,
                               max_tilt=3.0, max_bdr=1e6, res=res)
    flat = lambda p, acc: (lambda: ctx.check(ctx.lib.anet_minco_flat_partial_grads_dev(
        ctx.handle, ref(par), ref(p), s, N, B, ld, q(co), q(T), acc, q(gC), q(gT), q(pc), st)))
    pairs, samples = B * N, B * N * res
    for name, p, acc in (("flat_active", fpen, 0), ("flat_active_accumulate", fpen, 1), ("flat_no_row_active", far, 0)):
        med, mn = events_ms(flat(p, acc), reps)
        active = name != "flat_no_row_active"
        fl = piece_grad_flops(s, active)
        nbytes = 8 * (3 * 2 * s + 1 + (2 if acc else 1) * (3 * 2 * s + 2))
        out[name] = dict(median_ms=med, min_ms=mn, ns_per_sample=med * 1e6 / samples, counted_flops_per_sample=fl,
                         TFLOPs_if_every_sample_counted_so=fl * samples / (med * 1e-3) / 1e12, bytes_per_pair=nbytes,
                         achieved_TBps=nbytes * pairs / (med * 1e-3) / 1e12)
    flat(fpen, 0)()
    torch.cuda.synchronize()
    out["share_of_pieces_with_a_violated_limit"] = float((pc[:, :B] > 0).double().mean())
    pen = aa.make_penalty(rho=0.0, w_vel=25.0, w_acc=9.0, smooth_mu=0.05, max_vel=1.5, max_acc=2.5, res=res)
    box = lambda: ctx.check(ctx.lib.anet_minco_partial_grads_dev(ctx.handle, s, N, B, ld, q(co), q(T), None, ref(pen), 1, q(gC), q(gT),
                                                                q(pc), st))
    med, mn = events_ms(box, reps)
    out["box_rows_only_with_energy"] = dict(median_ms=med, min_ms=mn, ns_per_sample=med * 1e6 / samples,
                                            launch_shape=aa.minco_piece_grad_shape(s, N, B, pen))
    out["flat_over_box_rows"] = out["flat_active"]["median_ms"] / med
    return out


def run_step(step, reps):
    if step in ("forward", "forward_yaw", "backward", "backward_yaw"):
        return pointwise(step, reps)
    if step == "extrema":
        return extrema(step, reps)
    return piece_grad(step, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", default=None, help="one of %s, or all_once (every step in this process, for a profiler)" % STEPS)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.step == "all_once":
        print(json.dumps({s: run_step(s, 20) for s in STEPS}))
        return 0
    if args.step:
        print(json.dumps(run_step(args.step, args.reps)))
        return 0
    out = {}
    for step in STEPS:
        limit = LIMIT_S.get(step, 300)
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)],
                                 capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            out[step] = dict(error=f"no result within {limit} s")
            break                                       # nothing more is started on the device after a step that hung
        if res.returncode != 0:
            out[step] = dict(error=f"exit status {res.returncode}", stderr=res.stderr[-800:])
            break                                       # ... or failed
        out[step] = json.loads(res.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return 0 if all("error" not in v for v in out.values()) and len(out) == len(STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
