#!/usr/bin/env python3
"""SHA-256 of every output array of the penalty's four kernel forms, one line per array: two builds compute the same bits
exactly when their lines are equal (run both through tools/ab_head.sh and compare the OLD and NEW blocks).
    python tools/hash_cost_grad.py                       # the whole default list
    python tools/hash_cost_grad.py cg 4,3,8,4096 ...     # cost + gradient of these shapes only: order,boundary count,pieces,batch
    python tools/hash_cost_grad.py lbfgs 3,3,9,256 ...   # one-launch L-BFGS runs of these shapes only
The default list follows the launch ladders (launch_piece_grad, the one-launch ladder launch_cost_grad_fused and its decision
cost_grad_in_one_launch, the persistent ladder of anet_lbfgs_minco): orders 2..4; the exact and the generic piece counts; batches
that take the sample-split, the two-lane, the lane and both matrix-instruction shapes; res 20 and 7; 0 (hpolys NULL), 5, 13, 16
and 24 corridor rows; penalty on and off; piece counts on both sides of the persistent kernel's NB = 8 / 16 step.  The process-
level switches (ANET_PG_MX, ANET_FUSED_MX, ANET_FUSED_MAX_GROUPS) are read once per process: run one process per setting."""
import hashlib, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the tree this copy of the tool lies in
import torch
import allocnet_amd as aa
from allocnet_amd.synth import corridor_problem
from tools.bench_configs import to_bm

CG_SHAPES = [(s, min(s, 3), 8, B) for s in (2, 3, 4) for B in (64, 512, 4096, 20000)] + [
    (3, 3, 8, 65536), (4, 3, 8, 65536),                                # eight column sets per wave
    (3, 3, 16, 4096), (3, 3, 16, 20000), (3, 3, 12, 1024), (3, 3, 5, 1024), (3, 3, 1, 1024),
    (4, 3, 5, 1024), (4, 4, 8, 1024), (4, 3, 1, 1024), (2, 2, 16, 1024)]
LBFGS_SHAPES = [(s, 3, N, 192) for s in (3, 4) for N in (5, 8, 9, 16)]
# (res, corridor rows, penalty): every shape runs all of these, the largest batches the first two only
VARIANTS = [(20, 16, True), (20, 24, True), (7, 16, True), (20, 0, True), (20, 5, True), (20, 13, True), (7, 13, True), (20, 16, False)]

dev = torch.device("cuda", 0)
ctx = aa.Context(0)


def digest(t, B):
    return hashlib.sha256(np.ascontiguousarray(t[..., :B].cpu().numpy()).tobytes()).hexdigest()[:32]


def problem(s, c, N, B):
    """Host arrays of one problem; 24 corridor rows per piece (two draws of the generator's 16: the second's box rows are wider)."""
    head, tail, wps, T, hp = corridor_problem(np.random.default_rng(1000 * s + N), B, N, c, 16)
    hp2 = corridor_problem(np.random.default_rng(7), B, N, c, 16)[4]
    return head, tail, wps, T, np.concatenate([hp, hp2[:, :, :8]], axis=2)


def penalty(res, M):
    return aa.make_penalty(rho=50.0, w_corridor=1e4, w_vel=1e3, w_acc=1e3, smooth_mu=1e-2, max_vel=2.0, max_acc=3.0, res=res, poly_rows=M)


def variants(B):
    return VARIANTS[:2] if B > 30000 else VARIANTS


def run_cg(s, c, N, B):
    ld = aa.recommended_ld(B)
    head, tail, wps, T, hp = problem(s, c, N, B)
    th, tt, tw, tT = (to_bm(torch, x, B, ld, dev) for x in (head, tail, wps, T))
    nco = N * 3 * 2 * s
    for res, M, on in variants(B):
        thp = to_bm(torch, hp[:, :, :M], B, ld, dev) if on and M else None
        nwork = ctx.lib.anet_minco_cost_grad_workspace(s, N, ld)
        work = torch.zeros(nwork, device=dev, dtype=torch.float64)
        coeffs, cost, gP, gT = (torch.zeros(rows, ld, device=dev, dtype=torch.float64) for rows in (nco, 1, max(3 * (N - 1), 1), N))
        aa.minco_cost_grad_dev(th, tt, tw, tT, s, c, N, B, hpolys=thp, penalty=penalty(res, M) if on else None, work=work, cost=cost,
                               gradP=gP, gradT=gT, coeffs=coeffs, ctx=ctx)
        torch.cuda.synchronize()
        # the per-piece penalty costs of the three-launch forms: rows of the workspace (zeros where one launch did the work)
        pcost = work[(2 * nco + N) * ld:(2 * nco + 2 * N) * ld].view(N, ld)
        tag = f"cg s={s} c={c} N={N} B={B} res={res} M={M} pen={int(on)}"
        for name, t in (("cost", cost), ("gradP", gP), ("gradT", gT), ("coeffs", coeffs), ("pcost", pcost)):
            print(tag, name, digest(t, B), flush=True)


def run_lbfgs(s, c, N, B):
    ld = aa.recommended_ld(B)
    data = problem(s, c, N, B)
    for res, M, on in VARIANTS:
        th, tt, tw, tT = (to_bm(torch, x, B, ld, dev) for x in data[:4])
        thp = to_bm(torch, data[4][:, :, :M], B, ld, dev) if on and M else None
        r = aa.lbfgs_minco_dev(th, tt, tw, tT, s, c, N, B, hpolys=thp, penalty=penalty(res, M) if on else None,
                               param=aa.lbfgs_parameter_t(), max_evals=120, opt=3, ctx=ctx)
        torch.cuda.synchronize()
        tag = f"lbfgs s={s} c={c} N={N} B={B} res={res} M={M} pen={int(on)}"
        for name, t in (("wps", tw), ("T", tT), ("f", r["cost"]), ("status", r["status"]), ("iters", r["iters"]), ("evals", r["evals"])):
            print(tag, name, digest(t, B), flush=True)


def main(argv):
    what = argv[0] if argv else "all"
    shapes = [tuple(int(v) for v in a.split(",")) for a in argv[1:]]
    if what in ("cg", "all"):
        for sh in shapes or CG_SHAPES:
            run_cg(*sh)
    if what in ("lbfgs", "all"):
        for sh in shapes or LBFGS_SHAPES:
            run_lbfgs(*sh)


main(sys.argv[1:])
