"""The whole-body corridor penalty on the MI355X: anet_minco_body_partial_grads_dev at 4096 and 131 072 x 8-piece snap, res 20,
K = 8 body vertices (a plate), M = 16 rows per polytope, next to
  * what a user has to write without it: the states from a torch basis evaluation of the coefficients (traj_eval has no backward),
    the attitude from torch_layer.flat_layer, the rotation and the smoothed L1 in torch, the gradients from autograd -- in chunks
    of 8192 trajectories (the (row, vertex, sample) tensors of autograd do not fit otherwise);
  * anet_minco_flat_partial_grads_dev (the sibling kernel) on the same trajectories;
  * the same call with the corridor 1e6 m away (no term active: the adjoint is skipped everywhere).
The corridor rows have unit normals and offsets at a percentile drawn from [50, 100] of each row's own sampled terms; the active
share of the (sample, row, vertex) terms is reported.

Every step runs in a child process of its own under its own time limit; the driver stops at the first step that fails.  Times are
device events around one call after warm-up, medians of --reps (>= 20); the torch composition at 131 072 takes seconds per call and
is timed --slow-reps times (default 5), which its entry says.  Prints one JSON line.

    python tools/bench_body_corridor.py [--reps 30] [--step NAME]
"""
import argparse
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ["body_4096", "body_131072"]
LIMIT_S = {"body_4096": 300, "body_131072": 900}
CHUNK = 8192
W, MU, RES, K, M, N, S = 100.0, 0.05, 20, 8, 16, 8, 4


def events_ms(fn, reps, warm=3):
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


def snap_batch(B):
    """Rest-to-rest random-walk problems solved on the device, durations tripled (tools/bench_flatness.py's batch)."""
    import torch
    import allocnet_amd as aa
    from allocnet_amd.synth import random_problem
    head, tail, wps, T = random_problem(np.random.default_rng(7), B, N, 3, rest=True)
    T *= 3.0
    co, _ = aa.minco_solve(head, tail, wps, T, S)
    ld = aa.recommended_ld(B)
    up = lambda a, fill=0.0: torch.cat([torch.from_numpy(a.reshape(B, -1).T.copy()),
                                        torch.full((a.reshape(B, -1).shape[1], ld - B), fill, dtype=torch.float64)], 1).cuda()
    return up(co), up(T, 1.0), ld


def torch_terms(co, T, hp, verts, par, lo, hi):
    """g (M, K, J, N, n) for the lanes lo..hi from differentiable torch operations: co (N*3*D, ld), T (N, ld), hp (N*M*4, ld);
    gradients flow to co and T."""
    import torch
    from allocnet_amd.torch_layer import flat_layer
    D, n = 2 * S, hi - lo
    c = co.view(N, 3, D, -1)[..., lo:hi]
    t = T[:, lo:hi][None] * (torch.arange(RES, device=T.device, dtype=torch.float64) / RES)[:, None, None]     # (J, N, n)
    pw = torch.stack([t ** k for k in range(D)], 0)                                                              # (D, J, N, n)
    state = []
    for d in range(4):
        acc = 0.0
        for col in range(D):
            k = D - 1 - col
            if k >= d:
                acc = acc + math.perm(k, d) * c[:, :, col][None] * pw[k - d][:, :, None]                         # (J, N, 3, n)
        state.append(acc.permute(2, 0, 1, 3).reshape(3, -1).contiguous())                                        # (3, J N n)
    p, v, a, j = state
    zero = torch.zeros(v.shape[1], device=T.device, dtype=torch.float64)
    _, q, _ = flat_layer(v, a, j, zero, zero, par)
    w, x, y, z = q[0], q[1], q[2], q[3]
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)]),
                     torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)]),
                     torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])])          # (3, 3, J N n)
    pts = p[None] + torch.einsum("xye,ky->kxe", R, verts)                                                        # (K, 3, J N n)
    rows = hp.view(N, M, 4, -1)[..., lo:hi]
    pts = pts.view(K, 3, RES, N, n)
    return torch.einsum("imxe,kxjie->mkjie", rows[:, :, :3], pts) - rows[:, :, 3].permute(1, 0, 2)[:, None, None]


def torch_cost(co, T, hp, verts, par, lo, hi):
    import torch
    g = torch_terms(co, T, hp, verts, par, lo, hi)
    xc = torch.clamp(g, min=0.0)
    phi = torch.where(g < 0.0, torch.zeros_like(g), torch.where(g > MU, g - 0.5 * MU, (MU - 0.5 * xc) * (xc / MU) ** 3))
    return W * (T[:, lo:hi] / RES * phi.sum((0, 1, 2))).sum()


def make_corridor(co, T, verts, par, B, ld):
    """hp (N*M*4, ld) with unit normals and each row's offset at a percentile from [50, 100] of its own sampled terms"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randn(N, M, 3, ld, generator=g, device="cuda", dtype=torch.float64)
    hp = torch.zeros(N, M, 4, ld, device="cuda", dtype=torch.float64)
    hp[:, :, :3] = a / a.norm(dim=2, keepdim=True)
    hp = hp.view(N * M * 4, ld)
    pick = torch.rand(M, N, ld, generator=g, device="cuda", dtype=torch.float64) * 0.5 + 0.5
    with torch.no_grad():
        for lo in range(0, B, CHUNK):
            hi = min(lo + CHUNK, B)
            t = torch_terms(co, T, hp, verts, par, lo, hi)                                  # offsets still 0
            t = t.permute(0, 3, 4, 1, 2).reshape(M, N, hi - lo, K * RES).sort(-1).values
            idx = (pick[:, :, lo:hi] * (K * RES - 1)).long()
            hp.view(N, M, 4, ld)[:, :, 3, lo:hi] = t.gather(-1, idx[..., None])[..., 0].permute(1, 0, 2)
    return hp


def body(step, reps, slow_reps):
    import torch
    import allocnet_amd as aa
    B = int(step.rsplit("_", 1)[1])
    co, T, ld = snap_batch(B)
    ctx = aa.default_context(0)
    par = aa.make_flat_params()
    verts = aa.box_body((0.25, 0.25, 0.05))
    d_verts = torch.from_numpy(verts).cuda()
    hp = make_corridor(co, T, d_verts, par, B, ld)
    bpen = aa.make_body_penalty(verts, w=W, smooth_mu=MU, res=RES, poly_rows=M)
    new = lambda rows: torch.zeros(rows, ld, device="cuda", dtype=torch.float64)
    gC, gT, pc = new(N * 3 * 2 * S), new(N), new(N)
    out = dict(batch=B, pieces=N, order=S, res=RES, body_vertices=K, rows_per_polytope=M)
    pairs, samples = B * N, B * N * RES
    run = lambda rows, acc=False: (lambda: aa.minco_body_partial_grads_dev(par, bpen, S, N, B, co, T, rows, gC, gT, pc, accumulate=acc))
    far = hp.clone()
    far.view(N, M, 4, ld)[:, :, 3] += 1e6
    for name, fn in (("body_active", run(hp)), ("body_active_accumulate", run(hp, True)), ("body_corridor_far", run(far))):
        med, mn = events_ms(fn, reps)
        out[name] = dict(median_ms=med, min_ms=mn, ns_per_sample=med * 1e6 / samples,
                         ns_per_term=med * 1e6 / (samples * K * M))
    run(hp)()
    torch.cuda.synchronize()
    kernel_cost = float(pc[:, :B].sum())
    out["share_of_pieces_with_an_active_term"] = float((pc[:, :B] > 0).double().mean())
    # the torch composition: cost and gradients w.r.t. coefficients and durations, chunk by chunk
    cg, Tg = co.clone().requires_grad_(True), T.clone().requires_grad_(True)
    total = [0.0]

    def composed():
        cg.grad = Tg.grad = None
        total[0] = 0.0
        for lo in range(0, B, CHUNK):
            c = torch_cost(cg, Tg, hp, d_verts, par, lo, min(lo + CHUNK, B))
            c.backward()
            total[0] = total[0] + c.detach()
    r = reps if B <= CHUNK else slow_reps
    med, mn = events_ms(composed, r, warm=1)
    out["torch_composition"] = dict(median_ms=med, min_ms=mn, reps=r, chunk=min(CHUNK, B))
    out["torch_over_kernel"] = med / out["body_active"]["median_ms"]
    out["cost_kernel_against_torch_relative"] = abs(kernel_cost - float(total[0])) / abs(float(total[0]))
    eC = (cg.grad[:, :B] - gC[:, :B]).abs().max().item() / max(1.0, cg.grad[:, :B].abs().max().item())
    out["gdC_kernel_against_torch"] = eC
    with torch.no_grad():
        act = cnt = 0
        for lo in range(0, B, CHUNK):
            t = torch_terms(co, T, hp, d_verts, par, lo, min(lo + CHUNK, B))
            act, cnt = act + int((t > 0).sum()), cnt + t.numel()
    out["active_share_of_terms"] = act / cnt
    # the sibling kernel on the same trajectories
    fpen = aa.make_flat_penalty(w_thrust=30.0, w_tilt=200.0, w_bdr=10.0, smooth_mu=0.01, min_thrust=9.6, max_thrust=10.2,
                                max_tilt=0.12, max_bdr=0.6, res=RES)
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    ref = lambda o: ctypes.cast(ctypes.pointer(o), ctypes.c_void_p)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    flat = lambda: ctx.check(ctx.lib.anet_minco_flat_partial_grads_dev(ctx.handle, ref(par), ref(fpen), S, N, B, ld, q(co), q(T), 0,
                                                                       q(gC), q(gT), q(pc), st))
    med, mn = events_ms(flat, reps)
    out["flat_partial_grads"] = dict(median_ms=med, min_ms=mn, ns_per_sample=med * 1e6 / samples)
    out["body_over_flat"] = out["body_active"]["median_ms"] / med
    # the sampled margin at the same shape
    margin = lambda: aa.traj_body_margin_dev(par, bpen, S, N, B, co, T, hp, margin=gT, t=pc)
    med, mn = events_ms(margin, reps)
    out["body_margin"] = dict(median_ms=med, min_ms=mn, ns_per_sample=med * 1e6 / (pairs * (RES + 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--slow-reps", type=int, default=5)
    ap.add_argument("--step", default=None, help="one of %s" % STEPS)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.step:
        print(json.dumps(body(args.step, args.reps, args.slow_reps)))
        return 0
    out = {}
    for step in STEPS:
        limit = LIMIT_S.get(step, 300)
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--slow-reps",
                                  str(args.slow_reps)], capture_output=True, text=True, timeout=limit)
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
