"""The distance field of the voxel map on the MI355X (csrc/distance_kernels.h) on the launch-file map of tools/bench_voxel_map.py
(400 x 400 x 50 voxels of 0.1 m, a forest cloud of ~1e6 points, dilate(2)).  Steps:
  transform       anet_voxel_distance_dev (walls) beside scipy.ndimage.distance_transform_edt on the host, both polarities (one after
                  the other, and the two in two threads), checked for equality; dilate(5) of the same map for orientation
  query           anet_voxel_distance_query_dev at 1e6 uniform points, with and without the gradient
  penalty_131072  anet_minco_obstacle_partial_grads_dev at B x 8 snap pieces x 20 samples beside the route a user had before it:
  penalty_4096    anet_traj_eval_dev at the sample times, torch.nn.functional.grid_sample (trilinear, border) on the float64 field
                  of centre values, the smoothed penalty in torch and autograd back to the sampled positions.  The torch route is NOT
                  charged for the contraction of the sample gradients to coefficient and duration gradients.
Each step runs in a child process under its own `timeout -k 10`.  Device times are events around one call after 5 warm-ups, medians
of --reps; host times are wall clock, medians of --host-reps.  Prints one JSON line.

    python tools/bench_voxel_distance.py [--reps 20] [--host-reps 3] [--step NAME]
"""
import argparse
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ["transform", "query", "penalty_4096", "penalty_131072"]
SIZE, ORIGIN, SCALE = (400, 400, 50), (-20.0, -20.0, 0.0), 0.1
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


def forest_map(points=1_000_000):
    import torch
    import allocnet_amd as aa
    from allocnet_amd.synth import forest_cloud, forest_route
    rec = forest_cloud(np.random.default_rng(0), n_points=points, clear_route=forest_route())
    vm = aa.VoxelMap(SIZE, ORIGIN, SCALE)
    vm.setOccupiedCloud(torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).to(vm.device), 16)
    vm.dilate(2)
    torch.cuda.synchronize()
    return vm


def run_transform(reps, host_reps):
    import torch
    import allocnet_amd as aa
    from scipy import ndimage
    vm = forest_map()
    n = int(np.prod(SIZE))
    out = dict(map=list(SIZE), voxels=n, blocked=int((vm.voxels_dev != 0).sum()))
    for walls in (1, 0):
        sd2 = torch.empty(n, dtype=torch.int32, device=vm.device)
        med, mn = events_ms(lambda: aa.distance_transform_dev(vm, vm.voxels_dev, walls, out=sd2), reps)
        # traffic the algorithm needs: the bytes once, the field written by three passes and read by two
        out[f"device_walls{walls}"] = dict(median_ms=med, min_ms=mn, voxels_per_s=n / (med * 1e-3),
                                           gb_per_s=(n * (1 + 5 * 4)) / (med * 1e-3) / 1e9)
    base = vm.voxels_dev.clone()

    def fresh_dilate():
        vm.voxels_dev.copy_(base)
        vm.dilate(5)
    out["grid_copy_ms"] = events_ms(lambda: vm.voxels_dev.copy_(base), reps)[0]
    t = []
    for _ in range(max(3, reps // 4)):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fresh_dilate(); torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    out["dilate5_ms"] = float(np.median(t))                              # includes the reset copy, the compaction and a read-back
    vm.voxels_dev.copy_(base)
    torch.cuda.synchronize()
    blocked = (base.cpu().numpy() != 0).reshape(SIZE[2], SIZE[1], SIZE[0])
    padded = np.pad(blocked, 1, constant_values=True)

    def host(pool):
        a = pool.submit(lambda: ndimage.distance_transform_edt(~padded)[1:-1, 1:-1, 1:-1])
        b = pool.submit(lambda: ndimage.distance_transform_edt(blocked))
        return a.result(), b.result()
    for threads in (1, 2):
        pool = ThreadPoolExecutor(threads)
        ts = []
        for _ in range(host_reps):
            t0 = time.perf_counter(); dp, dm = host(pool); ts.append((time.perf_counter() - t0) * 1e3)
        pool.shutdown()
        out[f"scipy_edt_both_polarities_ms_{threads}t"] = float(np.median(ts))
    want = np.where(blocked, -np.rint(dm * dm), np.rint(dp * dp)).astype(np.int32).reshape(-1)
    got = aa.distance_transform_dev(vm, vm.voxels_dev, 1).cpu().numpy()
    out["device_equals_scipy"] = bool(np.array_equal(got, want))
    out["device_over_scipy_1t"] = out["device_walls1"]["median_ms"] / out["scipy_edt_both_polarities_ms_1t"]
    return out


def run_query(reps):
    import torch
    import allocnet_amd as aa
    vm = forest_map()
    sd2 = vm.distance_field()
    n = 1_000_000
    lo, hi = vm.getOrigin(), vm.getCorner()
    pos = torch.from_numpy(np.random.default_rng(1).uniform(lo, hi, (n, 3))).to(vm.device)
    out = dict(points=n)
    for grad in (True, False):
        med, mn = events_ms(lambda: aa.distance_query_dev(vm, sd2, pos, grad=grad), reps)
        nbytes = n * (24 + 8 + (24 if grad else 0))                       # positions in, dist (and grad) out; the gathers hit the cache
        out["dist_grad" if grad else "dist"] = dict(median_ms=med, min_ms=mn, points_per_s=n / (med * 1e-3),
                                                    gb_per_s_streamed=nbytes / (med * 1e-3) / 1e9,
                                                    gb_per_s_gathered=n * 32 / (med * 1e-3) / 1e9)
    return out


def run_penalty(B, reps):
    import ctypes
    import torch
    import torch.nn.functional as F
    import allocnet_amd as aa
    vm = forest_map()
    sd2 = vm.distance_field()
    N, s = 8, 4
    D = 2 * s
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
    pen = aa.make_obstacle_penalty(w=100.0, smooth_mu=0.05, clearance=0.5, res=RES)
    ld = aa.recommended_ld(B)

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a.reshape(B, -1).T)).cuda()
        return torch.cat([t, torch.ones(t.shape[0], ld - B, dtype=torch.float64, device="cuda")], 1).contiguous()
    d_co, d_T = up(co), up(T)
    new = lambda *shape: torch.zeros(*shape, device="cuda", dtype=torch.float64)
    gC, gT, pc = new(N * 3 * D, ld), new(N, ld), new(N, ld)
    ctx = aa.default_context(0)
    kernel = lambda: aa.minco_obstacle_partial_grads_dev(pen, s, N, B, d_co, d_T, (vm, sd2), gC, gT, pc, ctx=ctx)
    med, mn = events_ms(kernel, reps)
    kernel()
    torch.cuda.synchronize()
    cost = float(pc[:, :B].sum())
    samples = B * N * RES

    # the torch route
    S = N * RES
    sigma = torch.arange(RES, device="cuda", dtype=torch.float64) / RES
    Te = d_T[:, :B].T
    K = torch.cumsum(Te, 1) - Te
    tq = new(S, ld)
    tq[:, :B] = (K[:, :, None] + sigma[None, None, :] * Te[:, :, None]).reshape(B, S).T
    pos = new(S * 3, ld)
    q_ = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    s2 = sd2.to(torch.float64)
    field = (SCALE * torch.sign(s2) * torch.sqrt(s2.abs())).reshape(1, 1, SIZE[2], SIZE[1], SIZE[0])
    oc = torch.tensor(ORIGIN, device="cuda", dtype=torch.float64) + 0.5 * SCALE
    span = torch.tensor([SIZE[0] - 1, SIZE[1] - 1, SIZE[2] - 1], device="cuda", dtype=torch.float64)
    wgt = (Te[:, :, None].expand(B, N, RES).reshape(B, S) / RES)
    out = {}

    def ev():
        ctx.check(ctx.lib.anet_traj_eval_dev(ctx.handle, s, N, B, ld, q_(d_co), q_(d_T), S, q_(tq), 0, q_(pos), st))

    def penalty():
        p = pos.view(S, 3, ld)[..., :B].permute(2, 0, 1).contiguous().requires_grad_(True)      # (B, S, 3)
        g = (2.0 * ((p - oc) / SCALE) / span - 1.0).reshape(1, B * S, 1, 1, 3)
        d = F.grid_sample(field, g, mode="bilinear", padding_mode="border", align_corners=True).reshape(B, S)
        x = pen.clearance - d
        xd = (x / pen.smooth_mu).clamp(0.0, 1.0)
        f = torch.where(x > pen.smooth_mu, x - 0.5 * pen.smooth_mu, (pen.smooth_mu - 0.5 * xd * pen.smooth_mu) * xd ** 3)
        J = (pen.w * f * wgt).sum()
        J.backward()
        out["J"] = J.detach()

    def route():
        ev(); penalty()
    parts = {name: events_ms(fn, reps)[0] for name, fn in (("traj_eval_ms", ev), ("grid_sample_penalty_autograd_ms", penalty))}
    med2, mn2 = events_ms(route, reps)
    route()
    torch.cuda.synchronize()
    return dict(trajectories=B, pieces=N, order=s, res=RES, samples=samples,
                kernel=dict(median_ms=med, min_ms=mn, samples_per_s=samples / (med * 1e-3),
                            gb_per_s_gathered=samples * 32 / (med * 1e-3) / 1e9,
                            gb_per_s_streamed=B * (N * 3 * D * 2 + 3 * N) * 8 / (med * 1e-3) / 1e9),
                torch_route=dict(median_ms=med2, min_ms=mn2, **parts),
                kernel_over_torch_route=med / med2, cost=cost, torch_cost=float(out["J"]),
                cost_relative_difference=abs(float(out["J"]) - cost) / max(abs(cost), 1e-300))


def run(step, reps, host_reps):
    if step == "transform":
        return run_transform(reps, host_reps)
    if step == "query":
        return run_query(reps)
    return run_penalty(int(step.rsplit("_", 1)[1]), reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--step", default=None, help="one of %s" % STEPS)
    args = ap.parse_args()
    if args.step:
        print(json.dumps(run(args.step, args.reps, args.host_reps)))
        return 0
    out = {}
    for step in STEPS:
        res = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--step", step, "--reps",
                              str(args.reps), "--host-reps", str(args.host_reps)], capture_output=True, text=True)
        if res.returncode != 0:                         # nothing more is started on the device after a step that hung or failed
            out[step] = dict(error=f"exit status {res.returncode}" + (" (time limit)" if res.returncode in (124, 137) else ""),
                             stderr=res.stderr[-800:])
            break
        out[step] = json.loads(res.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return 0 if all("error" not in v for v in out.values()) and len(out) == len(STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
