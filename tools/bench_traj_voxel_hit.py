"""Exact first collision with the voxel map on the MI355X (anet_traj_voxel_hit_dev, csrc/voxel_hit_kernels.h) beside the route
that existed before it: anet_traj_eval_dev at res = 20 samples per piece (j T_i / 20, j = 0 .. 20), the positions turned to
[n][3] on the device, then anet_voxel_query_dev.  A 200 x 200 x 40 map of 0.25 m voxels (1.6 MB) with pillars and slabs dilated by
one voxel, 4096 and 131 072 trajectories of eight snap pieces from minco_solve through random waypoints inside the map (8192
distinct ones; larger batches repeat them on the device).  Reported: the time of each route, the share of pieces each calls
free, and how many pieces the sampled route calls free that the exact one does not (and the reverse, which only rounding at a cell
face can produce).

Every step runs in a child process of its own under its own `timeout -k 10`; the driver stops at the first step that fails.  Times
are device events around one call after 5 warm-ups, medians of --reps (30).  Prints one JSON line.

    python tools/bench_traj_voxel_hit.py [--reps 30] [--step NAME]
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

STEPS = ["hit_4096", "hit_131072"]
LIMIT_S = {"hit_131072": 420}
BASE = 8192
SIZE, ORIGIN, SCALE = (200, 200, 40), (-25.0, -25.0, 0.0), 0.25
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


def planner_map(aa, rng):
    """pillars (1 m square, full height) and slabs (4 m x 0.5 m, 2 to 6 m high), dilated by one voxel"""
    vm = aa.VoxelMap(SIZE, ORIGIN, SCALE)
    ids = []
    for _ in range(90):
        x, y = rng.integers(4, SIZE[0] - 8), rng.integers(4, SIZE[1] - 8)
        ids.append(np.stack(np.meshgrid(np.arange(x, x + 4), np.arange(y, y + 4), np.arange(SIZE[2]), indexing="ij"), -1).reshape(-1, 3))
    for _ in range(40):
        x, y, h = rng.integers(4, SIZE[0] - 20), rng.integers(4, SIZE[1] - 20), rng.integers(8, 24)
        w = (16, 2) if rng.random() < 0.5 else (2, 16)
        ids.append(np.stack(np.meshgrid(np.arange(x, x + w[0]), np.arange(y, y + w[1]), np.arange(h), indexing="ij"), -1).reshape(-1, 3))
    vm.setOccupied(np.concatenate(ids).astype(np.int32))
    vm.dilate(1)
    return vm


def hit(step, reps):
    import torch
    import allocnet_amd as aa
    B, N, s = int(step.rsplit("_", 1)[1]), 8, 4
    Bb = min(B, BASE)
    rng = np.random.default_rng(7)
    vm = planner_map(aa, rng)
    lo, hi = np.array(ORIGIN) + 2.0, np.array(ORIGIN) + np.array(SIZE) * SCALE - 2.0
    pts = np.empty((Bb, N + 1, 3))
    pts[:, 0] = rng.uniform(lo, hi, (Bb, 3))
    for i in range(N):       # steps of about 2 m, reflected into the map
        p = pts[:, i] + rng.normal(size=(Bb, 3)) * np.array([1.5, 1.5, 0.4])
        pts[:, i + 1] = np.clip(p, lo, hi)
    head, tail = np.zeros((Bb, 3, 3)), np.zeros((Bb, 3, 3))
    head[:, :, 0], tail[:, :, 0] = pts[:, 0], pts[:, -1]
    T = np.linalg.norm(np.diff(pts, axis=1), axis=2) / 1.5 + 0.4
    co, _ = aa.minco_solve(head, tail, pts[:, 1:-1], T, s)
    ld = aa.recommended_ld(B)

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a.reshape(Bb, -1).T)).cuda().repeat(1, B // Bb)
        return torch.cat([t, torch.ones(t.shape[0], ld - B, dtype=torch.float64, device="cuda")], 1).contiguous()
    d_co, d_T = up(co), up(T)
    ctx = aa.default_context(0)
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_t = torch.zeros(N, ld, device="cuda", dtype=torch.float64)
    d_v = torch.zeros(N, ld, device="cuda", dtype=torch.int32)
    exact = lambda: aa.traj_voxel_hit_dev(d_co, d_T, vm, s, N, B, t_hit=d_t, voxel=d_v, ctx=ctx)
    med, mn = events_ms(exact, reps)
    # the sampled route: N (RES + 1) absolute times per trajectory, positions [nq * 3][ld] -> [B nq][3] -> bytes
    nq = N * (RES + 1)
    begin = torch.cumsum(d_T, 0) - d_T
    frac = torch.arange(RES + 1, device="cuda", dtype=torch.float64) / RES
    tq = (begin[:, None, :] + frac[None, :, None] * d_T[:, None, :]).reshape(nq, ld).contiguous()
    pos = torch.zeros(nq * 3, ld, device="cuda", dtype=torch.float64)
    flat = torch.zeros(B * nq, 3, device="cuda", dtype=torch.float64)
    blocked = torch.zeros(B * nq, device="cuda", dtype=torch.uint8)
    grid = ctypes.byref(vm._grid)

    def ev():
        ctx.check(ctx.lib.anet_traj_eval_dev(ctx.handle, s, N, B, ld, q(d_co), q(d_T), nq, q(tq), 0, q(pos), st))

    def turn():
        flat.copy_(pos.view(nq, 3, ld)[:, :, :B].permute(2, 0, 1).reshape(B * nq, 3))

    def qu():
        ctx.check(ctx.lib.anet_voxel_query_dev(ctx.handle, grid, q(vm.voxels_dev), q(flat), B * nq, q(blocked), st))

    def sampled():
        ev(); turn(); qu()
    parts = {name: events_ms(fn, reps)[0] for name, fn in (("traj_eval_ms", ev), ("turn_ms", turn), ("query_ms", qu))}
    med2, mn2 = events_ms(sampled, reps)
    exact(); sampled()
    torch.cuda.synchronize()
    t_hit, vox = d_t[:, :B].T, d_v[:, :B].T                                   # (B, N)
    # piece i owns samples i (RES + 1) .. i (RES + 1) + RES; the query clamps nothing: times beyond a piece's end belong to the next
    samp_free = ~(blocked.view(B, N, RES + 1) != 0).any(dim=2)
    exact_free = torch.isinf(t_hit) & (t_hit > 0)
    occ = float((vm.voxels_dev != 0).double().mean())
    return dict(batch=B, pieces=N, order=s, res=RES, map=list(SIZE), occupancy=occ, distinct_trajectories=Bb,
                exact=dict(median_ms=med, min_ms=mn, ns_per_piece=med * 1e6 / (B * N)),
                sampled=dict(median_ms=med2, min_ms=mn2, ns_per_piece=med2 * 1e6 / (B * N), **parts),
                exact_over_sampled=med / med2,
                share_of_pieces_free_exact=float(exact_free.double().mean()), share_of_pieces_free_sampled=float(samp_free.double().mean()),
                pieces_sampled_free_exact_not=int((samp_free & ~exact_free).sum()), pieces_exact_free_sampled_not=int((~samp_free & exact_free).sum()),
                pieces_undecided=int(((vox == -3) & torch.isfinite(t_hit)).sum()),
                trajectories_sampled_free_exact_not=int((samp_free.all(dim=1) & ~exact_free.all(dim=1)).sum()),
                share_of_trajectories_free_exact=float(exact_free.all(dim=1).double().mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", default=None, help="one of %s" % STEPS)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.step:
        print(json.dumps(hit(args.step, args.reps)))
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
