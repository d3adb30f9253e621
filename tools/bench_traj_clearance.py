"""Exact clearance to obstacle points on the MI355X (anet_traj_clearance_dev, csrc/clearance_kernels.h) beside the route that
existed before it: anet_traj_eval_dev at res = 20 samples per piece (j T_i / 20, j = 0 .. 20), then a torch distance matrix
(torch.cdist) against the piece's points and its minimum.  A 200 x 200 x 40 map of 0.25 m voxels with pillars and slabs dilated by
one voxel; a base route of eight 2 m segments through it and, per segment, the box that holds it and 3 m around it
(convexCover's per-segment selection): VoxelMap.gather_boxes gives the eight per-piece sets.  The batch is 4096 or 131 072
candidate trajectories of eight snap pieces from minco_solve through the base waypoints moved by 0.3 m each (8192 distinct ones;
larger batches repeat them on the device), which is what candidate ranking looks at.  Steps:
  box_4096, box_131072   per-piece sets, counts as gather_boxes returns them
  shared_4096            one cloud for every piece: the surface points within 4 m of the route's bounding box
Reported per step: the time of each route, by how much the sampled clearance exceeds the exact one (median, 90 %, 99 %, worst),
and the points per piece that survive the cheap pass (marked for refinement), counted on the host for 256 trajectories with the
kernel's own test against the `best` of the first pass: an upper estimate of what the kernel refines, which tests a marked point
again when it visits it.

Every step runs in a child process of its own under its own `timeout -k 10`; the driver stops at the first step that fails.  Times
are device events around one call after 5 warm-ups, medians of --reps (30).  Prints one JSON line.

    python tools/bench_traj_clearance.py [--reps 30] [--step NAME]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
from math import comb

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ["box_4096", "box_131072", "shared_4096"]
LIMIT_S = {"box_131072": 420}
BASE = 8192
SIZE, ORIGIN, SCALE = (200, 200, 40), (-25.0, -25.0, 0.0), 0.25
RES = 20
K, SLACK, EPS = 9, 16.0, 2.220446049250313e-16           # csrc/clearance_kernels.h


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


def box_rows(lo, hi):
    """six rows h . [p; 1] < 0 inside [lo, hi]"""
    bd = np.zeros((6, 4))
    for ax in range(3):
        bd[2 * ax, ax], bd[2 * ax, 3] = 1.0, -hi[ax]
        bd[2 * ax + 1, ax], bd[2 * ax + 1, 3] = -1.0, lo[ax]
    return bd


def marked_per_piece(co, T, sets, counts):
    """the kernel's cheap pass on the host: per (trajectory, piece) the number of points with ub_j < best + L h / 2 + slack"""
    Bm, N, _, D = co.shape
    n = D - 1
    u = co[..., ::-1] * T[:, :, None, None] ** np.arange(D)[None, None, None]
    W = np.array([[comb(i, k) / comb(n, k) if k <= i else 0.0 for k in range(D)] for i in range(D)])
    bz = u @ W.T
    Lh2 = np.sqrt((np.diff(bz, axis=-1) ** 2).sum(axis=2).max(axis=-1)) * (n * 0.5 / (K - 1))
    taus = np.arange(K) / (K - 1)
    pos = u @ (taus[None] ** np.arange(D)[:, None])                            # (Bm, N, 3, K)
    A1 = np.abs(u).sum(axis=(2, 3))
    out = np.zeros((Bm, N), dtype=np.int64)
    for i in range(N):
        q = sets[i][:counts[i]] if sets.ndim == 3 else sets[:counts[0]]
        if len(q) == 0:
            continue
        d2 = ((pos[:, i, :, :, None] - q.T[None, :, None, :]) ** 2).sum(axis=1).min(axis=1)          # (Bm, P)
        thr = np.sqrt(d2.min(axis=1))[:, None] + Lh2[:, i, None] + SLACK * EPS * (A1[:, i, None] + np.abs(q).sum(axis=1)[None])
        out[:, i] = (d2 < thr * thr).sum(axis=1)
    return out


def run(step, reps):
    import torch
    import allocnet_amd as aa
    kind, B = step.rsplit("_", 1)[0], int(step.rsplit("_", 1)[1])
    N, s = 8, 4
    Bb = min(B, BASE)
    rng = np.random.default_rng(7)
    vm = planner_map(aa, rng)
    base = np.empty((N + 1, 3))
    base[0] = [-8.0, -6.0, 3.0]
    for i in range(N):
        step_ = rng.normal(size=3) * np.array([1.0, 1.0, 0.2])
        base[i + 1] = base[i] + 2.0 * step_ / np.linalg.norm(step_)
    pts = base[None] + rng.normal(size=(Bb, N + 1, 3)) * 0.3
    head, tail = np.zeros((Bb, 3, 3)), np.zeros((Bb, 3, 3))
    head[:, :, 0], tail[:, :, 0] = pts[:, 0], pts[:, -1]
    T = np.linalg.norm(np.diff(pts, axis=1), axis=2) / 1.5 + 0.4
    co, _ = aa.minco_solve(head, tail, pts[:, 1:-1], T, s)
    if kind == "box":
        bd = np.stack([box_rows(np.minimum(base[i], base[i + 1]) - 3.0, np.maximum(base[i], base[i + 1]) + 3.0) for i in range(N)])
        d_pts, counts = vm.gather_boxes(bd)
    else:
        d_pts, counts = vm.gather_boxes(box_rows(base.min(axis=0) - 4.0, base.max(axis=0) + 4.0)[None])
        d_pts = d_pts[0].contiguous()
    d_cnt = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    ld = aa.recommended_ld(B)

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a.reshape(Bb, -1).T)).cuda().repeat(1, B // Bb)
        return torch.cat([t, torch.ones(t.shape[0], ld - B, dtype=torch.float64, device="cuda")], 1).contiguous()
    d_co, d_T = up(co), up(T)
    ctx = aa.default_context(0)
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_c = torch.zeros(N, ld, device="cuda", dtype=torch.float64)
    d_p = torch.zeros(N, ld, device="cuda", dtype=torch.int32)
    d_t = torch.zeros(N, ld, device="cuda", dtype=torch.float64)
    exact = lambda: aa.traj_clearance_dev(d_co, d_T, d_pts, s, N, B, counts=d_cnt, clearance=d_c, point=d_p, t=d_t, ctx=ctx)
    med, mn = events_ms(exact, reps)
    # the sampled route: N (RES + 1) absolute times per trajectory, positions [nq * 3][ld], then per piece a distance matrix
    nq = N * (RES + 1)
    begin = torch.cumsum(d_T, 0) - d_T
    frac = torch.arange(RES + 1, device="cuda", dtype=torch.float64) / RES
    tq = (begin[:, None, :] + frac[None, :, None] * d_T[:, None, :]).reshape(nq, ld).contiguous()
    pos = torch.zeros(nq * 3, ld, device="cuda", dtype=torch.float64)
    d_s = torch.zeros(N, B, device="cuda", dtype=torch.float64)
    sets = [(d_pts[i] if kind == "box" else d_pts)[:int(min(counts[i if kind == "box" else 0], d_pts.shape[-2]))] for i in range(N)]
    chunk = max(1, (1 << 28) // max(1, max(int(x.shape[0]) for x in sets)))     # at most 2 GiB of distances at a time
    chunk = max(RES + 1, chunk - chunk % (RES + 1))

    def ev():
        ctx.check(ctx.lib.anet_traj_eval_dev(ctx.handle, s, N, B, ld, q(d_co), q(d_T), nq, q(tq), 0, q(pos), st))

    def dist():
        p4 = pos.view(N, RES + 1, 3, ld)
        for i in range(N):
            if sets[i].shape[0] == 0:                   # no point in this box: +inf, as the exact route answers
                d_s[i].fill_(float("inf"))
                continue
            flat = p4[i, :, :, :B].permute(2, 0, 1).reshape(B * (RES + 1), 3)
            for a in range(0, flat.shape[0], chunk):
                d_s[i].view(-1)[a // (RES + 1):(a + chunk) // (RES + 1)] = \
                    torch.cdist(flat[a:a + chunk], sets[i]).min(dim=1).values.view(-1, RES + 1).min(dim=1).values

    def sampled():
        ev(); dist()
    parts = {name: events_ms(fn, reps)[0] for name, fn in (("traj_eval_ms", ev), ("distance_ms", dist))}
    med2, mn2 = events_ms(sampled, reps)
    exact(); sampled()
    torch.cuda.synchronize()
    both = torch.isfinite(d_s[:, :Bb]) & torch.isfinite(d_c[:, :Bb])
    assert bool(both.any()), "no piece has a point in its set"
    over = (d_s[:, :Bb] - d_c[:, :Bb])[both].cpu().numpy().ravel()
    # (the first sample of pieces 1.. sits on a junction, which traj_eval gives to the earlier piece: the same position)
    h_pts = d_pts.cpu().numpy()
    marked = marked_per_piece(co[:256], T[:256], h_pts, np.minimum(counts, h_pts.shape[-2]))
    return dict(batch=B, pieces=N, order=s, res=RES, sets=kind, points_per_set=[int(x.shape[0]) for x in (sets if kind == "box" else sets[:1])],
                distinct_trajectories=Bb,
                exact=dict(median_ms=med, min_ms=mn, ns_per_piece=med * 1e6 / (B * N)),
                sampled=dict(median_ms=med2, min_ms=mn2, ns_per_piece=med2 * 1e6 / (B * N), **parts),
                exact_over_sampled=med / med2,
                clearance_m=dict(min=float(d_c[:, :Bb][both].min()), median=float(d_c[:, :Bb][both].median())),
                share_of_pieces_with_points=float(both.double().mean()),
                sampled_minus_exact_m=dict(min=float(over.min()), median=float(np.median(over)), p90=float(np.quantile(over, 0.9)),
                                           p99=float(np.quantile(over, 0.99)), worst=float(over.max())),
                marked_points_per_piece=dict(mean=float(marked.mean()), max=int(marked.max())))


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
