#!/usr/bin/env python3
"""SHA-256 of every output array of the four exact trajectory queries' device entry points (anet_traj_row_margin_dev,
anet_traj_voxel_hit_dev, anet_traj_clearance_dev, anet_traj_separation_dev), one line per array: two builds compute the same
bits exactly when their lines are equal (run both through tools/ab_head.sh and compare the OLD and NEW blocks).
    python tools/hash_traj_queries.py                 # every step
    python tools/hash_traj_queries.py --step margin   # one of: margin, hit, clearance, separation (what the children run)
Inputs: every case of the four golden fixtures, through the loaders of the GPU tests; and per order 2, 3, 4 a batch of 70
trajectories (one full wave and a part) of 3 pieces at ld = 96 from a seeded minco_solve: margins against 9 rows (two of them
padding) at derivative orders 0, 1, 2; clearance to a shared cloud of 130 points (two full tiles and a part, one point not
finite) and to per-piece sets with counts; separation of all pairs a <= b of the first 24 with staggered t0, cutoff off and at
1 m; first hits on a 40 x 40 x 10 map.  Every step runs in a child process under its own `timeout -k 10`; the tool ends at
the first step that fails."""
import argparse
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # the tree this copy of the tool lies in
sys.path.insert(0, ROOT)

STEPS = ["margin", "hit", "clearance", "separation"]
B, N, LD = 70, 3, 96


def digest(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()[:32]


def emit(tag, names, tensors, cols=None):
    for name, t in zip(names, tensors):
        print(tag, name, digest(t if cols is None else t[..., :cols]), flush=True)


def batch(s):
    """70 seeded trajectories of 3 pieces of order s: host coefficients (B, N, 3, 2s), durations (B, N), corridor rows (B, N, 16, 4)"""
    import allocnet_amd as aa
    from allocnet_amd.synth import corridor_problem
    head, tail, wps, T, hp = corridor_problem(np.random.default_rng(500 + s), B, N, min(s, 3), 16)
    head[:, :, 1:] = np.random.default_rng(600 + s).normal(size=head[:, :, 1:].shape) * 0.5
    co, _ = aa.minco_solve(head, tail, wps, T, s)
    return co, T, hp


def bm(a, nb, ld):
    """(nb, ...) host array -> batch-minor (F, ld) device tensor, junk behind the batch"""
    import torch
    f = np.asarray(a, dtype=np.float64).reshape(nb, -1)
    t = torch.full((f.shape[1], ld), 7.0, device="cuda", dtype=torch.float64)
    t[:, :nb] = torch.from_numpy(np.ascontiguousarray(f.T)).cuda()
    return t


def step_margin(ctx):
    import torch
    from tests import test_corridor_margin_gpu as tg
    fx = np.load(os.path.join(tg.GOLDEN, "corridor_margin_cases.npz"))
    q = lambda x: ctypes.c_void_p(x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(tag, co, T, rows, d, nb, n, ld):
        s, M = co.shape[-1] // 2, rows.shape[2]
        outs = (torch.full((n, ld), -7.0, device="cuda", dtype=torch.float64), torch.full((n, ld), -7, device="cuda", dtype=torch.int32),
                torch.full((n, ld), -7.0, device="cuda", dtype=torch.float64))
        ctx.check(ctx.lib.anet_traj_row_margin_dev(ctx.handle, s, n, nb, ld, q(bm(co, nb, ld)), q(bm(T, nb, ld)), d, M,
                                                   q(bm(rows, nb, ld)), q(outs[0]), q(outs[1]), q(outs[2]), stream))
        torch.cuda.synchronize()
        emit(tag, ("margin", "row", "t"), outs, nb)

    for s in (2, 3, 4):
        for d in (0, 1, 2):
            sel = np.flatnonzero((fx["s"] == s) & (fx["d"] == d))       # every golden case of (s, d), one piece each
            call(f"margin golden s={s} d={d} cases={len(sel)}", fx["cm"][sel][:, None, :, :2 * s], fx["T"][sel][:, None],
                 fx["rows"][sel][:, None], d, len(sel), 1, len(sel) + 5)
    for s in (2, 3, 4):
        co, T, hp = batch(s)
        rows = hp[:, :, :9].copy()
        rows[:, :, [2, 7]] = 0.0                                        # two padding rows
        for d in (0, 1, 2):
            call(f"margin batch s={s} d={d}", co, T, rows, d, B, N, LD)


def step_hit(ctx):
    import torch
    import allocnet_amd as aa
    from tests import test_traj_voxel_hit_gpu as tg
    fx = np.load(os.path.join(tg.GOLDEN, "traj_voxel_hit_cases.npz"))
    g, unit = tg.hm.Grid(tg.SIZE, tg.ORIGIN, tg.SCALE), tg.hm.Grid((1, 1, 1), (0.0, 0.0, 0.0), 1.0)      # the four grids of the fixture
    n = tg.SIZE[0] * tg.SIZE[1] * tg.SIZE[2]
    maps = [tg.make_map(ctx, gr, vx) for gr, vx in
            ((g, fx["vox0"]), (g, np.zeros(n, dtype=np.uint8)), (g, fx["vox2"]), (unit, np.zeros(1, dtype=np.uint8)))]

    def call(tag, vm, co, T, nb, n, ld):
        outs = (torch.full((n, ld), -7.0, device="cuda", dtype=torch.float64), torch.full((n, ld), -7, device="cuda", dtype=torch.int32))
        aa.traj_voxel_hit_dev(bm(co, nb, ld), bm(T, nb, ld), vm, co.shape[-1] // 2, n, nb, t_hit=outs[0], voxel=outs[1], ctx=ctx)
        torch.cuda.synchronize()
        emit(tag, ("t_hit", "voxel"), outs, nb)

    for s in (2, 3, 4):
        for gid, vm in enumerate(maps):
            sel = np.flatnonzero((fx["s"] == s) & (fx["grid"] == gid))
            call(f"hit golden s={s} grid={gid} cases={len(sel)}", vm, fx["cm"][sel][:, None, :, :2 * s], fx["T"][sel][:, None],
                 len(sel), 1, len(sel) + 5)
    # a 40 x 40 x 10 map of 0.5 m voxels around the batch: 2 % of the voxels blocked, the start of every trajectory free
    rng = np.random.default_rng(77)
    vox = (rng.random((10, 40, 40)) < 0.02).astype(np.uint8)
    vox[:, 18:22, 18:22] = 0
    vm = aa.VoxelMap((40, 40, 10), (-10.0, -10.0, -0.5), 0.5, ctx=ctx)
    vm.voxels_dev.copy_(torch.from_numpy(vox.ravel()))
    torch.cuda.synchronize()
    for s in (2, 3, 4):
        co, T, _ = batch(s)
        call(f"hit batch s={s}", vm, co, T, B, N, LD)


def step_clearance(ctx):
    import torch
    import allocnet_amd as aa
    from tests import test_traj_clearance_gpu as tg
    fx = np.load(os.path.join(tg.GOLDEN, "traj_clearance_cases.npz"))

    def call(tag, co, T, pts, counts, nb, n, ld):
        outs = (torch.full((n, ld), -7.0, device="cuda", dtype=torch.float64), torch.full((n, ld), -7, device="cuda", dtype=torch.int32),
                torch.full((n, ld), -7.0, device="cuda", dtype=torch.float64))
        aa.traj_clearance_dev(bm(co, nb, ld), bm(T, nb, ld), torch.as_tensor(np.ascontiguousarray(pts), device="cuda"), co.shape[-1] // 2, n, nb,
                              counts=None if counts is None else torch.as_tensor(counts, device="cuda"), clearance=outs[0],
                              point=outs[1], t=outs[2], ctx=ctx)
        torch.cuda.synchronize()
        emit(tag, ("clearance", "point", "t"), outs, nb)

    for i in range(len(fx["T"])):                                      # every golden case alone against its own set
        cm, T, pts = tg.case(fx, i)
        call(f"clearance golden case={i} s={int(fx['s'][i])} points={len(pts)}", cm[None, None], np.array([[T]]),
             np.asarray(pts, dtype=np.float64).reshape(-1, 3), None, 1, 1, 1)
    rng = np.random.default_rng(91)
    for s in (2, 3, 4):
        co, T, _ = batch(s)
        cloud = rng.uniform([-6.0, -6.0, 0.0], [6.0, 6.0, 4.0], (130, 3))
        cloud[40, 1] = np.nan
        call(f"clearance batch shared s={s}", co, T, cloud, None, B, N, LD)
        sets = rng.uniform([-6.0, -6.0, 0.0], [6.0, 6.0, 4.0], (N, 80, 3))
        call(f"clearance batch per-piece s={s}", co, T, sets, np.array([80, 0, 37], dtype=np.int32), B, N, LD)


def step_separation(ctx):
    import torch
    import allocnet_amd as aa
    from tests import traj_separation_mp as sp
    from tests.util import GOLDEN
    fx = np.load(os.path.join(GOLDEN, "traj_separation_cases.npz"))
    names = ("sep", "t", "piece_a", "piece_b")

    def call(tag, co, T, t0, pairs, cutoff, ld):
        nb, n = T.shape
        d_pa, d_pb = (torch.as_tensor(np.ascontiguousarray(pairs[:, k], dtype=np.int32), device="cuda") for k in (0, 1))
        outs = aa.traj_separation_dev(bm(co, nb, ld), bm(T, nb, ld), d_pa, d_pb, co.shape[-1] // 2, n, nb,
                                      t0=None if t0 is None else torch.as_tensor(np.asarray(t0, dtype=np.float64), device="cuda"),
                                      cutoff=cutoff, ctx=ctx)
        torch.cuda.synchronize()
        emit(tag, names, outs)

    for i in range(len(fx["d"])):                                      # every golden case: its batch, its one pair
        co, T, t0, pair = sp.fixture_case(fx, i)
        call(f"separation golden case={i} s={co.shape[-1] // 2}", np.asarray(co), np.asarray(T), t0, np.array([pair]), np.inf, len(T) + 3)
    a, b = np.triu_indices(24)                                         # a <= b, sorted by a
    pairs = np.stack([a, b], axis=1)
    for s in (2, 3, 4):
        co, T, _ = batch(s)
        t0 = 0.35 * (np.arange(B) % 7)
        for cutoff in (np.inf, 1.0):
            call(f"separation batch s={s} cutoff={cutoff}", co, T, t0, pairs, cutoff, LD)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None, help="one of %s" % STEPS)
    args = ap.parse_args()
    if args.step:
        import allocnet_amd as aa
        {"margin": step_margin, "hit": step_hit, "clearance": step_clearance, "separation": step_separation}[args.step](aa.default_context(0))
        return 0
    for step in STEPS:
        res = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--step", step])
        if res.returncode != 0:            # nothing more is started on the device after a step that hung or failed
            print(f"step {step}: exit status {res.returncode}" + (" (time limit)" if res.returncode in (124, 137) else ""), flush=True)
            return res.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
