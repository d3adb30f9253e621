#!/usr/bin/env python3
"""Device path search (sfc_gen::planPath) on the launch-file map: 400 x 400 x 50 voxels of 0.1 m filled from a
forest_cloud of 10^6 records and dilate(2), planning forest_route()[0] -> [-1].  Medians of --reps wall times after a
warm-up, for the field (it synchronises), the extraction (target, walk, shortcut, cost and the copies back) and the whole
plan_paths call, at B = 1 and at B = 8 (one start, eight goals along the route), with the round count.  Host baseline:
scipy's csgraph.dijkstra on the same graph (26 neighbours, weights 10 / 14 / 17, no corner cutting), one thread, the
graph construction timed apart.

    python tools/bench_voxel_path.py [--reps 20] [--no-host]      # prints one JSON line
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_graph(vox, size, oc, scale, lb, hb):
    """the search graph as a CSR matrix over the 13 moves whose first non-zero of (dz, dy, dx) is positive"""
    from scipy.sparse import csr_matrix
    sx, sy, sz = size
    ins = [(np.arange(s) * scale + oc[c] >= lb[c]) & (np.arange(s) * scale + oc[c] <= hb[c]) for c, s in enumerate(size)]
    free = (vox.reshape(sz, sy, sx) == 0) & ins[2][:, None, None] & ins[1][None, :, None] & ins[0][None, None, :]
    fp = np.zeros((sz + 2, sy + 2, sx + 2), dtype=bool)
    fp[1:-1, 1:-1, 1:-1] = free
    ids = np.arange(sx * sy * sz, dtype=np.int32).reshape(sz, sy, sx)
    moves = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)][13:]
    src, dst, wt = [], [], []
    for dx, dy, dz in moves:
        ok = free.copy()
        for ex in {0, dx}:
            for ey in {0, dy}:
                for ez in {0, dz}:
                    ok &= fp[1 + ez:1 + ez + sz, 1 + ey:1 + ey + sy, 1 + ex:1 + ex + sx]
        s = ids[ok]
        src.append(s); dst.append(s + np.int32(dx + sx * (dy + sy * dz)))
        wt.append(np.full(len(s), float({1: 10, 2: 14, 3: 17}[abs(dx) + abs(dy) + abs(dz)])))
    n = sx * sy * sz
    return csr_matrix((np.concatenate(wt), (np.concatenate(src), np.concatenate(dst))), shape=(n, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch
    import allocnet_amd as aa
    from allocnet_amd.path_search import path_field_dev, extract_paths
    from allocnet_amd.synth import forest_cloud, forest_route
    route = forest_route()
    rec = forest_cloud(np.random.default_rng(17), n_points=1_000_000, clear_route=route)
    vm = aa.VoxelMap((400, 400, 50), (-20.0, -20.0, 0.0), 0.1)
    vm.setOccupiedCloud(rec.tobytes(), 16)
    vm.dilate(2)
    torch.cuda.synchronize()
    # eight goals: the route's far end and seven points along its legs (clear by construction)
    t = np.linspace(0.0, 1.0, 9)[1:-1]
    legs = np.cumsum(np.r_[0.0, np.linalg.norm(np.diff(route, axis=0), axis=1)])
    along = np.stack([np.interp(t * legs[-1], legs, route[:, c]) for c in range(3)], axis=1)
    goals8 = np.concatenate([route[-1:], along])
    out = {"map": [400, 400, 50], "scale": 0.1, "reps": args.reps}
    for B, goals in ((1, route[-1:]), (8, goals8)):
        starts = np.repeat(route[:1], B, axis=0)
        for _ in range(3):
            aa.plan_paths(starts, goals, vm)
        tf, te, tt, rounds = [], [], [], set()
        for _ in range(args.reps):
            t0 = time.perf_counter()
            _, r = path_field_dev(vm, starts)
            t1 = time.perf_counter()
            costs, paths, status = extract_paths(vm, starts, goals)
            t2 = time.perf_counter()
            tf.append(t1 - t0); te.append(t2 - t1); rounds.add(r)
        for _ in range(args.reps):
            t0 = time.perf_counter()
            aa.plan_paths(starts, goals, vm)
            tt.append(time.perf_counter() - t0)
        out[f"B{B}"] = {"field_ms": 1e3 * float(np.median(tf)), "extract_ms": 1e3 * float(np.median(te)),
                        "total_ms": 1e3 * float(np.median(tt)), "rounds": sorted(rounds),
                        "status": [int(s) for s in status], "cost": [float(c) for c in costs],
                        "points": [len(p) for p in paths]}
    if not args.no_host:
        from scipy.sparse.csgraph import dijkstra
        vox = vm.getVoxels()
        oc = vm.getOrigin() + 0.5 * 0.1
        t0 = time.perf_counter()
        G = host_graph(vox, (400, 400, 50), oc, 0.1, vm.getOrigin(), vm.getCorner())
        t1 = time.perf_counter()
        sv = int(vm.posD2I(route[0]) @ np.array([1, 400, 400 * 400]))
        d = dijkstra(G, directed=False, indices=sv)
        t2 = time.perf_counter()
        f, _ = path_field_dev(vm, route[:1])
        dev = f.cpu().numpy()[0]
        host = np.where(np.isinf(d), 0xFFFFFFFF, d).astype(np.uint32)
        out["host"] = {"graph_ms": 1e3 * (t1 - t0), "dijkstra_ms": 1e3 * (t2 - t1), "edges": int(G.nnz),
                       "field_equal": bool(np.array_equal(dev, host))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
