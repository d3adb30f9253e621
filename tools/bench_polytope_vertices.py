"""Vertex enumeration of polytopes on the MI355X (anet_polytope_vertices_dev): one plan's worth -- 21 polytopes of up to 32 rows, as
corridor_vertices sends an 11-polytope corridor -- and the two large batches, 131 072 polytopes of 16 rows and 8 192 of 64, each
with one wave per polytope and with the workgroup's four waves per polytope (ANET_POLYTOPE_VERTICES_WPP), the two numbers behind
the dispatch threshold of csrc/tuning.h.

Every step runs in a child process of its own under its own time limit; the driver stops at the first step that fails.  Times are
device events around one _dev call (the depth kernels in front included) after warm-up, medians of --reps (>= 20).  Counted work:
triples x (a 3x3 solve of about 50 operations + 7 per row of the feasibility sweep) -- an upper bound, the sweep leaves a chunk of
64 triples as soon as none of them is feasible.  The step `qhull_host` times scipy.spatial.HalfspaceIntersection on ONE host core
on a sample of the same inputs, interior points given: a different algorithm, not the reference.  Prints one JSON line.

    python tools/bench_polytope_vertices.py [--reps 30] [--step NAME]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ["plan_21", "batch_131072x16", "batch_8192x64"]
STEPS = [f"{w}_wpp{k}" for w in WORKLOADS for k in (1, 4)] + ["qhull_host"]
LIMIT_S = 300


def workload(name):
    """(B, H, 4) raw-form polytopes, zero-padded."""
    from allocnet_amd.synth import corridor_problem, qp_corridor_problem
    if name == "plan_21":
        hp = qp_corridor_problem(np.random.default_rng(4), 11, 16)[2]
        hp[:, :, 3] *= -1.0
        out = np.zeros((21, 32, 4))
        for i in range(11):
            out[2 * i, :16] = hp[i]
            if i:
                out[2 * i - 1] = np.concatenate([hp[i - 1], hp[i]])
        return out
    if name == "batch_131072x16":
        hp = corridor_problem(np.random.default_rng(11), 32768, 4, 3, 16)[4].reshape(131072, 16, 4).copy()
        hp[:, :, 3] *= -1.0
        return hp
    # 64 tangent planes of a sphere of radius 1 to 3 about a point of the map
    rng = np.random.default_rng(6)
    n = rng.normal(size=(8192, 64, 3))
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    c = rng.uniform(-20.0, 20.0, size=(8192, 1, 3))
    r = rng.uniform(1.0, 3.0, size=(8192, 1))
    return np.concatenate([n, (-(n * c).sum(2) - r)[..., None]], axis=2)


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


def device_step(step, reps):
    import ctypes
    import torch
    import allocnet_amd as aa
    name, wpp = step.rsplit("_wpp", 1)
    os.environ["ANET_POLYTOPE_VERTICES_WPP"] = wpp
    hp_host = workload(name)
    B, H, _ = hp_host.shape
    hp = torch.from_numpy(hp_host).cuda()
    mv = 2 * H - 4
    ctx = aa.default_context(0)
    verts = torch.zeros(B, mv, 3, device="cuda", dtype=torch.float64)
    count = torch.zeros(B, device="cuda", dtype=torch.int32)
    status = torch.zeros(B, device="cuda", dtype=torch.int32)
    active = torch.zeros(B, mv, 2, device="cuda", dtype=torch.int64)
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = lambda: ctx.check(ctx.lib.anet_polytope_vertices_dev(ctx.handle, B, H, q(hp), 1e-6, mv, q(verts), q(count), q(active),
                                                              q(status), st))
    med, mn = events_ms(fn, reps)
    rows = (np.abs(hp_host[:, :, :3]).sum(2) != 0.0).sum(1).astype(np.int64)
    triples = rows * (rows - 1) * (rows - 2) // 6
    work = float((triples * (50 + 7 * rows)).sum())
    cnt = count.cpu().numpy()
    return dict(polytopes=B, max_rows=H, waves_per_polytope=int(wpp), median_ms=med, min_ms=mn, us_per_polytope=med * 1e3 / B,
                triples=int(triples.sum()), counted_operations_upper_bound=work, counted_TFLOPs_upper_bound=work / (med * 1e-3) / 1e12,
                vertices_mean=float(cnt.mean()), statuses={int(k): int(v) for k, v in zip(*np.unique(status.cpu().numpy(), return_counts=True))})


def qhull_host(reps):
    """scipy's HalfspaceIntersection (Qhull) on one host core, interior points from the device: a different algorithm."""
    import allocnet_amd as aa
    from scipy.spatial import HalfspaceIntersection
    out = {}
    for name in WORKLOADS:
        hp = workload(name)[:256]
        _, x = aa.polytope_depth(hp)
        t0 = time.perf_counter()
        for h, p in zip(hp, x):
            h = h[np.any(h[:, :3] != 0.0, axis=1)]
            HalfspaceIntersection(h, p).intersections
        out[name] = dict(sample=len(hp), us_per_polytope_one_core=(time.perf_counter() - t0) * 1e6 / len(hp),
                         note="Qhull on the polar dual, interior point given; not the reference, another algorithm")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", default=None, help="one of %s" % STEPS)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.step:
        print(json.dumps(qhull_host(args.reps) if args.step == "qhull_host" else device_step(args.step, args.reps)))
        return 0
    out = {}
    for step in STEPS:
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)],
                                 capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            out[step] = dict(error=f"no result within {LIMIT_S} s")
            break                                       # nothing more is started on the device after a step that hung
        if res.returncode != 0:
            out[step] = dict(error=f"exit status {res.returncode}", stderr=res.stderr[-800:])
            break                                       # ... or failed
        out[step] = json.loads(res.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return 0 if all("error" not in v for v in out.values()) and len(out) == len(STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())
