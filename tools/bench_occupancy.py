"""One depth scan into the occupancy grid on the MI355X: a 640 x 480 depth image into the launch-file map (400 x 400 x 50 voxels of
0.1 m), max_range 10 m.  The image is what a camera in the synthetic forest sees: VoxelMap.raycast on the truth map along the pixel
rays; a pixel without a return within 15 m reads 15 m, which the scan truncates at max_range and only carves.

Timed separately, device events around each call after warm-up, medians of --reps (>= 20):
    unproject        anet_depth_to_points_dev, 307 200 pixels
    integrate_plain  anet_occupancy_integrate_dev, the marks as two launches of plain byte stores (the default), update included
    integrate_atomic the same call with ANET_OCC_MARKS_ATOMIC set: one launch of atomicOr on flag bits, update included
                     (the two forms alternate inside one loop, on the same map)
    update_sweep     the same call with ONE zero-length ray: the mark launches are one workgroup each, the update sweeps the same
                     sub-box of the sensor -- the cost of the update launch when next to nothing is marked
    marks_*          integrate_* minus update_sweep: DERIVED, not measured on its own (kernel times: rocprofv3 --kernel-trace)
    to_voxels        anet_occupancy_to_voxels_dev over the whole grid
Before timing, the first scan's grid is compared with the numpy restatement (tests/occupancy_np.py) at full size, in both forms.
Host baseline: that restatement, one scan of the 1/16 subsample (every 4th pixel each way) on one host core -- labelled as such and
NOT scaled up; vectorised numpy, not a tuned CPU implementation.  Prints one JSON line.

    python tools/bench_occupancy.py [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, ORIGIN, SCALE = (400, 400, 50), (-20.0, -20.0, 0.0), 0.1
W, H = 640, 480
K = (525.0, 525.0, 319.5, 239.5)
MAX_RANGE = 10.0
FAR = 15.0


def camera():
    """At the third vertex of the forest's route, looking along +x with a yaw of 0.4 rad: (R camera-to-world, t)."""
    from allocnet_amd.synth import forest_route
    c, s = np.cos(0.4), np.sin(0.4)
    return np.array([[s, 0.0, c], [-c, 0.0, s], [0.0, -1.0, 0.0]]), forest_route()[2].copy()


def depth_image(truth, R, t):
    """float32 (H, W) z-depths of the truth map along the pixel rays; FAR along the ray where nothing is hit within it."""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones_like(u)], axis=-1).reshape(-1, 3)
    zc = 1.0 / np.linalg.norm(d, axis=1)                      # camera-frame z of the unit ray
    dw = (d * zc[:, None]) @ R.T
    voxel, tt = truth.raycast(np.broadcast_to(t, dw.shape), t + FAR * dw)
    rng = np.where(voxel >= 0, tt * FAR + 1e-6, FAR)
    return (rng * zc).reshape(H, W).astype(np.float32), int((voxel >= 0).sum())


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
    return ts


def stat(ts):
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    import allocnet_amd as aa
    from allocnet_amd.synth import forest_cloud, forest_route
    from tests import occupancy_np as onp
    assert "ANET_OCC_MARKS_ATOMIC" not in os.environ
    truth = aa.VoxelMap(SIZE, ORIGIN, SCALE)
    truth.setOccupiedCloud(forest_cloud(np.random.default_rng(17), n_points=1_000_000, clear_route=forest_route()).tobytes(), 16)
    R, t = camera()
    depth, returns = depth_image(truth, R, t)
    prm = aa.occupancy_params(max_range=MAX_RANGE)
    ref_prm = onp.Params(prm.hit, prm.miss, prm.lo, prm.hi, prm.min_range, prm.max_range)
    om = aa.OccupancyMap(SIZE, ORIGIN, SCALE, prm)
    dev = torch.from_numpy(depth).to(om.device)
    pts = aa.depth_to_points_dev(dev, K, (R, t))
    out = dict(map=list(SIZE), scale=SCALE, image=[W, H], max_range=MAX_RANGE, pixels_with_a_return=returns, reps=args.reps)

    # ---- the same bits at this size, in both forms
    want = onp.integrate(np.full(int(np.prod(SIZE)), onp.UNKNOWN, dtype=np.int16), SIZE, ORIGIN, SCALE, ref_prm, t, pts.cpu().numpy())
    om.integrate(pts, t)
    out["plain_equals_restatement"] = bool(np.array_equal(om.getLogOdds(), want))
    om.reset()
    os.environ["ANET_OCC_MARKS_ATOMIC"] = "1"
    om.integrate(pts, t)
    del os.environ["ANET_OCC_MARKS_ATOMIC"]
    out["atomic_equals_restatement"] = bool(np.array_equal(om.getLogOdds(), want))
    out["voxels_marked_per_scan"] = int((want != onp.UNKNOWN).sum())
    out["voxels_hit_per_scan"] = int((want > 0).sum())

    # ---- timings
    out["unproject"] = stat(events_ms(lambda: aa.depth_to_points_dev(dev, K, (R, t)), args.reps))

    def atomic():
        os.environ["ANET_OCC_MARKS_ATOMIC"] = "1"
        try:
            om.integrate(pts, t)
        finally:
            del os.environ["ANET_OCC_MARKS_ATOMIC"]
    for _ in range(5):
        om.integrate(pts, t); atomic()
    torch.cuda.synchronize()
    tp, ta = [], []
    for _ in range(args.reps):                                  # alternating, on the same map
        tp += events_ms(lambda: om.integrate(pts, t), 1, warm=0)
        ta += events_ms(atomic, 1, warm=0)
    out["integrate_plain"] = stat(tp)
    out["integrate_atomic"] = stat(ta)
    one = torch.from_numpy(t[None, :].copy()).to(om.device)
    out["update_sweep"] = stat(events_ms(lambda: om.integrate(one, t), args.reps))
    for k in ("plain", "atomic"):
        out["marks_%s_derived_ms" % k] = out["integrate_%s" % k]["median_ms"] - out["update_sweep"]["median_ms"]
    vm = aa.VoxelMap(SIZE, ORIGIN, SCALE)
    out["to_voxels"] = stat(events_ms(lambda: om.to_voxel_map(out=vm), args.reps))

    # ---- host: the restatement on the 1/16 subsample, one core, not scaled up
    sub = onp.depth_to_points(depth, K, R, t, step=4)
    L = np.full(int(np.prod(SIZE)), onp.UNKNOWN, dtype=np.int16)
    t0 = time.perf_counter()
    onp.integrate(L, SIZE, ORIGIN, SCALE, ref_prm, t, sub)
    out["host_numpy_restatement_sixteenth_subsample"] = dict(rays=len(sub), seconds_one_core=time.perf_counter() - t0,
                                                             note="1/16 of the rays, vectorised numpy, NOT scaled up")
    print(json.dumps(out))
    return 0 if out["plain_equals_restatement"] and out["atomic_equals_restatement"] else 1


if __name__ == "__main__":
    sys.exit(main())
