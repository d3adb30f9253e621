"""Device voxel map on the launch-file map (400 x 400 x 50 voxels of 0.1 m, a forest cloud of ~1e6 points): fill,
dilate(1/2/5), surface count + compaction, the box gather of a five-segment route, and convex_cover with the map against
convex_cover with getSurf() points; plus a host baseline: the same fill, frontier rounds and surface in vectorised numpy,
the rounds split into z-slabs over a thread pool (numpy releases the GIL in its array loops), timed with 1 and 16
threads and checked against the device's voxels.  Warm-ups, then medians over --reps; the first call of each stage in a
fresh process is reported too (the 8 MB grid stays in the Infinity Cache between repeated calls).  Prints one JSON line.
    python tools/bench_voxel_map.py [--points 1000000] [--reps 20]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_map(rec, size, origin, scale, r, pool, threads):
    """voxel_map::VoxelMap's fill, dilate(r) and getSurf in numpy: the dilation rounds run over z-slabs in `pool`, each
    slab reading the previous front with a one-plane halo and writing only its own planes.  Returns (voxels, points)."""
    sx, sy, sz = size
    o = np.asarray(origin, dtype=np.float64)
    p = rec[:, :3].astype(np.float64)
    p = p[np.isfinite(p).all(axis=1)]
    t = np.trunc((p - o) / scale)
    keep = ((t >= 0) & (t < np.asarray(size))).all(axis=1)
    t = t[keep].astype(np.int64)
    vox = np.zeros(sx * sy * sz, dtype=np.uint8)
    vox[t[:, 0] + sx * (t[:, 1] + sy * t[:, 2])] = 1
    v = vox.reshape(sz, sy, sx)
    front = v == 1
    bounds = np.linspace(0, sz, min(threads, sz) + 1).astype(int)

    def slab(front, new, z0, z1):
        lo, hi = max(z0 - 1, 0), min(z1 + 1, sz)
        f = np.zeros((hi - lo + 2, sy + 2, sx + 2), dtype=bool)      # zero-padded: out-of-map neighbours are no sources
        f[1:-1, 1:-1, 1:-1] = front[lo:hi]
        nb = np.zeros((z1 - z0, sy, sx), dtype=bool)
        k = z0 - lo + 1
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dz or dy or dx:
                        nb |= f[k + dz:k + dz + z1 - z0, 1 + dy:1 + dy + sy, 1 + dx:1 + dx + sx]
        nf = nb & (v[z0:z1] == 0)
        v[z0:z1][nf] = 2
        new[z0:z1] = nf
    for _ in range(r):
        new = np.empty_like(front)
        list(pool.map(lambda zz: slab(front, new, *zz), zip(bounds[:-1], bounds[1:])))
        front = new
    ids = np.flatnonzero(front.reshape(-1))
    step = np.array([1, sx, sx * sy], dtype=np.int64)
    xyz = np.stack([ids % sx, (ids % (sx * sy)) // sx, ids // (sx * sy)], axis=1)
    pts = (xyz * step).astype(np.float64) * ((1.0 / step.astype(np.float64)) * scale) + (o + 0.5 * scale)
    return vox, pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import allocnet_amd as aa
    from allocnet_amd.synth import forest_cloud, forest_route
    size, origin, scale = (400, 400, 50), (-20.0, -20.0, 0.0), 0.1
    route = forest_route()
    rec = forest_cloud(np.random.default_rng(0), n_points=args.points, clear_route=route)
    buf = rec.tobytes()
    ctx = aa.default_context()
    dev = torch.device("cuda", ctx.device)
    cloud_dev = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).to(dev)
    sync = torch.cuda.synchronize

    def timed(fn):
        sync(); t = time.perf_counter(); fn(); sync()
        return (time.perf_counter() - t) * 1e3

    def stage(fn, reps=args.reps):
        first = timed(fn)
        for _ in range(2):
            fn()
        ts = [timed(fn) for _ in range(reps)]
        return dict(first_ms=first, median_ms=float(np.median(ts)), min_ms=float(np.min(ts)))

    out = dict(map=list(size), scale=scale, cloud_points=args.points)
    vm = aa.VoxelMap(size, origin, scale, ctx=ctx)
    out["fill"] = stage(lambda: vm.setOccupiedCloud(cloud_dev, 16))

    def fresh_dilate(r):
        def go():
            vm.voxels_dev.copy_(base)
            vm.dilate(r)
        return go
    vm.setOccupiedCloud(cloud_dev, 16)
    sync()
    base = vm.voxels_dev.clone()
    copy_ms = stage(lambda: vm.voxels_dev.copy_(base))["median_ms"]
    out["grid_copy_ms"] = copy_ms
    for r in (1, 2, 5):
        s = stage(fresh_dilate(r))
        s["note"] = "includes the 8 MB reset copy (grid_copy_ms), the surface compaction and one count read-back"
        out[f"dilate{r}"] = s
    vm.voxels_dev.copy_(base)
    vm.dilate(2)
    out["surface_points"] = int(vm.surf_ids_dev.numel())

    def pipeline():
        m = aa.VoxelMap(size, origin, scale, ctx=ctx)
        m.setOccupiedCloud(cloud_dev, 16)
        m.dilate(2)
        m.surf_points_dev()
    out["fill_dilate2_surface"] = stage(pipeline, reps=max(5, args.reps // 2))

    # surface compaction alone (count + scan + write of the last front)
    work = vm._work; ids = torch.empty(out["surface_points"] + 1, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    import ctypes
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    out["surface_compaction"] = stage(lambda: ctx.check(ctx.lib.anet_voxel_surface_dev(
        ctx.handle, ctypes.byref(vm._grid), vp(work), ids.numel(), vp(ids), vp(cnt), st)))

    # box gather for the route's five segments (the boxes convex_cover builds)
    lo, hi = vm.getOrigin(), vm.getCorner()
    bd = np.zeros((len(route) - 1, 6, 4))
    for k in range(len(route) - 1):
        a, b = route[k], route[k + 1]
        h = np.minimum(np.maximum(a, b) + 3.0, hi); low = np.maximum(np.minimum(a, b) - 3.0, lo)
        for ax in range(3):
            bd[k, 2 * ax, ax] = 1.0; bd[k, 2 * ax, 3] = -h[ax]
            bd[k, 2 * ax + 1, ax] = -1.0; bd[k, 2 * ax + 1, 3] = low[ax]
    g = stage(lambda: vm.gather_boxes(bd))
    out["box_gather"] = g
    _, counts = vm.gather_boxes(bd)
    out["box_points"] = [int(c) for c in counts]
    surf = vm.getSurf()

    def host_select():
        return [surf[(surf @ bd[k, :, :3].T + bd[k, :, 3]).max(axis=1) < 0.0] for k in range(len(bd))]
    out["box_select_host_numpy"] = stage(host_select, reps=5)
    out["convex_cover_map"] = stage(lambda: aa.convex_cover(route, vm, lo, hi, 100.0, 3.0, ctx=ctx), reps=5)
    out["convex_cover_points"] = stage(lambda: aa.convex_cover(route, vm.getSurf(), lo, hi, 100.0, 3.0, ctx=ctx), reps=5)

    # host baseline: fill + dilate(2) + surface points with numpy, 1 and 16 threads; its voxels must equal the device's
    vm.voxels_dev.copy_(base)
    vm.dilate(2)
    dev_vox = vm.getVoxels()
    for threads in (1, 16):
        pool = ThreadPoolExecutor(threads)
        vox = None

        def go():
            nonlocal vox
            vox, _ = host_map(rec, size, origin, scale, 2, pool, threads)
        ht = [timed(go) for _ in range(args.host_reps)]
        pool.shutdown()
        out[f"host_numpy_fill_dilate2_surface_ms_{threads}t"] = float(np.median(ht))
        out[f"host_matches_device_{threads}t"] = bool(np.array_equal(vox, dev_vox))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
