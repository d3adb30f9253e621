"""Exploration goals on the MI355X, on the launch-file map (400 x 400 x 50 voxels of 0.1 m) after twelve scans of the synthetic forest
from poses along forest_route() (the fan and the sensor of examples/map_from_scans.py, max_range 10 m).

Timed with device events around each call after warm-up, medians of --reps (>= 20), each beside what a user of the parent commit
would do on the same data:
    frontier        anet_occupancy_frontier_dev over the whole map     | the same mask from shifted comparisons in eager torch
    label_6 / _26   anet_voxel_label_components_dev of that mask, with the rounds taken (wall clock: the call returns when the
                    labels are final)                                  | scipy.ndimage.label on the host (one core, copy excluded)
    stats           anet_voxel_component_stats_dev                     | numpy bincount / minimum.at / maximum.at on the host labels
    view_gain_1     64 views x (80 x 60) template points in one chunk  | per view: voxel_raycast_dev for the end points, a clone of
    view_gain_8     the same in chunks of 8 views                      |   the log-odds grid, integrate, the difference of known counts
The parent-commit view gain is an approximation (the ray query stops at the first blocked BYTE of the hand-over, the scan then
marks that end cell): its distance from the exact count is printed.  The device results are compared with each other (one chunk
against chunks of 8) before timing.  --profile-run: the device calls alone, three times each, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/bench_frontier.py --profile-run).  Prints one JSON line.

    python tools/bench_frontier.py [--reps 20]
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
MAX_RANGE = 10.0
FAN = (128, 96)
N_VIEWS = 64
TEMPLATE = dict(K=(60.0, 60.0, 39.5, 29.5), width=80, height=60, step=1, depth=15.0)


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
    return float(np.median(ts))


def wall_ms(fn, reps, warm=1):
    import torch
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def scanned_map(aa, torch):
    from allocnet_amd.synth import forest_cloud, forest_route
    route = forest_route()
    truth = aa.VoxelMap(SIZE, ORIGIN, SCALE)
    truth.setOccupiedCloud(forest_cloud(np.random.default_rng(17), n_points=1_000_000, clear_route=route).tobytes(), 16)
    om = aa.OccupancyMap(SIZE, ORIGIN, SCALE, aa.occupancy_params(max_range=MAX_RANGE))
    az = (np.arange(FAN[0]) + 0.5) * (2.0 * np.pi / FAN[0])
    el = -0.5 * np.pi + (np.arange(FAN[1]) + 0.5) * (np.pi / FAN[1])
    a, e = np.meshgrid(az, el, indexing="ij")
    dirs = torch.from_numpy(np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=-1).reshape(-1, 3)).to(om.device)
    seg = np.linalg.norm(np.diff(route, axis=0), axis=1)
    s = np.concatenate([[0.0], np.cumsum(seg)])
    reach = 1.5 * MAX_RANGE
    for at in np.linspace(0.0, s[-1], 12):
        pose = np.array([np.interp(at, s, route[:, c]) for c in range(3)])
        o = torch.from_numpy(pose).to(om.device).expand(dirs.shape[0], 3).contiguous()
        q = o + reach * dirs
        voxel, t = aa.voxel_raycast_dev(truth, truth.voxels_dev, o, q)
        t = torch.where(voxel >= 0, t + 1e-6 * SCALE / reach, torch.ones_like(t))
        om.integrate(o + t[:, None] * (q - o), pose)
    return om


def torch_frontier(torch, L, occ):
    G = L.reshape(SIZE[2], SIZE[1], SIZE[0])
    unk = G == -32768
    near = torch.zeros_like(unk)
    near[:, :, 1:] |= unk[:, :, :-1]; near[:, :, :-1] |= unk[:, :, 1:]
    near[:, 1:, :] |= unk[:, :-1, :]; near[:, :-1, :] |= unk[:, 1:, :]
    near[1:, :, :] |= unk[:-1, :, :]; near[:-1, :, :] |= unk[1:, :, :]
    return (~unk & (G < occ) & near).reshape(-1).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile-run", action="store_true")
    args = ap.parse_args()
    if args.reps < 20 and not args.profile_run:
        ap.error("--reps must be at least 20")
    import torch
    import allocnet_amd as aa
    from allocnet_amd import frontier as fr
    om = scanned_map(aa, torch)
    dev, L, prm = om.device, om.logodds_dev(), om.params
    out = dict(map=list(SIZE), scale=SCALE, max_range=MAX_RANGE, known_fraction=om.known_fraction(), reps=args.reps,
               note="one run on one machine; device-event medians unless marked wall")

    mask, count = om.frontier()
    assert torch.equal(mask, torch_frontier(torch, L, 0)) and count == int(mask.sum().item())
    work = fr._components_work(om._grid, om.ctx, dev)
    labels = {c: fr.label_components_dev(om, mask, c, work=work, with_rounds=True) for c in (6, 26)}
    lab26 = labels[26][0]
    n_comp, root, cnt, sums, bbox = fr.component_stats_dev(om, lab26, 1 << 16, work=work)
    out.update(frontier_voxels=count, rounds_6=labels[6][1], rounds_26=labels[26][1], components_26=n_comp)

    # 64 poses in known free space, looking along a yaw that turns with the index
    rng = np.random.default_rng(4)
    free = torch.nonzero((L != -32768) & (L < 0)).reshape(-1).cpu().numpy()
    ids = free[rng.choice(len(free), N_VIEWS, replace=False)]
    t = np.asarray(ORIGIN) + (np.stack([ids % SIZE[0], (ids // SIZE[0]) % SIZE[1], ids // (SIZE[0] * SIZE[1])], axis=1) + 0.5) * SCALE
    yaw = np.arange(N_VIEWS) * (2.0 * np.pi / N_VIEWS)
    R = fr.look_at(t, t + np.stack([np.cos(yaw), np.sin(yaw), np.zeros(N_VIEWS)], axis=1))
    Rd, td = torch.from_numpy(np.ascontiguousarray(R)).to(dev), torch.from_numpy(t).to(dev)
    pts = aa.frustum_points(device=dev, ctx=om.ctx, **TEMPLATE)
    one = fr.view_gain_workspace(om, prm)
    work_all = torch.zeros(N_VIEWS * one, dtype=torch.uint8, device=dev)
    work_8 = torch.zeros(8 * one, dtype=torch.uint8, device=dev)
    gain = aa.view_gain_dev(om, prm, L, Rd, td, pts, 0, work=work_all)
    assert torch.equal(gain, aa.view_gain_dev(om, prm, L, Rd, td, pts, 0, work=work_8)) and not work_all.any().item()
    out.update(views=N_VIEWS, template_points=int(pts.shape[0]), slot_bytes=one, gain_mean=float(gain.double().mean().item()))

    calls = dict(frontier=lambda: om.frontier(out=mask),
                 label_6=lambda: fr.label_components_dev(om, mask, 6, out=labels[6][0], work=work),
                 label_26=lambda: fr.label_components_dev(om, mask, 26, out=lab26, work=work),
                 stats=lambda: fr.component_stats_dev(om, lab26, 1 << 16, work=work),
                 view_gain_1=lambda: aa.view_gain_dev(om, prm, L, Rd, td, pts, 0, work=work_all),
                 view_gain_8=lambda: aa.view_gain_dev(om, prm, L, Rd, td, pts, 0, work=work_8))
    if args.profile_run:
        for fn in calls.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        print(json.dumps(dict(profile_run=True)))
        return 0
    dev_ms = {k: (wall_ms if k.startswith("label") or k == "stats" else events_ms)(fn, args.reps) for k, fn in calls.items()}
    out["device_ms"] = dev_ms
    out["device_ms_clock"] = dict(label_6="wall", label_26="wall", stats="wall (the count is read back)")

    # ---- what the parent commit offers on the same data
    base = dict(frontier_torch_eager=events_ms(lambda: torch_frontier(torch, L, 0), args.reps))
    from scipy import ndimage
    m3 = mask.cpu().numpy().reshape(SIZE[2], SIZE[1], SIZE[0])
    for c, rank in ((6, 1), (26, 3)):
        st = ndimage.generate_binary_structure(3, rank)
        t0 = time.perf_counter(); ref, k = ndimage.label(m3, structure=st); base[f"label_{c}_scipy_host"] = 1e3 * (time.perf_counter() - t0)
        got = labels[c][0].cpu().numpy()
        assert k == len(np.unique(got[got >= 0]))
    hl = lab26.cpu().numpy()
    t0 = time.perf_counter()
    v = np.flatnonzero(hl >= 0)
    r_, inv = np.unique(hl[v], return_inverse=True)
    xyz = np.stack([v % SIZE[0], (v // SIZE[0]) % SIZE[1], v // (SIZE[0] * SIZE[1])], axis=1)
    c_ = np.bincount(inv); s_ = np.zeros((len(r_), 3), dtype=np.int64); np.add.at(s_, inv, xyz)
    base["stats_numpy_host"] = 1e3 * (time.perf_counter() - t0)
    assert np.array_equal(r_, root.cpu().numpy()) and np.array_equal(c_, cnt.cpu().numpy()) and np.array_equal(s_, sums.cpu().numpy())

    vm = om.to_voxel_map(occ=0, unknown="free")
    scratch = aa.OccupancyMap(SIZE, ORIGIN, SCALE, prm, ctx=om.ctx)
    known0 = int((L != -32768).sum().item())

    def parent_view_gain():
        res = []
        for k in range(N_VIEWS):
            o = td[k].expand(pts.shape[0], 3).contiguous()
            d = pts @ Rd[k].T
            q = o + d * (MAX_RANGE / d.norm(dim=1, keepdim=True))
            voxel, tt = aa.voxel_raycast_dev(vm, vm.voxels_dev, o, q)
            scratch.logodds_dev().copy_(L)
            scratch.integrate(o + torch.where(voxel >= 0, tt, torch.ones_like(tt))[:, None] * (q - o), t[k])
            res.append(int((scratch.logodds_dev() != -32768).sum().item()) - known0)
        return res
    approx = np.asarray(parent_view_gain())
    base["view_gain_parent_sequence_wall"] = wall_ms(parent_view_gain, 3, warm=0)
    exact = gain.cpu().numpy()
    out["baseline_ms"] = base
    out["parent_view_gain_error"] = dict(mean_abs=float(np.abs(approx - exact).mean()), max_abs=int(np.abs(approx - exact).max()),
                                         mean_exact=float(exact.mean()))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
