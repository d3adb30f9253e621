"""The time-allocation network on the MI355X: batched inference at B = 1, 64, 4096 and 131 072 (L = 5, the recorded model's
weights and its 256 fixture corridors, repeated), both kernel forms where the batch allows, next to torch running the same layers
(torch.nn.Conv1d / Conv2d / Linear / LSTMCell built from the same weights inside this script) on the same device; and
LearningPlanner.call_model_batch at 4096 split into the network and the QP.

Every step runs in a child process of its own under its own time limit; the driver stops at the first step that fails.  Network
times are device events around one call on device tensors after warm-up, medians of --reps (>= 20).  FLOP/s are the COUNTED
operations per problem (below) over that time, as a share of the 155 TFLOP/s measured peak of the f32 matrix instruction.
Prints one JSON line.

    python tools/bench_timenet.py [--reps 30] [--step NAME]
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

F32_MATRIX_PEAK = 155e12      # FLOP/s, measured peak of v_mfma_f32_32x32x2_f32 on the MI355X
L = 5


def flops_per_problem(seq_len=L):
    """Counted multiply-adds x 2: the recurrent product seq_len x 1024 x 256, the input projection 1024 x 38 once, the live
    conv positions 16 (L / 4) x 16 x 450.  Encoders' linears, heads and nonlinearities are not counted."""
    return 2 * (seq_len * 1024 * 256 + 1024 * 38 + 16 * (seq_len // 4) * 16 * 450)


STEPS = ["net_1", "net_64", "net_4096", "net_131072", "call_model_batch_4096"]
LIMIT_S = {"net_131072": 600, "call_model_batch_4096": 900}


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


def fixtures():
    from tests import timenet_np as tnp
    g = os.path.join(ROOT, "tests", "golden")
    return tnp.load_golden_weights(os.path.join(g, "timenet_seq5")), np.load(os.path.join(g, "timenet_seq5_cases.npz"))


def torch_layers(w, dev):
    """The same layers in torch, from the same weights: returns f(state, hpolys) -> tf, stop (B, L)."""
    import torch
    from torch import nn
    t = lambda k: torch.from_numpy(np.ascontiguousarray(w[k])).to(dev)
    sm = nn.Sequential(nn.Conv1d(9, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool1d(2, 2), nn.Flatten(), nn.Linear(8, 6)).to(dev)
    hm = nn.Sequential(nn.Conv2d(50, 16, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(2, 2), nn.MaxPool2d(2, 2), nn.Flatten(),
                       nn.Linear(16, 32)).to(dev)
    cell = nn.LSTMCell(38, 256).to(dev)
    with torch.no_grad():
        sm[0].weight.copy_(t("state_input_module.0.weight")); sm[0].bias.copy_(t("state_input_module.0.bias"))
        sm[4].weight.copy_(t("state_input_module.4.weight")); sm[4].bias.copy_(t("state_input_module.4.bias"))
        hm[0].weight.copy_(t("hpoly_input_module.0.weight")); hm[0].bias.copy_(t("hpoly_input_module.0.bias"))
        hm[5].weight.copy_(t("hpoly_input_module.5.weight")); hm[5].bias.copy_(t("hpoly_input_module.5.bias"))
        cell.weight_ih.copy_(t("output_module.weight_ih_l0")); cell.weight_hh.copy_(t("output_module.weight_hh_l0"))
        cell.bias_ih.copy_(t("output_module.bias_ih_l0")); cell.bias_hh.copy_(t("output_module.bias_hh_l0"))
    wt, bt = t("tfs_output_layer.weight"), t("tfs_output_layer.bias")
    ws, bs = t("stop_token_output_layer.0.weight"), t("stop_token_output_layer.0.bias")

    def f(state, hpolys):
        with torch.no_grad():
            x = torch.cat([sm(state), hm(hpolys)], dim=1)
            h = torch.zeros(x.shape[0], 256, device=dev); c = torch.zeros_like(h)
            tf, stop = [], []
            for _ in range(L):
                h, c = cell(x, (h, c))
                tf.append(h @ wt.T + bt); stop.append(torch.sigmoid(h @ ws.T + bs))
            return torch.cat(tf, 1), torch.cat(stop, 1)
    return f


def net_step(B, reps):
    import torch
    import allocnet_amd as aa
    from allocnet_amd.time_net import SINGLE_MAX
    w, d = fixtures()
    dev = torch.device("cuda:0")
    idx = np.arange(B) % 256
    state = torch.from_numpy(d["state"][idx]).to(dev); hp = torch.from_numpy(d["hpolys"][idx]).to(dev)
    net = aa.TimeAllocNet.from_state_dict(w)
    out = dict(batch=B, seq_len=L, counted_flops_per_problem=flops_per_problem(), default_form="single" if B <= SINGLE_MAX else "tile")
    forms = [None] + (["single"] if B <= 4096 else []) + ["tile"]
    for form in forms:
        res = net.forward_dev(state, hp, steps=True, form=form)
        med, mn = events_ms(lambda: net.forward_dev(state, hp, steps=True, form=form, out=res), reps)
        fl = flops_per_problem() * B / (med * 1e-3)
        out[form or "default"] = dict(median_ms=med, min_ms=mn, us_per_problem=med * 1e3 / B, counted_TFLOPs=fl / 1e12,
                                      share_of_f32_matrix_peak=fl / F32_MATRIX_PEAK)
    f = torch_layers(w, dev)
    tf, stop = f(state, hp)
    torch.cuda.synchronize()
    ours = net.forward_dev(state, hp, steps=True)
    out["torch_same_layers_same_device"] = dict(zip(("median_ms", "min_ms"), events_ms(lambda: f(state, hp), reps)))
    out["torch_same_layers_same_device"]["largest_distance_to_ours"] = float(
        max((tf - ours[2]).abs().max(), (stop - ours[3]).abs().max()))
    out["torch_over_default"] = out["torch_same_layers_same_device"]["median_ms"] / out["default"]["median_ms"]
    return out


def batch_step(reps):
    """call_model_batch at 4096 (the fixture corridors, 16 times over): wall time of the call, and of its network and QP parts
    called the same way by hand (host entry points: transfers included)."""
    import torch
    import allocnet_amd as aa
    from allocnet_amd.learning_planner import group_by_seg, stack_group
    from allocnet_amd.qp import QP_METHOD_INTERIOR_POINT
    w, d = fixtures()
    B = 4096
    idx = np.arange(B) % 256
    planner = aa.LearningPlanner(aa.LearningPlannerConfig(ModelMaxSeg=5, OptOrder=4))
    planner.net = aa.TimeAllocNet.from_state_dict(w)
    ini = d["state"][idx, :, 0].astype(np.float64).reshape(B, 3, 3); fin = d["state"][idx, :, 1].astype(np.float64).reshape(B, 3, 3)
    corridors = []
    for i in idx:
        hp = d["hpolys"][i].astype(np.float64)
        corridors.append([hp[:, :, k][np.abs(hp[:, :, k]).sum(axis=1) > 0] for k in range(int(d["seg"][i]))])
    state, hps = d["state"][idx], d["hpolys"][idx]
    segs = [len(c) for c in corridors]

    def wall(fn, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ts)), r
    planner.call_model_batch(ini, fin, corridors)                                # warm-up
    total, (ok, _, times) = wall(lambda: planner.call_model_batch(ini, fin, corridors), reps)
    t_net, _ = wall(lambda: planner.net.forward(state, hps), reps)
    keep = [not (times[b, :segs[b]] < 1e-10).any() for b in range(B)]
    groups = {s: (g, stack_group(corridors, g, s)) for s, g in group_by_seg(segs, keep).items()}

    def qp():
        for s, (g, hp) in groups.items():
            aa.qp_solve(4, ini[g], fin[g], hp, times[g, :s].astype(np.float64), settings=aa.qp_settings(method=QP_METHOD_INTERIOR_POINT))
    t_qp, _ = wall(qp, reps)
    return dict(batch=B, reps=reps, wall_ms_call_model_batch=total, wall_ms_network_host_entry=t_net, wall_ms_qp_solve_groups=t_qp,
                wall_ms_host_packing_and_trajectories=total - t_net - t_qp, problems_passing_the_time_check=int(sum(keep)),
                problems_solved=int(ok.sum()), groups={int(s): len(g) for s, (g, _) in groups.items()})


def run_step(step, reps):
    if step.startswith("net_"):
        return net_step(int(step.split("_")[1]), reps)
    return batch_step(reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", default=None, help="one of %s" % STEPS)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.step:
        print(json.dumps(run_step(args.step, args.reps)))
        return 0
    out = {}
    for step in STEPS:
        limit = LIMIT_S.get(step, 300)
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)],
                                 capture_output=True, text=True, timeout=limit)
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
