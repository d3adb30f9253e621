"""Cost + gradient on the edge-input families of tests/edge_problems.py, through EVERY kernel form that shares the reduced,
unpivoted block-LDL' solve and its adjoint, against the C port (oracle/minco_costgrad.c, classic banded LU; its own error on
these inputs is pinned by tests/test_costgrad_envelope_cpu.py at <= 1e-9, measured <= 7.5e-11).

Every form sees the same 48 distinct trajectories per family and shape; larger batches are the 48 tiled, and every tiled copy
must return what the first 48 return.  Two kinds of bars:

* FIXED -- the parity bars of the other cost + gradient tests (cost 1e-9, gradients 1e-7 of max(1, |g|_inf), coefficients 1e-9
  of the trajectory's largest), where DESIGN.md section 2 promises no loss: durations scaled together, a 100 m offset, hover,
  stationary, constant velocity, a spread of up to 10;
* MEASURED -- ten times the worst error recorded on the device over three seeds (ENVELOPE below = the table of DESIGN.md
  section 2, cell for cell), for spreads of up to 25, 50 and 100, the alternating 0.05 s / 2.5 s family and a 10 km offset.
  Whatever was measured: (a) up to a spread of 50 everything stays within 1e-6, (b) no form is more than 100 x worse than the
  best form on the same inputs.  (a) has ONE open cell, A_OPEN below: the coefficients of the 5-piece snap chain of the
  alternating family come out 2.5e-6 from every form and from the host restatement of the algorithm alike (the Gram form's
  conditioning; cost 1.1e-10, gradP 1.2e-9, gradT 6.9e-8 on the same trajectories) -- asserted at 10 x that, open in DESIGN.md.

Errors are per trajectory: cost relative, gradients over max(1, |ref|_inf) of that trajectory, coefficients over its largest
coefficient."""
import functools

import numpy as np
import pytest

from oracle import cbind
from tests import edge_problems as ep

pytestmark = pytest.mark.gpu

NT = 48                                                    # distinct trajectories per family and shape
SHAPES = [(4, 3, 8, 16), (3, 3, 16, 12), (4, 4, 5, 7)]     # (s, c, N, M): the two exact shapes and a generic one
EXACT = SHAPES[:2]
FIXED = ("spread0.5", "scale0.05", "scale20", "offset1e2", "hover", "stationary", "constant_velocity")
MEASURED = ("spread0.7", "spread0.85", "spread1.0", "alternating", "offset1e4")
UP_TO_50 = ("spread0.7", "spread0.85", "alternating")      # conditions (a) and (b)
assert set(FIXED) | set(MEASURED) == set(ep.FAMILIES)
BAR = dict(cost=1e-9, gradP=1e-7, gradT=1e-7, coef=1e-9, energy=1e-9)
LARGE = 16384 + 257

# The cost + gradient forms and how a batch reaches them (api_cost_grad.hip: cost_grad_in_one_launch, piece_grad_shape).
# launches / pshape are ASSERTED through aa.minco_cost_grad_launches / aa.minco_piece_grad_shape.
#   res = 65 is past the one-launch kernel's basis table (kFusedMaxRes = 64): three launches at any small batch.
#   pshape 2: two lanes per pair and the samples over four waves (<= 16384 pairs); 1: two lanes per pair; 0: k_piece_grad with a
#   lane per pair; 3: k_piece_grad_mx.  The exact 8-piece snap shape at 20 samples stays in ONE launch up to six rounds of groups
#   (24576 trajectories on 256 compute units), so its streaming batch is the first tiled size past that.
CG_FORMS = {
    "fused_g1": dict(B=NT, res=20, launches=1),
    "fused_mx": dict(B=4096, res=20, launches=1),          # groups of 16 (8 for 16 pieces); exact shapes: phase 2 on the matrix instructions
    "fused_vec": dict(B=4096, res=7, launches=1),
    "three_48": dict(B=NT, res=65, launches=3, pshape=2),
    "three_300": dict(B=300, res=65, launches=3, pshape=2),
    "three_4096": dict(B=4096, res=65, launches=3, pshape=1),
    "large_vec": dict(B=LARGE, res=7, launches=3, pshape=0),
    "large_mx": dict(B=LARGE, res=20, launches=3, pshape=3),
}
# The solve-only forms through aa.minco_solve_dev (no pivoted re-solve on top).  api_solve.hip launch_solve: up to 16384 a lane per
# (trajectory, axis), and for the exact shapes up to 4096 two lanes per axis (the chain from both ends); beyond, a lane per trajectory.
SOLVE_FORMS = {
    "solve_130": dict(B=130),                              # exact shapes: k_minco_solve_axis_two; generic: k_minco_solve_axis
    "solve_2048": dict(B=2048),                            # the same kernels, several workgroups per CU
    "solve_axis": dict(B=4096 + 130),                      # k_minco_solve_axis for every shape
    "solve_lane": dict(B=LARGE),                           # k_minco_solve
}
# forms whose lanes do the same work on every tiled copy (a lane owns a whole trajectory or a whole axis of one, no cross-lane
# reduction whose partner changes with the position in the batch): copies bit for bit
BITWISE_COPIES = ("solve_lane", "solve_axis", "solve_130", "solve_2048")

# ---------------------------------------------------------------------------------------------------------------------------
# DESIGN.md section 2, tables "Measured envelope of the reduced form": the worst error on an MI355X over seeds 0, 1, 2 and the three
# shapes, per family (row) and form and quantity (column), rounded up to two digits -- measured 2026-10-18 with the kernels of commit
# f2794c2.  Every literal below IS a cell of those tables; the tests assert 10 x the cell (in the conditioning-dominated regime the
# error moves by up to an order of magnitude between draws).  Not to be widened to make a failing kernel pass: a form that leaves
# its cell by more than that has changed its arithmetic.
ENVELOPE = {
    "spread0.7": {
        "fused_g1": dict(cost=5.1e-11, gradP=9.4e-11, gradT=2.5e-10, coef=1.1e-10),
        "fused_mx": dict(cost=5.1e-11, gradP=5.8e-11, gradT=2.5e-10, coef=1.1e-10),
        "fused_vec": dict(cost=5.1e-11, gradP=3.6e-10, gradT=2.7e-10, coef=1.1e-10),
        "three_48": dict(cost=1.4e-10, gradP=9.1e-11, gradT=2.5e-10, coef=1.1e-10),
        "three_300": dict(cost=1.4e-10, gradP=9.1e-11, gradT=2.5e-10, coef=1.1e-10),
        "three_4096": dict(cost=1.4e-10, gradP=6.8e-11, gradT=2.3e-10, coef=1.1e-10),
        "large_vec": dict(cost=1.4e-10, gradP=3.7e-10, gradT=3.9e-10, coef=9.6e-11),
        "large_mx": dict(cost=1.4e-10, gradP=1.7e-10, gradT=4.4e-10, coef=9.6e-11),
        "solve_130": dict(coef=1.1e-10, energy=2.9e-12),
        "solve_2048": dict(coef=1.1e-10, energy=2.9e-12),
        "solve_axis": dict(coef=9.6e-11, energy=2.9e-12),
        "solve_lane": dict(coef=9.6e-11, energy=2.9e-12),
        "sample": dict(cost=2.0e-12),
        "lbfgs": dict(cost=2.0e-10),
    },
    "spread0.85": {
        "fused_g1": dict(cost=1.4e-10, gradP=4.0e-10, gradT=7.8e-10, coef=5.1e-10),
        "fused_mx": dict(cost=1.4e-10, gradP=4.0e-10, gradT=6.9e-10, coef=5.1e-10),
        "fused_vec": dict(cost=1.4e-10, gradP=2.3e-09, gradT=1.0e-09, coef=5.1e-10),
        "three_48": dict(cost=1.4e-10, gradP=4.1e-10, gradT=5.8e-10, coef=5.1e-10),
        "three_300": dict(cost=1.4e-10, gradP=4.1e-10, gradT=5.8e-10, coef=5.1e-10),
        "three_4096": dict(cost=1.4e-10, gradP=4.1e-10, gradT=7.2e-10, coef=5.1e-10),
        "large_vec": dict(cost=1.4e-10, gradP=3.4e-10, gradT=1.1e-09, coef=4.7e-10),
        "large_mx": dict(cost=1.4e-10, gradP=4.1e-10, gradT=6.2e-10, coef=4.7e-10),
        "solve_130": dict(coef=5.1e-10, energy=1.2e-11),
        "solve_2048": dict(coef=5.1e-10, energy=1.2e-11),
        "solve_axis": dict(coef=4.7e-10, energy=1.2e-11),
        "solve_lane": dict(coef=4.7e-10, energy=1.2e-11),
        "sample": dict(cost=1.2e-11),
        "lbfgs": dict(cost=6.8e-10),
    },
    "spread1.0": {
        "fused_g1": dict(cost=4.6e-09, gradP=3.3e-08, gradT=3.4e-07, coef=5.0e-09),
        "fused_mx": dict(cost=4.6e-09, gradP=2.3e-08, gradT=3.5e-07, coef=5.0e-09),
        "fused_vec": dict(cost=4.6e-09, gradP=1.6e-08, gradT=3.3e-07, coef=5.0e-09),
        "three_48": dict(cost=4.7e-09, gradP=3.2e-08, gradT=1.1e-07, coef=5.0e-09),
        "three_300": dict(cost=4.7e-09, gradP=3.2e-08, gradT=1.1e-07, coef=5.0e-09),
        "three_4096": dict(cost=4.7e-09, gradP=2.3e-08, gradT=1.1e-07, coef=5.0e-09),
        "large_vec": dict(cost=4.6e-09, gradP=1.5e-08, gradT=5.4e-07, coef=4.2e-09),
        "large_mx": dict(cost=4.6e-09, gradP=2.4e-08, gradT=5.5e-07, coef=4.2e-09),
        "solve_130": dict(coef=5.0e-09, energy=4.5e-11),
        "solve_2048": dict(coef=5.0e-09, energy=4.5e-11),
        "solve_axis": dict(coef=4.2e-09, energy=4.5e-11),
        "solve_lane": dict(coef=4.2e-09, energy=4.5e-11),
        "sample": dict(cost=4.5e-11),
        "lbfgs": dict(cost=3.5e-09),
    },
    "alternating": {
        "fused_g1": dict(cost=1.1e-10, gradP=1.2e-09, gradT=6.9e-08, coef=2.5e-06),
        "fused_mx": dict(cost=1.1e-10, gradP=1.2e-09, gradT=6.9e-08, coef=2.5e-06),
        "fused_vec": dict(cost=1.1e-10, gradP=2.7e-09, gradT=8.3e-08, coef=2.5e-06),
        "three_48": dict(cost=9.2e-11, gradP=7.0e-10, gradT=5.3e-08, coef=2.5e-06),
        "three_300": dict(cost=9.2e-11, gradP=7.0e-10, gradT=5.3e-08, coef=2.5e-06),
        "three_4096": dict(cost=9.2e-11, gradP=6.8e-10, gradT=5.3e-08, coef=2.5e-06),
        "large_vec": dict(cost=9.8e-11, gradP=2.5e-09, gradT=5.7e-08, coef=2.5e-06),
        "large_mx": dict(cost=9.8e-11, gradP=1.2e-09, gradT=5.1e-08, coef=2.5e-06),
        "solve_130": dict(coef=2.5e-06, energy=7.9e-12),
        "solve_2048": dict(coef=2.5e-06, energy=7.9e-12),
        "solve_axis": dict(coef=2.5e-06, energy=7.9e-12),
        "solve_lane": dict(coef=2.5e-06, energy=7.9e-12),
        "sample": dict(cost=7.9e-12),
        "lbfgs": dict(cost=3.5e-10),
    },
    "offset1e4": {
        "fused_g1": dict(cost=4.2e-12, gradP=1.9e-11, gradT=1.6e-09, coef=4.0e-13),
        "fused_mx": dict(cost=4.2e-12, gradP=1.9e-11, gradT=1.6e-09, coef=4.0e-13),
        "fused_vec": dict(cost=4.2e-12, gradP=2.8e-11, gradT=1.6e-09, coef=4.0e-13),
        "three_48": dict(cost=4.2e-12, gradP=1.5e-11, gradT=1.5e-09, coef=4.0e-13),
        "three_300": dict(cost=4.2e-12, gradP=1.5e-11, gradT=1.5e-09, coef=4.0e-13),
        "three_4096": dict(cost=4.2e-12, gradP=1.5e-11, gradT=1.6e-09, coef=4.0e-13),
        "large_vec": dict(cost=4.2e-12, gradP=2.8e-11, gradT=1.7e-09, coef=4.0e-13),
        "large_mx": dict(cost=4.2e-12, gradP=1.9e-11, gradT=1.6e-09, coef=4.0e-13),
        "solve_130": dict(coef=4.0e-13, energy=4.3e-12),
        "solve_2048": dict(coef=4.0e-13, energy=4.3e-12),
        "solve_axis": dict(coef=4.0e-13, energy=4.3e-12),
        "solve_lane": dict(coef=4.0e-13, energy=4.3e-12),
        "sample": dict(cost=4.1e-12),
        "lbfgs": dict(cost=4.5e-12),
    },
}


@functools.lru_cache(maxsize=None)
def problem(family, shape, seed=0):
    s, c, N, M = shape
    out = ep.make(family, seed, NT, N, c, M)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(family, shape, res, seed=0):
    """C port on the 48 distinct trajectories: cost, gradP, gradT, coefficients, energy -- computed once, shared, read-only."""
    s, c, N, M = shape
    head, tail, wps, T, hp = problem(family, shape, seed)
    cost, gP, gT = cbind.minco_cost_grad_batch(s, head, tail, wps, T, hp, ep.RHO, nthreads=4, **ep.penalty_kw(family, res))
    co, en = cbind.minco_solve_batch(s, head, tail, wps, T)
    out = dict(cost=cost, gradP=gP, gradT=gT, coef=co, energy=en, penalty=cost - en - ep.RHO * T.sum(axis=1))
    for a in out.values():
        a.setflags(write=False)
    return out


def _scale(name, ref):
    """Per-trajectory scale of a quantity's error (module docstring)."""
    r = np.abs(ref).reshape(NT, -1).max(axis=1)
    return r if name in ("cost", "coef", "energy") else np.maximum(1.0, r)


def _errors(got, ref, names):
    """got[name]: (B, ...) with B >= 48, trajectory b a copy of b % 48.  -> per-trajectory errors of the first 48 against the
    reference, the largest deviation of any copy from its original (same scales), and whether all copies are the same bits."""
    err, dev, bits = {}, 0.0, True
    for k in names:
        g = got[k]
        B = g.shape[0]
        base = g[:NT]
        sc = _scale(k, ref[k])
        err[k] = np.abs(base - ref[k]).reshape(NT, -1).max(axis=1) / sc
        if B > NT:
            idx = np.arange(B) % NT
            d = np.abs(g - base[idx]).reshape(B, -1).max(axis=1) / sc[idx]
            dev = max(dev, float(d.max())); bits = bits and bool(np.array_equal(g, base[idx]))
    return err, dev, bits


def _tile(a, B):
    return a[np.arange(B) % NT]


def _large_batch(aa, ctx, s, c, N, pen, want):
    """The first tiled size from 16384 + 257 on that takes three launches (see CG_FORMS)."""
    for B in (LARGE, 6 * 256 * 16 + 257, 8 * 256 * 16 + 257):
        if aa.minco_cost_grad_launches(s, N, B, penalty=pen, ctx=ctx, c=c) == want:
            return B
    return LARGE


@functools.lru_cache(maxsize=None)
def run_cost_grad(family, shape, form, seed=0):
    import allocnet_amd as aa
    ctx = aa.default_context(0)
    s, c, N, M = shape
    f = CG_FORMS[form]
    kw = ep.penalty_kw(family, f["res"])
    pen = aa.make_penalty(rho=ep.RHO, w_corridor=kw["wc"], w_vel=kw["wv"], w_acc=kw["wa"], smooth_mu=kw["mu"], max_vel=kw["vmax"],
                          max_acc=kw["amax"], res=kw["res"], poly_rows=M)
    B = f["B"] if f["B"] != LARGE else _large_batch(aa, ctx, s, c, N, pen, f["launches"])
    head, tail, wps, T, hp = (_tile(a, B) for a in problem(family, shape, seed))
    cost, gP, gT, co = aa.minco_cost_grad(head, tail, wps, T, s, hpolys=hp, penalty=pen, want_coeffs=True, ctx=ctx)
    ref = reference(family, shape, f["res"], seed)
    err, dev, bits = _errors(dict(cost=cost, gradP=gP, gradT=gT, coef=co), ref, ("cost", "gradP", "gradT", "coef"))
    return dict(err=err, copy_dev=dev, copy_bits=bits, B=B, cost=cost[:NT].copy(),
                finite=bool(np.isfinite(cost).all() and np.isfinite(gP).all() and np.isfinite(gT).all() and np.isfinite(co).all()),
                launches=aa.minco_cost_grad_launches(s, N, B, penalty=pen, ctx=ctx, c=c),
                pshape=aa.minco_piece_grad_shape(s, N, B, penalty=pen, ctx=ctx),
                active=int((ref["penalty"] > 1e-12 * ref["cost"]).sum()))


@functools.lru_cache(maxsize=None)
def run_solve(family, shape, form, seed=0):
    import torch
    import allocnet_amd as aa
    from tools.bench_configs import to_bm
    ctx = aa.default_context(0)
    s, c, N, M = shape
    B = SOLVE_FORMS[form]["B"]
    dev = torch.device("cuda", 0)
    ld = aa.recommended_ld(B)
    head, tail, wps, T, _ = (_tile(a, B) for a in problem(family, shape, seed))
    th, tt, tw, tT = (to_bm(torch, x, B, ld, dev) for x in (head, tail, wps, T))
    tT[:, B:] = 1.0                                         # (padding columns: any positive duration)
    co = torch.empty(N * 3 * 2 * s, ld, device=dev, dtype=torch.float64); en = torch.empty(ld, device=dev, dtype=torch.float64)
    aa.minco_solve_dev(th, tt, tw, tT, s, c, N, B, coeffs=co, energy=en, ctx=ctx)
    torch.cuda.synchronize()
    got = dict(coef=co[:, :B].T.cpu().numpy().reshape(B, N, 3, 2 * s), energy=en[:B].cpu().numpy())
    ref = reference(family, shape, 7, seed)
    err, devn, bits = _errors(got, ref, ("coef",))
    # energy: relative -- where the exact energy is zero (stationary, constant velocity) against rho * sum T, like the cost
    sc = ep.RHO * problem(family, shape, seed)[3].sum(axis=1) if family in ep.NO_PENALTY else np.abs(ref["energy"])
    idx = np.arange(B) % NT
    err["energy"] = np.abs(got["energy"][:NT] - ref["energy"]) / sc
    devn = max(devn, float((np.abs(got["energy"] - got["energy"][idx]) / sc[idx]).max()))
    bits = bits and bool(np.array_equal(got["energy"], got["energy"][idx]))
    return dict(err=err, copy_dev=devn, copy_bits=bits, B=B, finite=bool(np.isfinite(got["coef"]).all() and np.isfinite(got["energy"]).all()))


SAMPLE_PROBLEMS = 4


@functools.lru_cache(maxsize=None)
def run_sample(family, shape, seed=0):
    """k_minco_sample: the family's 48 duration vectors as candidates for each of its first four problems, against the C port's
    energy + rho * sum T of every candidate.  -> relative cost error per (problem, candidate)."""
    import allocnet_amd as aa
    ctx = aa.default_context(0)
    s, c, N, M = shape
    head, tail, wps, T, _ = problem(family, shape, seed)
    err = np.empty((SAMPLE_PROBLEMS, NT)); fin = True
    for p in range(SAMPLE_PROBLEMS):
        cost = aa.minco_sample_costs(head[p], tail[p], wps[p], T, s, rho=ep.RHO, ctx=ctx)
        rep = lambda x: np.repeat(x[p:p + 1], NT, axis=0)
        _, en = cbind.minco_solve_batch(s, rep(head), rep(tail), rep(wps), T, want_coeffs=False)
        ref = en + ep.RHO * T.sum(axis=1)
        err[p] = np.abs(cost - ref) / np.abs(ref); fin = fin and bool(np.isfinite(cost).all())
    return dict(err=dict(cost=err.max(axis=0)), finite=fin)


@functools.lru_cache(maxsize=None)
def run_lbfgs_eval(family, shape, seed=0):
    """The evaluation inside k_lbfgs_minco_persistent (one wave per problem, the chain factored from both ends): one iteration over
    the waypoints only -- the durations, and so the spread, stay the family's -- and the cost it reports for the point it returns
    against the C port's cost of that point."""
    import allocnet_amd as aa
    ctx = aa.default_context(0)
    s, c, N, M = shape
    head, tail, wps, T, hp = problem(family, shape, seed)
    kw = ep.penalty_kw(family, 20)
    pen = aa.make_penalty(rho=ep.RHO, w_corridor=kw["wc"], w_vel=kw["wv"], w_acc=kw["wa"], smooth_mu=kw["mu"], max_vel=kw["vmax"],
                          max_acc=kw["amax"], res=kw["res"], poly_rows=M)
    out = aa.lbfgs_minco(head, tail, wps, T, s, hpolys=hp, penalty=pen, param=aa.lbfgs_parameter_t(max_iterations=1),
                         opt=aa.lbfgs.OPT_WAYPOINTS, max_evals=40, want_coeffs=False, ctx=ctx)
    assert np.array_equal(out["T"], T)
    ref, _, _ = cbind.minco_cost_grad_batch(s, head, tail, out["wps"], T, hp, ep.RHO, nthreads=4, **kw)
    sc = ep.RHO * T.sum(axis=1) if family in ep.NO_PENALTY else np.abs(ref)
    return dict(err=dict(cost=np.abs(out["cost"] - ref) / sc), finite=bool(np.isfinite(out["cost"]).all()),
                moved=int((np.abs(out["wps"] - wps).reshape(NT, -1).max(axis=1) > 0).sum()), evals=out["evals"].copy())


def _kept(family, shape, seed=0):
    """The trajectories a test compares: all whose realised spread is inside the family's nominal bound -- at least 44 of 48, and
    never chosen by their error."""
    T = problem(family, shape, seed)[3]
    bound = ep.SPREAD_BOUND.get(family)
    keep = np.ones(NT, dtype=bool) if bound is None else ep.spread_of(T) <= bound * (1 + 1e-12)
    assert keep.sum() >= NT - 4
    return keep


# Condition (a) holds in every cell but these: the 5-piece snap chain of the alternating family (every 0.05 s piece between two
# 2.5 s pieces, c = 4) loses 1e-6 on its COEFFICIENTS in every form alike, and so does the host restatement of the same algorithm
# (oracle/minco_cpu_reduced.cpp: 2.5e-6) -- a property of the reduced Gram form, not of a kernel (open item;
# cost and gradients of the same trajectories stay within 1e-6).  There the bar is 10 x the measured cell.
A_OPEN = {("alternating", (4, 4, 5, 7), "coef")}


def _bars(family, shape, form):
    """The bar of every quantity for this family and form: the fixed parity bars, or 10 x the cell of DESIGN.md section 2 -- and up to
    a spread of 50 never more than 1e-6 (condition (a): the north-star bar)."""
    if family in FIXED:
        return BAR
    bars = {k: 10.0 * v for k, v in ENVELOPE[family][form].items()}
    if family in UP_TO_50:
        bars = {k: v if (family, shape, k) in A_OPEN else min(v, 1e-6) for k, v in bars.items()}
    return bars


def _check(family, shape, form, r):
    keep = _kept(family, shape)
    assert r["finite"]
    bars = _bars(family, shape, form)
    worst = {k: float(e[keep].max()) for k, e in r["err"].items()}
    print(f"{family} {shape} {form}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + (f" | copies {r['copy_dev']:.1e} bits {r['copy_bits']}" if "copy_dev" in r else ""))
    for k, v in worst.items():
        assert v <= bars[k], (family, shape, form, k, v, bars[k])
    if "copy_dev" in r:
        assert r["copy_dev"] <= 1e-12, (family, shape, form, r["copy_dev"])
        if form in BITWISE_COPIES:
            assert r["copy_bits"], (family, shape, form)


@pytest.mark.parametrize("form", list(CG_FORMS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "s%dc%dN%dM%d" % sh)
@pytest.mark.parametrize("family", ep.FAMILIES)
def test_cost_grad_form(anet_ctx, family, shape, form):
    r = run_cost_grad(family, shape, form)
    f = CG_FORMS[form]
    assert r["launches"] == f["launches"], (form, r["B"], r["launches"])      # the intended form ran
    if "pshape" in f:
        assert r["pshape"] == f["pshape"], (form, r["B"], r["pshape"])
    if family in ep.NO_PENALTY:
        T = problem(family, shape)[3]
        assert r["active"] == 0
        assert (np.abs(r["cost"] - ep.RHO * T.sum(axis=1)) <= 1e-9 * ep.RHO * T.sum(axis=1)).all()
    else:
        assert 2 * r["active"] >= NT                     # the penalty is active on at least half of the compared trajectories
    _check(family, shape, form, r)


@pytest.mark.parametrize("form", list(SOLVE_FORMS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "s%dc%dN%dM%d" % sh)
@pytest.mark.parametrize("family", ep.FAMILIES)
def test_solve_only_form(anet_ctx, family, shape, form):
    _check(family, shape, form, run_solve(family, shape, form))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "s%dc%dN%dM%d" % sh)
@pytest.mark.parametrize("family", ep.FAMILIES)
def test_sampled_duration_costs(anet_ctx, family, shape):
    _check(family, shape, "sample", run_sample(family, shape))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "s%dc%dN%dM%d" % sh)
@pytest.mark.parametrize("family", ep.FAMILIES)
def test_evaluation_inside_the_persistent_lbfgs(anet_ctx, family, shape):
    _check(family, shape, "lbfgs", run_lbfgs_eval(family, shape))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda sh: "s%dc%dN%dM%d" % sh)
@pytest.mark.parametrize("family", UP_TO_50)
def test_no_form_is_two_orders_worse_than_the_best(anet_ctx, family, shape):
    """Condition (b): all forms implement the same reduced algebra, so on the same inputs an outlier by two orders is a defect of
    that form (its staging, its both-ends meeting block, its reduction order), not conditioning.  Cost and gradients among the
    cost + gradient forms OF THE SAME SAMPLE COUNT (the reference changes with it), coefficients among all of them and the
    solve-only forms, energy among the solve-only forms."""
    keep = _kept(family, shape)
    groups = {}
    for form, f in CG_FORMS.items():
        r = run_cost_grad(family, shape, form)
        for k in ("cost", "gradP", "gradT"):
            groups.setdefault((k, f["res"]), {})[form] = float(r["err"][k][keep].max())
        groups.setdefault(("coef", 0), {})[form] = float(r["err"]["coef"][keep].max())
    for form in SOLVE_FORMS:
        r = run_solve(family, shape, form)
        groups[("coef", 0)][form] = float(r["err"]["coef"][keep].max())
        groups.setdefault(("energy", 0), {})[form] = float(r["err"]["energy"][keep].max())
    for (k, res), errs in groups.items():
        best = min(errs.values())
        print(f"{family} {shape} {k} res={res}: best {min(errs.values()):.2e} worst {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
        for form, v in errs.items():
            assert v <= 100.0 * best, (family, shape, k, form, v, best)


def _lbfgs_wide_spread_problem(seed=9):
    """The problem of tests/test_lbfgs_gpu.py::test_returned_coefficients_of_wide_spread_durations...: the first half ends an
    optimisation with durations spread over more than 10^3, the second half with ordinary ones."""
    rng = np.random.default_rng(seed)
    s, c, N, B = 4, 3, 6, 24
    seg = np.tile(np.array([0.004, 9.0, 0.004, 7.0, 0.004, 8.0]), (B, 1)) * rng.uniform(0.8, 1.2, size=(B, N))
    d = rng.normal(size=(B, N, 3)); d /= np.linalg.norm(d, axis=2, keepdims=True)
    pts = np.concatenate([np.zeros((B, 1, 3)), np.cumsum(d * seg[:, :, None], axis=1)], axis=1)
    head = np.zeros((B, 3, c)); tail = np.zeros((B, 3, c))
    head[:, :, 0] = pts[:, 0]; tail[:, :, 0] = pts[:, N]
    wps = pts[:, 1:N].copy()
    T = np.where(seg < 0.1, 0.012, 30.0) * rng.uniform(0.9, 1.1, size=(B, N))
    T[B // 2:] = rng.uniform(0.8, 1.6, size=(B - B // 2, N))
    return s, c, N, B, head, tail, wps, T


# DESIGN.md section 2, "The cost the persistent L-BFGS reports": worst relative error of the reported cost over the wide half (seeds
# 9, 10, 11), after one iteration (an ordinary point: the energy is what the start's was) and after three (the waypoints have moved to
# where the energy is eleven orders below the terms it is summed from: the reported cost is rounding noise there, see the open item)
LBFGS_WIDE_COST = {1: 2.2e-08, 3: 29.0}


def lbfgs_reported_cost_errors(ctx, iterations, seed=9):
    import allocnet_amd as aa
    s, c, N, B, head, tail, wps, T = _lbfgs_wide_spread_problem(seed)
    kw = dict(res=4, vmax=4.0, amax=6.0, wc=0.0, wv=0.0, wa=0.0, mu=1e-2)
    pen = aa.make_penalty(rho=1e-6, w_corridor=0.0, w_vel=0.0, w_acc=0.0, smooth_mu=kw["mu"], max_vel=kw["vmax"], max_acc=kw["amax"],
                          res=kw["res"], poly_rows=0)
    out = aa.lbfgs_minco(head, tail, wps, T, s, penalty=pen, param=aa.lbfgs_parameter_t(max_iterations=iterations), max_evals=60,
                         ctx=ctx)
    spread = ep.spread_of(out["T"])
    assert (spread[:B // 2] > 1e3).all() and (spread[B // 2:] < 50).all(), spread
    ref, _, _ = cbind.minco_cost_grad_batch(s, head, tail, out["wps"], out["T"], None, 1e-6, **kw)
    err = np.abs(out["cost"] - ref) / np.abs(ref)
    return err[:B // 2], err[B // 2:]


@pytest.mark.parametrize("iterations", [1, 3])
def test_lbfgs_reported_cost_at_wide_spread_matches_the_c_port(anet_ctx, iterations):
    """The problem of test_returned_coefficients_of_wide_spread_durations...: the cost the persistent kernel reports for the point it
    returns is the C port's cost of that point -- to the parity bar where the returned durations are ordinary, to 10 x the measured
    value where they spread over more than 10^3 (there the loop works with the reduced system; only the returned coefficients are
    re-solved)."""
    wide, ordinary = lbfgs_reported_cost_errors(anet_ctx, iterations)
    print(f"lbfgs reported cost after {iterations} iterations: wide {wide.max():.2e} ordinary {ordinary.max():.2e}")
    assert ordinary.max() <= BAR["cost"]
    assert wide.max() <= 10.0 * LBFGS_WIDE_COST[iterations]
