"""Numpy restatement of the shortest route through a corridor (test code only; shares nothing with the kernel of
allocnet_amd/csrc/sfc_path_kernels.h but the formulas of the issue):

    P_0 = start, P_N = goal, P_w(xi) for w = 1 .. N-1 the transform of tests/sfc_np.py on the vertices of overlap(w-1, w)
    L(xi) = sum_{i=0}^{N-1} sqrt(|P_{i+1} - P_i|^2 + eps^2) + w_norm sum_w max(S_w - 1, 0)^3
    dL/dP_w = (P_w - P_{w-1}) / l_{w-1} - (P_{w+1} - P_w) / l_w,  then sfc_np.backward

its own route solve (the C restatement of lbfgs_optimize on it, from the vertex mean) and a convex reference: the same L
minimised over the points P themselves subject to the rows of both polytopes of every junction (scipy SLSQP, ftol 1e-14, started
from the restatement's result).  The legs are strictly convex in P for eps > 0, so the value of that programme is unique."""
import functools

import numpy as np

from oracle import cbind
from tests import polytope_np as pnp
from tests import sfc_np

EPS_M = 1e-2                # the smoothing length of the legs, metres
ENUM_EPS = 1e-6             # the enumeration's epsilon
DEFAULTS = dict(mem_size=8, past=3, delta=1e-6, g_epsilon=1e-5)
MAX_EVALS = 400

# ---- the inputs of the tests: sfc_np.INPUTS, the whole of seeds 9 and 7 and the first 32 problems of seed 1 -------------------------
# seed -> (problems, pieces N, rows M)
SUBSET = {9: (65, 2, 8), 7: (65, 3, 12), 1: (32, 8, 16)}
# Measured by measure() below (python -m tests.sfc_path_np) with the restatement's own run on this CPU -- never from the device:
#   seed  N  problems  worst gap   median evaluations  max evaluations   vertex-mean start above the optimum (median)
#   9     2  65        4.67e-05    16                  54                26 %
#   7     3  65        2.07e-04    20                  169               45 %
#   1     8  32        1.79e-04    92.5                258               109 %
# gap = (smoothed length of the restatement's route - convex optimum) / convex optimum; every run ended by its own stopping test
# (LBFGS_CONVERGENCE or LBFGS_STOP), none at the 400 evaluations.  GAP is twice the largest.
WORST_GAP = {9: 4.67e-05, 7: 2.07e-04, 1: 1.79e-04}
GAP = 2.0 * 2.07e-04


def legs(points, eps=EPS_M):
    """Smoothed leg lengths of a polyline (n+1, 3) -> (n,)."""
    d = np.diff(np.asarray(points, dtype=np.float64), axis=0)
    return np.sqrt(np.square(d).sum(1) + eps * eps)


def fixed_order_sum(values):
    """((v_0 + v_1) + v_2) + ...: the order in which one lane sums."""
    s = 0.0
    for v in values:
        s = s + float(v)
    return s


def polyline_length(start, wps, goal):
    """The unsmoothed length sum |P_{i+1} - P_i|."""
    return fixed_order_sum(legs(np.vstack([start, wps, goal]), 0.0))


def route_cost(xi, verts, start, goal, eps=EPS_M, w_norm=1.0):
    """L and dL/dxi of one problem: xi (N-1, K), verts (N-1, K, 3), start, goal (3,).  Returns (L, gradient (N-1, K), P (N-1, 3))."""
    xi = np.asarray(xi, dtype=np.float64)
    P, _ = sfc_np.forward(xi, verts)
    pts = np.vstack([start, P, goal])
    l = legs(pts, eps)
    d = np.diff(pts, axis=0) / l[:, None]
    gP = d[:-1] - d[1:]
    nc, _ = sfc_np.norm_term(xi, w_norm)
    L = fixed_order_sum(l) + fixed_order_sum(nc)
    return L, sfc_np.backward(xi, verts, gP, w_norm), P


def mean_start(count, K):
    """xi_j = 1 / sqrt(k) for j < k: count (N-1,) -> (N-1, K)."""
    count = np.asarray(count)
    return np.where(np.arange(K)[None, :] < count[:, None], 1.0 / np.sqrt(np.maximum(count, 1))[:, None], 0.0)


def solve(verts, count, start, goal, eps=EPS_M, w_norm=1.0, xi0=None, max_evals=MAX_EVALS, **over):
    """The restatement's own route solve: cbind.lbfgs_optimize with the defaults of the entry point, stopped after max_evals
    evaluations.  Returns dict(ret, xi (N-1, K), wps, cost, iters, evals)."""
    Nm1, K = verts.shape[:2]
    x0 = (mean_start(count, K) if xi0 is None else np.asarray(xi0, dtype=np.float64)).ravel()
    evals = [0]

    def fun(x):
        evals[0] += 1
        L, g, _ = route_cost(x.reshape(Nm1, K), verts, start, goal, eps, w_norm)
        return L, g.ravel()

    def progress(x, g, fx, step, it, ls):
        return evals[0] >= max_evals
    prm = dict(DEFAULTS); prm.update(over)
    ret, x, f, it, ev = cbind.lbfgs_optimize(x0, fun, cbind.lbfgs_default_param(**prm), progress=progress)
    xi = x.reshape(Nm1, K)
    return dict(ret=ret, xi=xi, wps=sfc_np.forward(xi, verts)[0], cost=f, iters=it, evals=ev)


def convex_optimum(pairs_raw, start, goal, P0, eps=EPS_M):
    """min over P (N-1, 3) of sum of the smoothed legs subject to the unit rows of both polytopes of every junction (pairs_raw
    (N-1, 2M, 4) stacked raw pairs), SLSQP with ftol 1e-14 from P0.  Returns (value, P)."""
    from scipy.optimize import minimize
    Nm1 = len(pairs_raw)
    A = np.zeros((0, 3 * Nm1)); d = np.zeros(0)
    for w in range(Nm1):
        n, dd, _ = pnp.unit_rows(pairs_raw[w])
        blk = np.zeros((len(n), 3 * Nm1)); blk[:, 3 * w:3 * w + 3] = n
        A = np.vstack([A, blk]); d = np.concatenate([d, dd])

    def fun(p):
        pts = np.vstack([start, p.reshape(Nm1, 3), goal])
        l = legs(pts, eps)
        u = np.diff(pts, axis=0) / l[:, None]
        return l.sum(), (u[:-1] - u[1:]).ravel()
    res = minimize(fun, np.asarray(P0, dtype=np.float64).ravel(), jac=True, method="SLSQP",
                   constraints=[dict(type="ineq", fun=lambda p: -(A @ p + d), jac=lambda p: -A)], options=dict(ftol=1e-14, maxiter=500))
    P = res.x.reshape(Nm1, 3)
    # SLSQP keeps linear constraints to rounding; a value from a point outside would not be a value of the programme
    assert (A @ res.x + d).max() <= 1e-9, (res.message, (A @ res.x + d).max())
    return float(fun(res.x)[0]), P


@functools.lru_cache(maxsize=None)
def reference(seed):
    """Everything the CPU and GPU tests share for one input, computed once per process: per problem of SUBSET[seed] the start,
    goal, stacked pairs, the vertices in the enumeration's order (pnp.enumerate_triples, padded to sfc_np.K_OF[seed]), the
    restatement's route and the convex optimum."""
    nprob, N, M = SUBSET[seed]
    _, Bf, Nf, Mf = next(i for i in sfc_np.INPUTS if i[0] == seed)
    assert (N, M) == (Nf, Mf)
    head, tail, _, _, hp = sfc_np.corridor(seed, Bf, Nf, Mf)
    K = sfc_np.K_OF[seed]
    st = sfc_np.stacked_raw(hp[:nprob])
    out = dict(start=head[:nprob, :, 0].copy(), goal=tail[:nprob, :, 0].copy(), hp=hp[:nprob].copy(), pairs=st, N=N, M=M, K=K,
               verts=np.zeros((nprob, N - 1, K, 3)), count=np.zeros((nprob, N - 1), dtype=np.int32), route=[], optimum=np.zeros(nprob),
               opt_wps=np.zeros((nprob, N - 1, 3)))
    for b in range(nprob):
        out["verts"][b], out["count"][b] = sfc_np.pack_vertices([pnp.enumerate_triples(st[b, w], ENUM_EPS)[0] for w in range(N - 1)], K)
        r = solve(out["verts"][b], out["count"][b], out["start"][b], out["goal"][b])
        out["route"].append(r)
        out["optimum"][b], out["opt_wps"][b] = convex_optimum(st[b], out["start"][b], out["goal"][b], r["wps"])
    return out


def smoothed_length(start, wps, goal, eps=EPS_M):
    return fixed_order_sum(legs(np.vstack([start, wps, goal]), eps))


def gaps(seed):
    """Relative gap of the restatement's route above the convex optimum, per problem of SUBSET[seed]."""
    R = reference(seed)
    got = np.array([smoothed_length(R["start"][b], R["route"][b]["wps"], R["goal"][b]) for b in range(len(R["optimum"]))])
    return (got - R["optimum"]) / R["optimum"]


def measure():
    for seed in (9, 7, 1):
        R = reference(seed)
        g = gaps(seed)
        ev = np.array([r["evals"] for r in R["route"]])
        mean = np.array([smoothed_length(R["start"][b], sfc_np.forward(mean_start(R["count"][b], R["K"]), R["verts"][b])[0], R["goal"][b])
                         for b in range(len(g))])
        print("seed %d N %d problems %d: worst gap %.2g (smallest %.2g), evaluations median %g max %d, vertex mean above optimum "
              "median %.0f %% worst %.2fx" % (seed, R["N"], len(g), g.max(), g.min(), np.median(ev), ev.max(),
                                              100.0 * np.median(mean / R["optimum"] - 1.0), (mean / R["optimum"]).max()))


if __name__ == "__main__":
    measure()
