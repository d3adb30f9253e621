"""Numpy restatement of the vertex parametrisation of corridor waypoints (test code only; shares nothing with the kernels of
allocnet_amd/csrc/sfc_param_kernels.h but the formulas of the issue):

    forward    S = sum_j xi_j^2,  P = (sum_j xi_j^2 v_j) / S
    gradient   dJ/dxi_j = 2 xi_j ((v_j - P) . dJ/dP) / S
    norm       w_norm max(S - 1, 0)^3,  gradient 6 w_norm max(S - 1, 0)^2 xi_j
    tiny NLS   f = |P(xi) - p|^2 and its gradient; backward_p runs the C restatement of lbfgs_optimize on it

and the composed objective in (xi, tau): forward -> oracle/minco_costgrad.c (cbind.minco_cost_grad_batch) -> backward, with the
durations through T = forward_T(tau)."""
import numpy as np

from oracle import cbind


def forward_T(tau):
    tau = np.asarray(tau, dtype=np.float64)
    return np.where(tau > 0.0, (0.5 * tau + 1.0) * tau + 1.0, 1.0 / ((0.5 * tau - 1.0) * tau + 1.0))


def dforward_T(tau):
    tau = np.asarray(tau, dtype=np.float64)
    den = (0.5 * tau - 1.0) * tau + 1.0
    return np.where(tau > 0.0, tau + 1.0, (1.0 - tau) / (den * den))


def backward_T(T):
    T = np.asarray(T, dtype=np.float64)
    return np.where(T > 1.0, np.sqrt(np.maximum(2.0 * T - 1.0, 0.0)) - 1.0, 1.0 - np.sqrt(np.maximum(2.0 / T - 1.0, 0.0)))


def forward(xi, verts):
    """xi (..., K), verts (..., K, 3) -> P (..., 3), S (...)."""
    q2 = np.square(np.asarray(xi, dtype=np.float64))
    S = q2.sum(-1)
    return np.einsum("...j,...ja->...a", q2, verts) / S[..., None], S


def norm_term(xi, w_norm=1.0):
    """(cost (...), gradient (..., K)) of w_norm max(S - 1, 0)^3."""
    xi = np.asarray(xi, dtype=np.float64)
    over = np.maximum(np.square(xi).sum(-1) - 1.0, 0.0)
    return w_norm * over ** 3, 6.0 * w_norm * (over ** 2)[..., None] * xi


def backward(xi, verts, gP, w_norm=0.0):
    """dJ/dxi (..., K) from dJ/dP (..., 3), plus the norm term's gradient."""
    xi = np.asarray(xi, dtype=np.float64)
    P, S = forward(xi, verts)
    dot = np.einsum("...ja,...a->...j", verts - P[..., None, :], gP)
    return 2.0 * xi * dot / S[..., None] + norm_term(xi, w_norm)[1]


def tiny_nls(x, verts, p):
    """f = |P(x) - p|^2 and df/dx for one waypoint: x (K,), verts (K, 3), p (3,)."""
    P, _ = forward(x, verts)
    r = P - p
    return float(r @ r), backward(x, verts, 2.0 * r)


TINY = dict(mem_size=8, g_epsilon=0.0, past=3, delta=1e-16)
TINY_MAX_EVALS = 200


def backward_p(p, verts, k):
    """The restatement's own run of backward_p for one waypoint: lbfgs_optimize (C restatement) on tiny_nls from the vertex mean,
    stopped after at most 200 evaluations.  Returns (xi of unit norm (K,), |P(xi) - p|)."""
    K = len(verts)
    x0 = np.zeros(K)
    x0[:k] = 1.0 / np.sqrt(k)
    evals = [0]

    def fun(x):
        evals[0] += 1
        return tiny_nls(x, verts, p)

    def progress(x, g, fx, step, it, ls):
        return evals[0] >= TINY_MAX_EVALS
    ret, x, f, it, ev = cbind.lbfgs_optimize(x0, fun, cbind.lbfgs_default_param(**TINY), progress=progress)
    x = x / np.linalg.norm(x)
    return x, float(np.linalg.norm(forward(x, verts)[0] - p))


class Composed:
    """One problem's objective in x = (xi (N-1, K) flattened, tau (N,)): f(x) -> (cost, gradient)."""

    def __init__(self, s, head, tail, hpolys, verts, pen, w_norm=1.0, with_times=True):
        self.s, self.head, self.tail, self.hp, self.verts = s, head[None], tail[None], None if hpolys is None else hpolys[None], verts
        self.kw = dict(rho=pen["rho"], res=pen["res"], vmax=pen["max_vel"], amax=pen["max_acc"], wc=pen["w_corridor"],
                       wv=pen["w_vel"], wa=pen["w_acc"], mu=pen["smooth_mu"])
        self.w_norm, self.with_times = w_norm, with_times
        self.Nm1, self.K = verts.shape[:2]
        self.T_fixed = None

    def split(self, x):
        nxi = self.Nm1 * self.K
        return x[:nxi].reshape(self.Nm1, self.K), x[nxi:]

    def waypoints(self, x):
        return forward(self.split(x)[0], self.verts)[0]

    def __call__(self, x):
        xi, tau = self.split(x)
        T = forward_T(tau) if self.with_times else self.T_fixed
        P, _ = forward(xi, self.verts)
        cost, gP, gT = cbind.minco_cost_grad_batch(self.s, self.head, self.tail, P[None], T[None], self.hp, **self.kw)
        g_xi = backward(xi, self.verts, gP[0], self.w_norm)
        f = float(cost[0]) + float(norm_term(xi, self.w_norm)[0].sum())
        g = g_xi.ravel()
        if self.with_times:
            g = np.concatenate([g, gT[0] * dforward_T(tau)])
        return f, g


def pack_vertices(vlist, K):
    """A list of (k_i, 3) vertex arrays -> (verts (n, K, 3) zero-padded, count (n,))."""
    verts = np.zeros((len(vlist), K, 3))
    count = np.zeros(len(vlist), dtype=np.int32)
    for i, v in enumerate(vlist):
        k = min(len(v), K)
        verts[i, :k] = v[:k]
        count[i] = k
    return verts, count


# ---- the inputs of the tests ----------------------------------------------------------------------------------------------------
# (seed, B, N, M) of synth.corridor_problem, and per input: the smallest Chebyshev depth of an overlap (HiGHS), the largest vertex
# count (Qhull) and the K that so truncates nothing -- re-asserted by tests/test_sfc_opt_cpu.py
INPUTS = [(1, 257, 8, 16), (7, 65, 3, 12), (9, 65, 2, 8)]
MIN_DEPTH = 0.34
MAX_COUNT = {1: 30, 7: 22, 9: 14}
K_OF = {1: 32, 7: 24, 9: 16}


def corridor(seed, B, N, M, c=3):
    from allocnet_amd.synth import corridor_problem
    return corridor_problem(np.random.default_rng(seed), B, N, c, M)


def stacked_raw(hp):
    """hp (B, N, M, 4) rows a.x <= b -> (B, N-1, 2 M, 4) the stacked pairs in raw form h.[x;1] <= 0."""
    st = np.concatenate([hp[:, :-1], hp[:, 1:]], axis=2).copy()
    st[..., 3] *= -1.0
    return st


def row_violation(hp_pair_raw, P):
    """Largest n.P + d over the unit rows of a stacked pair (<= 0 inside)."""
    from tests import polytope_np as pnp
    n, d, _ = pnp.unit_rows(hp_pair_raw)
    return float((n @ P + d).max())
