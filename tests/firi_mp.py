"""TEST INFRASTRUCTURE ONLY -- 50-digit reference for the two numerical stages of FIRI (csrc/firi_kernels.h): the plane pass
(`k_firi_planes`, the loop body of firi::firi, gcopter/firi.hpp:297-405) and the objective of the inscribed-ellipsoid stage
(firi::costMVIE, firi.hpp:86-157), the latter written as a function of the ELLIPSOID (Q, p) and not of the optimiser's nine
variables, so that the iterate of any implementation can be scored with it.  Written from the statement of the algorithm; it
shares no code with oracle/firi_np.py, oracle/lbfgs_oracle.c or the product.

A double is an exact rational: every input enters as mpf(double) exactly and all arithmetic runs at DPS digits, so each
DECISION of the greedy selection (which candidate is nearest, is a point cut, does a tangent plane keep an endpoint inside) is
the decision of exact arithmetic unless its margin is below 10^-45.  The margins are returned: a float64 implementation may
legitimately decide the other way only where a margin is of the order of its rounding error, and the tests leave out (and
count) the passes where one is below 1e-9.

The plane pass, for the ellipsoid {p + R diag(r) u : |u| <= 1}:
    forward map      x -> diag(1/r) R' (x - p)          (the ellipsoid becomes the unit ball)
    boundary row h   -> (h[:3] R diag(r), h[3] + h[:3].p), distance |.[3]| / |.[:3]|
    obstacle point q (forward): the plane through q nearest the origin that keeps both forward endpoints fa, fb inside:
        form 0  tangent to the ball about the origin through q:  n = q / |q|, offset -|q|
        form 1  if that leaves fa outside (n.fa - |q| > eps): the nearest plane through q and fa
        form 2  the same for fb
        form 3  if fa is outside again: the plane through fa, fb and q, oriented to keep the origin inside
      its distance is that of the last of forms 0-2 it took (form 3 does not update it, as in the reference).
    selection        repeat: take the nearest remaining candidate (boundary rows and still-flagged points together; a boundary
                     row only if strictly nearer than the nearest point; first minimum on ties), emit its plane, unflag every
                     point with plane.q > -eps; until nothing remains.
    back             row (n, d) -> (n forward, d - (n forward).p)
"""
import numpy as np

try:
    import mpmath
    from mpmath import mpf
except ImportError:      # collection still works; every function below needs mpmath
    mpmath = mpf = None

DPS = 50
SCREEN = 1e-6            # a cut test whose float64 value is farther than this from its threshold is not repeated at DPS digits


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _vec(x):
    return [mpf(float(v)) for v in np.asarray(x, dtype=np.float64).reshape(-1)]


def planes(bd, pc, a, b, R, p, r, eps=1e-6):
    """One plane pass on the doubles given.  Returns a dict:
      rows      (K, 4) float64, the polytope rows in selection order (rounded once from DPS digits)
      kind      (K,) int: -1 boundary row, else the tangent form (0..3) of the point the row belongs to
      index     (K,) int: the boundary row or the point
      form      (N,) int: the tangent form every obstacle point took
      pt_margin (N,) float: the smallest |v - eps| over the (up to three) `> eps` tests of that point
      margins   dict of the smallest decision margins of the pass:
                  argmin_bd  relative gap (d2 - d1) / d2 between the selected distance and the runner-up, over the selections
                             whose winner and runner-up are both boundary rows
                  argmin_pt  the same over the selections where either is an obstacle point
                  tangent    min of pt_margin
                  cut        min |v + eps| over every cut test of a still-flagged point
                (inf where no such decision was taken)
    """
    with mpmath.workdps(DPS):
        return _planes(np.asarray(bd, dtype=np.float64), np.asarray(pc, dtype=np.float64).reshape(-1, 3), a, b, R, p, r, eps)


def _planes(bd, pc, a, b, R, p, r, eps):
    M, N = bd.shape[0], pc.shape[0]
    eps = mpf(float(eps))
    Rm = [_vec(row) for row in np.asarray(R, dtype=np.float64).reshape(3, 3)]
    p = _vec(p); r = _vec(r); a = _vec(a); b = _vec(b)
    fw = [[Rm[j][i] / r[i] for j in range(3)] for i in range(3)]          # diag(1/r) R'
    forward = lambda x: [_dot(fw[i], [x[0] - p[0], x[1] - p[1], x[2] - p[2]]) for i in range(3)]
    fa, fb = forward(a), forward(b)

    # boundary rows
    bdrow, bddist = [], []
    for h in bd:
        h = _vec(h)
        fB = [(h[0] * Rm[0][c] + h[1] * Rm[1][c] + h[2] * Rm[2][c]) * r[c] for c in range(3)]
        fD = h[3] + _dot(h, p)
        bdrow.append(fB + [fD])
        bddist.append(abs(fD) / mpmath.sqrt(_dot(fB, fB)))

    # obstacle points: forward image, tangent plane, distance, form
    fq, tang, dist = [], [], []
    form = np.zeros(N, dtype=np.int64)
    pt_margin = np.full(N, np.inf)
    for j in range(N):
        q = forward(_vec(pc[j]))
        d = mpmath.sqrt(_dot(q, q))
        t = [q[0] / d, q[1] / d, q[2] / d, -d]

        def test(f, j=j):
            v = _dot(t, f) + t[3]
            pt_margin[j] = min(pt_margin[j], float(abs(v - eps)))
            return v > eps

        def toward(f):
            dd = [q[0] - f[0], q[1] - f[1], q[2] - f[2]]
            s = _dot(dd, f) / _dot(dd, dd)
            n = [f[i] - s * dd[i] for i in range(3)]
            nd = mpmath.sqrt(_dot(n, n))
            return [n[0] / nd, n[1] / nd, n[2] / nd, -nd], nd
        if test(fa):
            t, d = toward(fa); form[j] = 1
        if test(fb):
            t, d = toward(fb); form[j] = 2
        if test(fa):
            u = [fa[i] - q[i] for i in range(3)]; v = [fb[i] - q[i] for i in range(3)]
            n = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
            nn = mpmath.sqrt(_dot(n, n))
            n = [n[0] / nn, n[1] / nn, n[2] / nn]
            off = -_dot(n, fa)
            sg = -1 if off > 0 else 1
            t = [sg * n[0], sg * n[1], sg * n[2], sg * off]; form[j] = 3
        fq.append(q); tang.append(t); dist.append(d)
    fqf = np.array([[float(c) for c in q] for q in fq], dtype=np.float64).reshape(N, 3)
    fqn = np.abs(fqf).sum(axis=1)

    bdF = [True] * M
    pcF = np.ones(N, dtype=bool)
    m_bd = m_pt = m_cut = mpf("inf")
    rows, kind, index = [], [], []
    inf = mpf("inf")
    step = 0
    while step < M + N:
        # the two smallest distances among what remains, boundary rows first (on an exact tie the earlier one is `first`;
        # between a boundary row and a point the point wins, as `minD < minR` says)
        cand = [(bddist[j], 1, j) for j in range(M) if bdF[j]] + [(dist[j], 0, j) for j in np.flatnonzero(pcF)]
        if not cand:
            break
        first = min(cand)            # ties: a point (0) before a boundary row (1), then the lower index
        if len(cand) > 1:
            second = min(c for c in cand if c is not first)
            gap = (second[0] - first[0]) / second[0] if second[0] > 0 else mpf(0)
            if first[1] == 1 and second[1] == 1:
                m_bd = min(m_bd, gap)
            else:
                m_pt = min(m_pt, gap)
        if first[1] == 1:
            row = bdrow[first[2]]; bdF[first[2]] = False
            kind.append(-1)
        else:
            row = tang[first[2]]; pcF[first[2]] = False
            kind.append(int(form[first[2]]))
        index.append(first[2])
        rows.append(row)
        # cut: float64 screens, DPS digits decide whatever is near the threshold
        live = np.flatnonzero(pcF)
        if len(live):
            rf = np.array([float(c) for c in row])
            vf = fqf[live] @ rf[:3] + rf[3]
            scale = np.maximum(1.0, fqn[live] * np.abs(rf[:3]).max() + abs(rf[3]))
            near = np.abs(vf + float(eps)) <= SCREEN * scale
            cut = vf > -float(eps)
            far = np.abs(vf + float(eps))[~near]
            if len(far):
                m_cut = min(m_cut, mpf(float(far.min())))
            for k in np.flatnonzero(near):
                v = _dot(row, fq[live[k]]) + row[3]
                m_cut = min(m_cut, abs(v + eps))
                cut[k] = bool(v > -eps)
            pcF[live[cut]] = False
        step += 1
    out = np.zeros((len(rows), 4))
    for k, row in enumerate(rows):
        h = [row[0] * fw[0][c] + row[1] * fw[1][c] + row[2] * fw[2][c] for c in range(3)]
        h.append(row[3] - _dot(h, p))
        out[k] = [float(c) for c in h]
    fl = lambda v: float(v) if v != inf else np.inf
    return dict(rows=out, kind=np.array(kind, dtype=np.int64), index=np.array(index, dtype=np.int64), form=form,
                pt_margin=pt_margin,
                margins=dict(argmin_bd=fl(m_bd), argmin_pt=fl(m_pt), tangent=float(pt_margin.min()) if N else np.inf,
                             cut=fl(m_cut)))


def ellipsoid_q(R, r):
    """Q = R diag(r^2) R' at DPS digits (an mpmath matrix)."""
    with mpmath.workdps(DPS):
        Rm = mpmath.matrix([[mpf(float(v)) for v in row] for row in np.asarray(R, dtype=np.float64).reshape(3, 3)])
        D = mpmath.diag([mpf(float(v)) ** 2 for v in r])
        return Rm * D * Rm.T


def factor_q(x, diag_eps=0.0):
    """Q = L L' of the optimiser's variables x = [p - c, rtd, cde] (firi.hpp:95-102): L = [[rtd0^2, 0, 0], [cde0, rtd1^2, 0],
    [cde2, cde1, rtd2^2]], with `diag_eps` added to the diagonal as costMVIE does with DBL_EPSILON."""
    with mpmath.workdps(DPS):
        x = _vec(x); e = mpf(float(diag_eps))
        L = mpmath.matrix([[x[3] ** 2 + e, 0, 0], [x[6], x[4] ** 2 + e, 0], [x[8], x[7], x[5] ** 2 + e]])
        return L * L.T


def normalised_rows(rows, c):
    """The rows of mvie_setup (firi.hpp:189-200) at DPS digits: unit normal n and offset b = -h3 / |h|, then a = n / (b - n.c)."""
    out = []
    for h in np.asarray(rows, dtype=np.float64):
        h = _vec(h)
        nrm = mpmath.sqrt(_dot(h, h))
        n = [h[0] / nrm, h[1] / nrm, h[2] / nrm]
        den = -h[3] / nrm - _dot(n, c)
        out.append([n[0] / den, n[1] / den, n[2] / den])
    return out


def cost_mvie(rows, c, Q, p, eps=1e-2, wt=1e3, parts=False):
    """costMVIE as a function of the ellipsoid {p + Q^(1/2) u}: wt * sum_i smoothedL1(sqrt(a_i' Q a_i) + a_i.(p - c) - 1)
    - 1/2 log det Q, rows a_i normalised about the interior point c.  rows (K, 4) raw polytope rows; c, p doubles or mpf;
    Q a 3x3 of doubles or an mpmath matrix.  Returns an mpf (parts=True: also the sum of the magnitudes of its terms)."""
    with mpmath.workdps(DPS):
        c = [mpf(v) if isinstance(v, mpf) else mpf(float(v)) for v in c]
        p = [mpf(v) if isinstance(v, mpf) else mpf(float(v)) for v in p]
        if not isinstance(Q, mpmath.matrix):
            Q = mpmath.matrix([[mpf(float(v)) for v in row] for row in np.asarray(Q, dtype=np.float64).reshape(3, 3)])
        mu = mpf(float(eps)); wt = mpf(float(wt))
        d = [p[0] - c[0], p[1] - c[1], p[2] - c[2]]
        pen = mpf(0)
        for a in normalised_rows(rows, c):
            Qa = [Q[i, 0] * a[0] + Q[i, 1] * a[1] + Q[i, 2] * a[2] for i in range(3)]
            x = mpmath.sqrt(_dot(a, Qa)) + _dot(a, d) - 1
            if x < 0:
                continue
            if x > mu:
                pen += x - mu / 2                                   # penalty_terms.h smoothed_l1: linear branch
            else:
                pen += (mu - x / 2) * (x / mu) ** 3                 # its cubic-quartic blend, C2 at 0 and at mu
        logdet = mpmath.log(mpmath.det(Q))
        f = wt * pen - logdet / 2
        return (f, wt * pen + abs(logdet) / 2) if parts else f


def chebyshev_centre(rows):
    """The deepest interior point of the polytope rows (K, 4), h.[x;1] <= 0, normals taken to unit length: HiGHS' vertex,
    polished at DPS digits by solving the four rows of least slack for (x, t).  Returns (c as three mpf, depth as mpf,
    nondegenerate): exactly four rows within 1e-9 of the depth and positive multipliers on all four, i.e. the optimum is unique
    and every exact method finds the same point."""
    from scipy.optimize import linprog
    h = np.asarray(rows, dtype=np.float64)
    nrm = np.linalg.norm(h[:, :3], axis=1)
    A = np.c_[h[:, :3] / nrm[:, None], np.ones(len(h))]
    res = linprog(c=[0, 0, 0, -1.0], A_ub=A, b_ub=-h[:, 3] / nrm, bounds=[(None, None)] * 4, method="highs")
    if res.status != 0:
        return None, None, False
    slack = -h[:, 3] / nrm - A @ res.x
    act = np.argsort(slack)[:4]
    with mpmath.workdps(DPS):
        G, rhs = [], []
        for i in act:
            hh = _vec(h[i]); n = mpmath.sqrt(_dot(hh, hh))
            G.append([hh[0] / n, hh[1] / n, hh[2] / n, mpf(1)]); rhs.append(-hh[3] / n)
        Gm = mpmath.matrix(G)
        try:
            v = mpmath.lu_solve(Gm, mpmath.matrix(rhs))
            lam = mpmath.lu_solve(Gm.T, mpmath.matrix([0, 0, 0, 1]))      # G' lam = objective
        except ZeroDivisionError:
            return None, None, False
        c = [v[0], v[1], v[2]]; t = v[3]
        tight = 0
        for hr in h:
            hh = _vec(hr); n = mpmath.sqrt(_dot(hh, hh))
            s = -hh[3] / n - _dot(hh, c) / n - t
            if s < mpf("-1e-30"):
                return c, t, False                                          # not the optimum: the four rows were not the active ones
            tight += s < mpf("1e-9")
        return c, t, bool(tight == 4 and all(lam[i] > mpf("1e-9") for i in range(4)))


def x_of_ellipsoid(R, p, r, c):
    """The optimiser's nine variables of the ellipsoid (R, p, r) about the interior point c (firi.hpp:202-206): the Cholesky
    factor of Q = R diag(r^2) R' with the square roots of its diagonal, in float64."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3); r = np.asarray(r, dtype=np.float64)
    L = np.linalg.cholesky(R @ np.diag(r * r) @ R.T)
    return np.r_[np.asarray(p, dtype=np.float64) - c, np.sqrt(np.diag(L)), L[1, 0], L[2, 1], L[2, 0]]


def score(rows, c, R, p, r):
    """cost_mvie of the ellipsoid (R, p, r) given as doubles."""
    return cost_mvie(rows, c, ellipsoid_q(R, r), p)


def f_star(rows, c, starts):
    """The minimum of costMVIE over all ellipsoids, for the polytope `rows` normalised about c: scipy's BFGS on the float64
    objective (oracle.cbind.cost_mvie) with gtol 1e-10 from every start in `starts` (nine variables each), every end point
    scored at DPS digits.  Returns (the smallest value, the spread of the values): a spread above 1e-9 means the optimiser did
    not pin the minimum down and the case cannot carry a 1e-9 statement."""
    from scipy.optimize import minimize
    from oracle import cbind
    cf = np.array([float(v) for v in c])
    with mpmath.workdps(DPS):
        A = np.array([[float(v) for v in a] for a in normalised_rows(rows, c)])
    vals = []
    for x0 in starts:
        res = minimize(lambda x: cbind.cost_mvie(A, 1e-2, 1e3, x), np.asarray(x0, dtype=np.float64), jac=True, method="BFGS",
                       options=dict(gtol=1e-10, maxiter=5000))
        vals.append(cost_mvie(rows, c, factor_q(res.x), [res.x[0] + cf[0], res.x[1] + cf[1], res.x[2] + cf[2]]))
    return min(vals), float(max(vals) - min(vals))


def match_rows(got, ref, bar, as_set=False):
    """The largest |got - ref| over the rows in units of the per-row bar `bar` (K,), rows paired in order or, as_set, each
    reference row with its nearest row of `got` (a permutation is required).  inf on a count mismatch."""
    got = np.asarray(got); ref = np.asarray(ref)
    if got.shape != ref.shape:
        return np.inf
    if not as_set:
        return float((np.abs(got - ref).max(axis=1) / bar).max())
    d = np.abs(got[None, :, :] - ref[:, None, :]).max(axis=2)            # [ref row, got row]
    pick = d.argmin(axis=1)
    if len(set(pick.tolist())) != len(ref):
        return np.inf
    return float((d[np.arange(len(ref)), pick] / bar).max())
