"""The multiprecision flatness reference (tests/flatness_mp.py) and its fixture, without a GPU: the reference against facts
that do not depend on it, a float64 restatement of the kernels' order of operations against the fixture's bounds on every
case (what the GPU tests ask of the kernels, so a bound that plain float64 cannot meet shows here first), and the
generator against the committed file."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import flatness_mp as fmp
from tests.golden.make_flatness_golden import locate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_mp = pytest.mark.skipif(fmp.mpmath is None, reason="mpmath is not installed")


@pytest.fixture(scope="module")
def fx():
    return fmp.load()


# ---- the reference against independent facts ----------------------------------------------------------------
def _fwd(v, a, j, psi=0.0, dpsi=0.0, par=fmp.LAUNCH):
    fmp._need_mp()
    return fmp.forward_mp(fmp._m(v) + fmp._m(a) + fmp._m(j) + [fmp.mpf(psi), fmp.mpf(dpsi)], fmp._m(par))


@needs_mp
def test_reference_hover():
    Y, mag, delta = _fwd([0, 0, 0], [0, 0, 0], [0.3, -2.0, 1.0])
    assert Y[0] == fmp.mpf(1.0) * fmp.mpf(9.8)                          # thr = m g, exactly
    assert Y[1:5] == [1, 0, 0, 0] and Y[11] == 0 and delta == 2          # no tilt
    Y2, _, _ = _fwd([0, 0, 0], [0, 0, 0], [0, 0, 0], psi=0.7, dpsi=-0.4)
    assert Y2[5:8] == [0, 0, fmp.mpf(-0.4)]                              # the yaw rate alone
    assert abs(Y2[1] - fmp.mpmath.cos(fmp.mpf(0.7) / 2)) < 1e-65 and abs(Y2[4] - fmp.mpmath.sin(fmp.mpf(0.7) / 2)) < 1e-65


@needs_mp
def test_reference_attitude_identities():
    rng = np.random.default_rng(7)
    for _ in range(20):
        v, a, j = rng.uniform(-4, 4, 3), rng.uniform(-12, 6, 3), rng.normal(size=3) * 5
        Y, _, delta = _fwd(v, a, j, rng.uniform(-3, 3), rng.normal())
        q, z = Y[1:5], Y[8:11]
        assert abs(sum(t * t for t in q) - 1) < 1e-60                    # |quat| = 1
        w, x, y, k = q
        Re3 = [2 * (x * k + w * y), 2 * (y * k - w * x), 1 - 2 * (x * x + y * y)]
        assert max(abs(r - t) for r, t in zip(Re3, z)) < 1e-60           # R(quat) e3 = z
        assert abs(Y[11] - fmp.mpmath.acos(z[2])) < 1e-30 and abs(delta - (1 + z[2])) < 1e-60
        # with dh = dv the force to produce is along z: the thrust is its norm
        par = (1.0, 9.8, 0.8, 0.8, 0.01, 1e-4)
        Ye, _, _ = _fwd(v, a, j, par=par)
        s = fmp.mpmath.sqrt(sum(fmp.mpf(float(t)) ** 2 for t in v) + fmp.mpf(1e-4))
        f = [fmp.mpf(float(a[k])) + fmp.mpf(0.8) * (1 + fmp.mpf(0.01) * s) * fmp.mpf(float(v[k])) for k in range(3)]
        f[2] += fmp.mpf(9.8)
        assert abs(Ye[0] - fmp.mpmath.sqrt(sum(t * t for t in f))) < 1e-60


@needs_mp
def test_reference_body_rate_is_the_quaternion_rate():
    """omg = 2 conj(q) dq/dt with dq/dt by central differences at working precision along a quintic piece with a quadratic
    yaw: the reference's omg comes out of its own dtilt/dt and dyaw/dt, this checks them against q(t) itself."""
    fmp._need_mp()
    rng = np.random.default_rng(11)
    h = fmp.mpf(10) ** -25
    for _ in range(6):
        cm = [fmp._m(r) for r in rng.uniform(-1, 1, (3, 6)) * np.array([0.1, 0.15, 0.25, 0.5, 1.0, 1.0])]
        yc = fmp._m(rng.normal(size=3))
        par = fmp._m(fmp.LAUNCH)

        def at(t):
            d, _ = fmp._derivs(cm, t, 3)
            return fmp.forward_mp(d[1] + d[2] + d[3] + [yc[0] + yc[1] * t + yc[2] * t * t, yc[1] + 2 * yc[2] * t], par)[0]
        t0 = fmp.mpf(float(rng.uniform(0.1, 0.9)))
        Y, qp, qm = at(t0), at(t0 + h)[1:5], at(t0 - h)[1:5]
        qd = [(p - m) / (2 * h) for p, m in zip(qp, qm)]
        q = Y[1:5]
        w = [2 * sum(t) for t in fmp._qmul_terms([q[0], -q[1], -q[2], -q[3]], qd)]
        assert abs(w[0]) < 1e-40                                         # a unit quaternion's rate is pure
        assert max(abs(w[k + 1] - Y[5 + k]) for k in range(3)) < 1e-40


@needs_mp
def test_reference_adjoint_is_the_gradient_of_the_pairing():
    """<g, Y(x + t e)> differentiated directly along a random direction e equals <J^T g, e>."""
    fmp._need_mp()
    rng = np.random.default_rng(13)
    x = fmp._m(np.r_[rng.uniform(-4, 4, 3), rng.uniform(-6, 6, 3), rng.normal(size=3) * 5, 0.9, -0.3])
    par, g, e = fmp._m(fmp.LAUNCH), fmp._m(rng.normal(size=8)), fmp._m(rng.normal(size=11))
    h = fmp.mpf(10) ** -25
    pair = lambda t: sum(gi * yi for gi, yi in zip(g, fmp.forward_mp([xi + t * ei for xi, ei in zip(x, e)], par)[0][:8]))
    gx, _ = fmp.adjoint_mp(x, par, g)
    assert abs((pair(h) - pair(-h)) / (2 * h) - sum(a * b for a, b in zip(gx, e))) < 1e-40


# ---- float64 in the kernels' order of operations (no FMA) ---------------------------------------------------
def _dot3(x, y):
    return x[..., 2] * y[..., 2] + (x[..., 1] * y[..., 1] + x[..., 0] * y[..., 0])


def forward_f64(par, v, a, j, psi, dpsi):
    """flat_forward, vectorised over the leading axis; returns the FlatMid fields as a dict"""
    mass, grav, dh, dv, cp, eps = par
    m = {}
    dhm = dh / mass
    m["s"] = np.sqrt(_dot3(v, v) + eps)
    m["wt"] = cp * m["s"] + 1.0
    m["w"] = m["wt"][:, None] * v
    zu = dhm * m["w"] + a
    zu[:, 2] += grav
    m["iL"] = 1.0 / np.sqrt(_dot3(zu, zu))
    m["z"] = zu * m["iL"][:, None]
    m["dwt"] = cp * _dot3(v, a) / m["s"]
    m["u"] = dhm * (m["wt"][:, None] * a + m["dwt"][:, None] * v) + j
    m["zu_dot"] = _dot3(m["z"], m["u"])
    m["dz"] = (-m["z"] * m["zu_dot"][:, None] + m["u"]) * m["iL"][:, None]
    m["f"] = mass * a + dv * m["w"]
    m["f"][:, 2] = mass * grav + m["f"][:, 2]
    m["thr"] = _dot3(m["z"], m["f"])
    z, dz = m["z"], m["dz"]
    m["den"] = np.sqrt(2.0 * (1.0 + z[:, 2]))
    t0, t1, t2 = 0.5 * m["den"], -z[:, 1] / m["den"], z[:, 0] / m["den"]
    m["ch"], m["sh"], m["cps"], m["sps"] = np.cos(0.5 * psi), np.sin(0.5 * psi), np.cos(psi), np.sin(psi)
    m["q"] = np.stack([t0 * m["ch"], t1 * m["ch"] + t2 * m["sh"], t2 * m["ch"] - t1 * m["sh"], t0 * m["sh"]], 1)
    m["iod"] = 1.0 / (1.0 + z[:, 2])
    m["ot"] = dz[:, 2] * m["iod"]
    A, Bv = z[:, 0] * m["sps"] - z[:, 1] * m["cps"], z[:, 0] * m["cps"] + z[:, 1] * m["sps"]
    m["o"] = np.stack([dz[:, 0] * m["sps"] - dz[:, 1] * m["cps"] - A * m["ot"], dz[:, 0] * m["cps"] + dz[:, 1] * m["sps"] - Bv * m["ot"],
                       (z[:, 1] * dz[:, 0] - z[:, 0] * dz[:, 1]) * m["iod"] + dpsi], 1)
    return m


def adjoint_f64(par, v, a, m, thr_b, qb, ob, yaw=True):
    """flat_adjoint -> vb, ab, jb (n, 3), psib, dpsib (n,)"""
    mass, grav, dh, dv, cp, eps = par
    dhm = dh / mass
    z, dz, o, q = m["z"], m["dz"], m["o"], m["q"]
    col = lambda x: x[:, None]
    dpsib = ob[:, 2]
    psib = ob[:, 0] * o[:, 1] - ob[:, 1] * o[:, 0]
    A, Bv = z[:, 0] * m["sps"] - z[:, 1] * m["cps"], z[:, 0] * m["cps"] + z[:, 1] * m["sps"]
    r0, r1 = ob[:, 0] * m["sps"] + ob[:, 1] * m["cps"], ob[:, 1] * m["sps"] - ob[:, 0] * m["cps"]
    cr = z[:, 1] * dz[:, 0] - z[:, 0] * dz[:, 1]
    otb = -(ob[:, 0] * A + ob[:, 1] * Bv)
    o2i = ob[:, 2] * m["iod"]
    dzb = np.stack([o2i * z[:, 1] + r0, -o2i * z[:, 0] + r1, otb * m["iod"]], 1)
    zb = np.stack([-(r0 * m["ot"]) - o2i * dz[:, 1], -(r1 * m["ot"]) + o2i * dz[:, 0],
                   -(o2i * cr + otb * dz[:, 2] * m["iod"]) * m["iod"]], 1)
    t1, t2 = -z[:, 1] / m["den"], z[:, 0] / m["den"]
    t0b, t1b, t2b = qb[:, 0] * m["ch"] + qb[:, 3] * m["sh"], qb[:, 1] * m["ch"] - qb[:, 2] * m["sh"], qb[:, 1] * m["sh"] + qb[:, 2] * m["ch"]
    if yaw:
        psib = psib + 0.5 * (qb[:, 1] * q[:, 2] - qb[:, 0] * q[:, 3] - qb[:, 2] * q[:, 1] + qb[:, 3] * q[:, 0])
    iden = 1.0 / m["den"]
    denb = 0.5 * t0b - (t1b * t1 + t2b * t2) * iden
    zb = zb + np.stack([t2b * iden, -t1b * iden, denb * iden], 1)
    zb = col(thr_b) * m["f"] + zb
    fb = col(thr_b) * z
    rb = dzb * col(m["iL"])
    r = -z * col(m["zu_dot"]) + m["u"]
    iLb, rbz = _dot3(dzb, r), _dot3(rb, z)
    ub = -z * col(rbz) + rb
    zb = zb - (rb * col(m["zu_dot"]) + m["u"] * col(rbz))
    zbz = _dot3(zb, z)
    zub = col(m["iL"]) * ((-z * col(zbz) + zb) - col(iLb * m["iL"]) * z)
    jb, dwb = ub, dhm * ub
    wb = dv * fb + dhm * zub
    ab = mass * fb + zub
    wtb = _dot3(dwb, a)
    dwtb = _dot3(dwb, v)
    vab = dwtb * cp / m["s"]
    sb = -dwtb * m["dwt"] / m["s"]
    wtb = wtb + _dot3(wb, v)
    sb = cp * wtb + sb
    sbs = sb / m["s"]
    ab = col(m["wt"]) * dwb + (col(vab) * v + ab)
    vb = col(m["dwt"]) * dwb + (col(vab) * a + (col(m["wt"]) * wb + col(sbs) * v))
    return vb, ab, jb, psib, dpsib


def tilt_f64(q):
    return 2.0 * np.arctan2(np.sqrt(q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]), np.sqrt(q[:, 0] * q[:, 0] + q[:, 3] * q[:, 3]))


def _sl1(mu, inv_mu, x):
    xd = x * inv_mu
    sq, mm = xd * xd, -0.5 * x + mu
    fm, dm = mm * sq * xd, sq * (-0.5 * xd + 3.0 * mm * inv_mu)
    if x < 0.0:
        return 0.0, 0.0
    return (x - 0.5 * mu, 1.0) if x > mu else (fm, dm)


def _fall(k, d):
    r = 1.0
    for i in range(d):
        r *= (k - i)
    return r


def piece_f64(cm, T, par, pen):
    """k_flat_piece_grad for one piece -> pc, gC (3, D), gT"""
    w_thr, w_tilt, w_bdr, mu, thr_min, thr_max, tilt_max, bdr_max, res = pen
    res = int(res)
    cos_max, b2_max = math.cos(tilt_max), bdr_max * bdr_max
    D = cm.shape[1]
    pw = np.ones(D)
    for k in range(1, D):
        pw[D - 1 - k] = pw[D - k] * T
    ct = cm * pw
    gN = np.zeros((3, D))
    inv_mu, inv_res = 1.0 / mu, 1.0 / res
    rT = 1.0 / T
    rT2 = rT * rT
    rT3, rT4 = rT2 * rT, rT2 * rT2
    csum = gts = 0.0
    for jj in range(res):
        tau = jj * inv_res
        tb = np.array([[_fall(D - 1 - col, d) * tau ** (D - 1 - col - d) if D - 1 - col >= d else 0.0 for col in range(D)]
                       for d in range(5)])
        x = ct @ tb[1:].T                                                # (3, 4): v, a, j, snap in normalised time
        v, ac, jr, sn = x[:, 0] * rT, x[:, 1] * rT2, x[:, 2] * rT3, x[:, 3] * rT4
        m = forward_f64(par, v[None], ac[None], jr[None], np.zeros(1), np.zeros(1))
        thr, q, o = m["thr"][0], m["q"][0], m["o"][0]
        f, df = _sl1(mu, inv_mu, thr - thr_max)
        phi, thr_b = w_thr * f, w_thr * df
        f, df = _sl1(mu, inv_mu, thr_min - thr)
        phi, thr_b = w_thr * f + phi, -w_thr * df + thr_b
        q12 = q[1] * q[1] + q[2] * q[2]
        f, df = _sl1(mu, inv_mu, cos_max - (1.0 - 2.0 * q12))
        phi = w_tilt * f + phi
        qb = np.array([0.0, 4.0 * w_tilt * df * q[1], 4.0 * w_tilt * df * q[2], 0.0])
        f, df = _sl1(mu, inv_mu, float(_dot3(o, o)) - b2_max)
        phi = w_bdr * f + phi
        ob = 2.0 * w_bdr * df * o
        csum += phi
        if phi > 0.0:
            vb, ab, jb, _, _ = adjoint_f64(par, v[None], ac[None], m, np.array([thr_b]), qb[None], ob[None], yaw=False)
            vb, ab, jb = vb[0], ab[0], jb[0]
            gts = tau * (float(_dot3(vb, ac)) + float(_dot3(ab, jr)) + float(_dot3(jb, sn))) + gts
            gN += np.outer(vb * rT, tb[1]) + np.outer(ab * rT2, tb[2]) + np.outer(jb * rT3, tb[3])
    step = T * inv_res
    return step * csum, gN * (step * pw), step * gts + csum * inv_res


def states_f64(cm, t, par):
    """k_traj_flat_states' 11 fields at local time t of one piece (ascending powers, tn *= t)"""
    D = cm.shape[1]
    d = np.zeros((3, 3))
    for q in range(3):
        tn = 1.0
        for k in range(q + 1, D):
            d[q] += _fall(k, q + 1) * tn * cm[:, D - 1 - k]
            tn *= t
    m = forward_f64(par, d[0][None], d[1][None], d[2][None], np.zeros(1), np.zeros(1))
    return np.r_[m["thr"], m["q"][0], m["o"][0], np.sqrt(_dot3(d[0], d[0])), tilt_f64(m["q"]), np.sqrt(_dot3(m["o"][0], m["o"][0]))]


def extrema_f64(cms, T, par, res):
    """k_traj_flat_extrema for one trajectory: samples j T_i / res, j = 0..res; the tilt from the largest q1^2 + q2^2 and the
    smallest q0^2 + q3^2"""
    lo, hi, s2, c2, b2 = np.inf, -np.inf, 0.0, np.inf, 0.0
    inv_res = 1.0 / res
    for cm, Ti in zip(cms, T):
        for jj in range(res + 1):
            st = states_f64(cm, jj * Ti * inv_res, par)
            lo, hi, b2 = min(lo, st[0]), max(hi, st[0]), max(b2, float(_dot3(st[5:8], st[5:8])))
            s2, c2 = max(s2, st[2] * st[2] + st[3] * st[3]), min(c2, st[1] * st[1] + st[4] * st[4])
    return np.array([lo, hi, 2.0 * math.atan2(math.sqrt(s2), math.sqrt(c2)), math.sqrt(b2)])


def _by_family(fams, ratios, what, bar=1.0):
    worst = {}
    for f, r in zip(fams, ratios):
        worst[f] = max(worst.get(f, 0.0), float(r))
    print(what + ": " + ", ".join(f"{f} {r:.3g}" for f, r in worst.items()))
    assert max(worst.values()) <= bar, (what, worst)
    return worst


def test_float64_forward_and_adjoint_meet_the_bounds(fx):
    n = len(fx["pt_delta"])
    rf, ra = np.zeros(n), np.zeros(n)
    for veh in np.unique(fx["pt_veh"]):
        k = np.flatnonzero(fx["pt_veh"] == veh)
        par = fx["vehicles"][veh]
        v, a, j, g = fx["pt_v"][k], fx["pt_a"][k], fx["pt_j"][k], fx["pt_g"][k]
        m = forward_f64(par, v, a, j, fx["pt_psi"][k], fx["pt_dpsi"][k])
        got = np.c_[m["thr"], m["q"], m["o"]]
        vb, ab, jb, pb, db = adjoint_f64(par, v, a, m, g[:, 0], g[:, 1:5], g[:, 5:8])
        gad = np.c_[vb, ab, jb, pb, db]
        for r, i in enumerate(k):
            rf[i] = fmp.spare(got[r], fx["pt_fwd"][i], fx["pt_fwd_scale"][i], fx["pt_delta"][i], fmp.K_FWD)
            ra[i] = fmp.spare(gad[r], fx["pt_adj"][i], fx["pt_adj_scale"][i], fx["pt_delta"][i], fmp.K_ADJ)
    _by_family(fx["pt_family"], rf, "forward, error / bound")
    _by_family(fx["pt_family"], ra, "adjoint, error / bound")
    hov = np.flatnonzero((fx["pt_family"] == "hover") & (np.abs(fx["pt_v"]).sum(1) == 0.0) & ~fx["pt_yaw"])
    assert len(hov) == 1 and fx["pt_fwd"][hov[0], 0] == 9.8 and (fx["pt_fwd"][hov[0], 1:5] == [1.0, 0.0, 0.0, 0.0]).all()


def test_float64_piece_sums_meet_the_bounds(fx):
    r = []
    for i in range(len(fx["pn_pc"])):
        s = int(fx["pn_s"][i])
        p = fx["pn_piece"][i]
        pc, gC, gT = piece_f64(fx["pc_cm"][p][:, 8 - 2 * s:], fx["pc_T"][p], fmp.LAUNCH, fx["pn_pen"][i])
        dl = fx["pn_delta"][i]
        r.append(max(fmp.spare(pc, fx["pn_pc"][i], fx["pn_pc_scale"][i], dl, fmp.K_PIECE),
                     fmp.spare(gC, fx["pn_gC"][i][:, 8 - 2 * s:], fx["pn_gC_scale"][i][:, 8 - 2 * s:], dl, fmp.K_PIECE),
                     fmp.spare(gT, fx["pn_gT"][i], fx["pn_gT_scale"][i], dl, fmp.K_PIECE)))
    _by_family(fx["pn_family"], r, "piece penalty, error / bound")


def test_float64_states_and_extrema_meet_the_bounds(fx):
    r, fam = [], []
    for i in range(len(fx["tr_s"])):
        for s in ((3, 4) if fx["tr_s"][i] == 0 else (int(fx["tr_s"][i]),)):
            T = fx["pc_T"][fx["tr_piece"][i]]
            for k, t in enumerate(fx["tr_tq"][i]):
                idx, tl = locate(T, t)
                got = states_f64(fx["pc_cm"][fx["tr_piece"][i][idx]][:, 8 - 2 * s:], tl, fmp.LAUNCH)
                r.append(fmp.spare(got, fx["tr_state"][i, k], fx["tr_state_scale"][i, k], fx["tr_state_delta"][i, k], fmp.K_TRAJ))
                fam.append(str(fx["tr_family"][i]))
    _by_family(fam, r, "trajectory states, error / bound")
    r, fam = [], []
    for i in range(len(fx["tr_s"])):
        for s in ((3, 4) if fx["tr_s"][i] == 0 else (int(fx["tr_s"][i]),)):
            p = fx["tr_piece"][i]
            got = extrema_f64(fx["pc_cm"][p][..., 8 - 2 * s:], fx["pc_T"][p], fmp.LAUNCH, 4)
            r.append(fmp.spare(got, fx["tr_ext"][i], fx["tr_ext_scale"][i], fx["tr_ext_delta"][i], fmp.K_TRAJ))
            fam.append(str(fx["tr_family"][i]))
    _by_family(fam, r, "trajectory extrema, error / bound")


def test_the_old_tilt_expression_misses_the_bound(fx):
    """acos(1 - 2 (q1^2 + q2^2)) in float64 on the small-tilt trajectories: the factor over the bound, printed, is the defect
    the kernels had; it must be a failure, or the fixture would not have caught it."""
    worst = 0.0
    for i in np.flatnonzero(fx["tr_family"] == "smalltilt"):
        T = fx["pc_T"][fx["tr_piece"][i]]
        for k, t in enumerate(fx["tr_tq"][i]):
            idx, tl = locate(T, t)
            got = states_f64(fx["pc_cm"][fx["tr_piece"][i][idx]][:, 2:], tl, fmp.LAUNCH)
            old = math.acos(1.0 - 2.0 * (got[2] ** 2 + got[3] ** 2))
            worst = max(worst, fmp.spare(old, fx["tr_state"][i, k, 9], fx["tr_state_scale"][i, k, 9], fx["tr_state_delta"][i, k], fmp.K_TRAJ))
    print(f"old tilt expression on smalltilt: error / bound {worst:.3g}")
    assert worst > 1.0


def test_fixture_shape(fx):
    fam, cnt = np.unique(fx["pt_family"], return_counts=True)
    assert set(fam) == {"box", "hover", "smalltilt", "fast", "slow", "freefall", "tilted", "drag"} and (cnt == 16).all()
    assert (fx["pt_yaw"].sum(), len(fx["pn_pc"]), len(fx["tr_s"])) == (64, 60, 17)
    assert 0.0 < fx["pt_delta"].min() < 1.01e-3 and fx["tr_ext_delta"].min() < 1.01e-3
    assert os.path.getsize(fmp.FIXTURE) < 100_000
    for k, v in fx.items():
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), k


@needs_mp
def test_generator_reproduces_the_fixture():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_flatness_golden.py"), "--check", "--procs", "8"],
                         capture_output=True, text=True, timeout=1200)
    assert res.returncode == 0, res.stdout + res.stderr
