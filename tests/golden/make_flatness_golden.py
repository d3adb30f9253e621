#!/usr/bin/env python3
"""Generate tests/golden/flatness_cases.npz: hard inputs for the five flatness kernels with references from the
multiprecision restatement tests/flatness_mp.py (mpmath, 70 digits), each rounded once to double, and the condition-aware
scales of the bound (stored as float32, rounded up).  Deterministic: running it again reproduces the committed file byte
for byte.  It takes a few minutes on 8 processes.

    python tests/golden/make_flatness_golden.py [--check] [--procs N]

POINTWISE (keys pt_*): 16 cases per family, 8 with a yaw (the first three psi = 0, pi, -pi, the others uniform in (-pi, pi))
and 8 with psi = dpsi = None (stored as 0, pt_yaw False).  pt_veh indexes `vehicles` (mass, grav, dh, dv, cp, eps); pt_g are
the upstream gradients of (thr, q0..q3, o0..o2); pt_fwd the 8 outputs in that order, pt_adj the 11 gradients w.r.t.
(v, a, j, psi, dpsi); pt_fwd_scale, pt_adj_scale, pt_delta as flatness_mp defines them.
  box       |v| <= 4, |a| <= 6 per axis, j ~ 5 N(0, 1): the planner's boxes.
  hover     |v|, |a| ~ 1e-6; the last case of each half has v = a = 0 exactly and j != 0 (thr = m g, tilt quaternion
            (1, 0, 0, 0): exact).
  smalltilt zu = L (th cos f, th sin f, 1), th in {1e-2, 1e-4, 1e-6, 1e-8}; every other case has v = 0, so that the small
            horizontal acceleration is an input and not a difference of two large ones.
  fast      |v| in [5, 30].
  slow      |v|^2 from 1e-2 to 1e2 times the speed smoothing eps.
  freefall  |zu| in {1, 0.1, 1e-2, 1e-4}, z3 >= -0.5.
  tilted    delta = 1 + z3 in {0.5, 0.1, 0.01, 1e-3}.
  drag      box states on a vehicle with dh = dv and on one with cp = 0.

PIECES (piece table pc_cm (3 x 8, column col holds the power 7 - col: use pc_cm[:, :, 8 - 2 s:]), pc_T; cases pn_*).  Per order
s in {3, 4} one rest-to-rest solve of three pieces, durations scaled until |v| <= 3.8, |a| <= 5.7 on 40 samples (as the GPU
tests' scale_into_limits), coefficients rounded to multiples of 2^-24 (so the linear solver's last bits do not enter the
fixture; the first piece then starts at exact hover).  The limits belong to a launch, not to a piece, so they are chosen
per group (s, res), res in {1, 4}, from the reference's own sample values of the group's two LOUD pieces (the solve's
second and third piece):
  none    no row is active at any sample of the loud pieces and the quiet piece.
  linear  every one of the four rows is in the linear zone x > mu at some loud sample.
  cubic   every row has a loud sample in the cubic zone 0 < x < mu.
and every piece of the group has a reference under every one of the three sets.  Next to the loud pieces a group holds a
QUIET piece (vertical acceleration only, thrust between the limits: no row active under any set, so that a launch can hold
whole waves without an active row) and, for res = 4, the second piece with T in {0.05, 1, 20} and the solve's first piece
(first sample: exact hover).  pn_piece indexes the table, pn_pen is the API's penalty (w_thr, w_tilt, w_bdr, mu, thr_min,
thr_max, tilt_max, bdr_max, res), pn_group numbers the launches (s, res, limit set).

TRAJECTORIES (keys tr_*): three table pieces each (tr_piece), tr_s = 0 where the pieces have degree <= 3 and serve both
orders.  Per order 12: four of constant small tilt (th as above), one at exact hover, two through tilted states
(delta as above, T = 0.05), five of solve pieces.  tr_tq: 0, the first knot, the end, beyond the end, five interior
times; tr_state (9 x 11) in the order of k_traj_flat_states; tr_ext (4): min and max thrust, max tilt, max body rate over
the closed sample set j T_i / 4, j = 0..4, with the largest scale and the smallest delta over the samples.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import flatness_mp as fmp  # noqa: E402
from tests.golden.make_max_rate_golden import npz_bytes  # noqa: E402
from oracle import minco_np  # noqa: E402

OUT = fmp.FIXTURE
VEHICLES = np.array([fmp.LAUNCH, (1.0, 9.8, 0.8, 0.8, 0.01, 1e-4), (1.3, 9.81, 0.7, 0.8, 0.0, 1e-4)])
FAMILIES = ("box", "hover", "smalltilt", "fast", "slow", "freefall", "tilted", "drag")
PER_HALF = 8
WEIGHTS = (30.0, 200.0, 10.0)
STATE_FIELDS = [0, 1, 2, 3, 4, 5, 6, 7, 12, 11, 13]     # thr, q, omg, speed, tilt, body rate out of flatness_mp.OUT_NAMES
EXT_RES = 4


def f32_up(x):
    """float32 not below x (zero stays zero)."""
    x = np.asarray(x, dtype=np.float64)
    y = x.astype(np.float32)
    low = y.astype(np.float64) < x
    y[low] = np.nextafter(y[low], np.float32(np.inf))
    return y


def _unit(rng):
    d = rng.standard_normal(3)
    return d / np.linalg.norm(d)


def _acc_for(zu, v, par):
    """the acceleration that gives the thrust direction zu at velocity v (in double: the reference takes what comes out)"""
    mass, grav, dh, dv, cp, eps = par
    w = (1.0 + cp * math.sqrt(float(v @ v) + eps)) * v
    return zu - (dh / mass) * w - np.array([0.0, 0.0, grav])


def _tilted_zu(rng, delta):
    z3, f, L = delta - 1.0, rng.uniform(-math.pi, math.pi), rng.uniform(5.0, 15.0)
    r = math.sqrt(1.0 - z3 * z3)
    return L * np.array([r * math.cos(f), r * math.sin(f), z3])


def pointwise_cases():
    rng = np.random.default_rng(20250117)
    out = []
    for fam in FAMILIES:
        for yaw in (True, False):
            for i in range(PER_HALF):
                veh = 0
                v, a, j = rng.uniform(-4.0, 4.0, 3), rng.uniform(-6.0, 6.0, 3), rng.standard_normal(3) * 5.0
                if fam == "hover":
                    v, a = rng.standard_normal(3) * 1e-6, rng.standard_normal(3) * 1e-6
                    if i == PER_HALF - 1:
                        v, a = np.zeros(3), np.zeros(3)
                elif fam == "smalltilt":
                    th, f, L = 10.0 ** (-2 * (i % 4 + 1)), rng.uniform(-math.pi, math.pi), rng.uniform(5.0, 15.0)
                    if i >= 4:
                        v = np.zeros(3)
                    a = _acc_for(L * np.array([th * math.cos(f), th * math.sin(f), 1.0]), v, VEHICLES[0])
                elif fam == "fast":
                    v = _unit(rng) * rng.uniform(5.0, 30.0)
                elif fam == "slow":
                    v = _unit(rng) * math.sqrt(1e-4 * 10.0 ** (-2.0 + 4.0 * i / (PER_HALF - 1)))
                elif fam == "freefall":
                    d = _unit(rng)
                    while d[2] < -0.5:
                        d = _unit(rng)
                    a = _acc_for((1.0, 0.1, 1e-2, 1e-4)[i % 4] * d, v, VEHICLES[0])
                elif fam == "tilted":
                    a = _acc_for(_tilted_zu(rng, (0.5, 0.1, 0.01, 1e-3)[i % 4]), v, VEHICLES[0])
                elif fam == "drag":
                    veh = 1 + i % 2
                psi = (0.0, math.pi, -math.pi)[i] if i < 3 else rng.uniform(-math.pi, math.pi)
                dpsi = rng.standard_normal()
                g = rng.integers(-16, 17, 8) / 8.0
                out.append((fam, yaw, veh, v, a, j, psi if yaw else 0.0, dpsi if yaw else 0.0, g))
    return out


def pointwise_ref(c):
    fam, yaw, veh, v, a, j, psi, dpsi, g = c
    return fmp.pointwise_mp(v, a, j, psi, dpsi, VEHICLES[veh], g)


# ---- pieces -------------------------------------------------------------------------------------------------
def _rest_to_rest(s, seed):
    """three pieces, (3, 8) right-aligned, and their durations"""
    rng = np.random.default_rng(seed)
    d = np.stack([_unit(rng) for _ in range(3)]) * rng.uniform(1.0, 3.0, (3, 1))
    pts = np.concatenate([np.zeros((1, 3)), np.cumsum(d, 0)])
    head, tail = np.zeros((3, 3)), np.zeros((3, 3))
    head[:, 0], tail[:, 0] = pts[0], pts[3]
    T = rng.uniform(0.5, 2.0, 3)
    for _ in range(60):
        co = minco_np.minco_dense_solve(s, head, tail, pts[1:3].T, T)[0]
        vmax = amax = 0.0
        for i in range(3):
            t = np.linspace(0.0, T[i], 41)
            for ax in range(3):
                vmax = max(vmax, np.abs(np.polyval(np.polyder(co[i, ax], 1), t)).max())
                amax = max(amax, np.abs(np.polyval(np.polyder(co[i, ax], 2), t)).max())
        if vmax <= 3.8 and amax <= 5.7:
            break
        T = T * 1.15
    else:
        raise RuntimeError("could not scale the trajectory into the boxes")
    T = np.round(T * 2.0 ** 20) / 2.0 ** 20
    cm = np.zeros((3, 3, 8))
    cm[:, :, 8 - 2 * s:] = np.round(co * 2.0 ** 24) / 2.0 ** 24
    return cm, T


def _samples(job):
    cm, T, s, res = job
    pen = WEIGHTS + (1.0, 0.0, 1.0, 1.0, 1.0, res)
    return fmp.piece_penalty_mp(cm[:, 8 - 2 * s:], T, fmp.LAUNCH, pen, scales=False)["samples"]


def _piece_ref(job):
    cm, T, s, pen = job
    return fmp.piece_penalty_mp(cm[:, 8 - 2 * s:], T, fmp.LAUNCH, pen)


def _state_piece(v, a, j):
    cm = np.zeros((3, 8))
    cm[:, 6], cm[:, 5], cm[:, 4] = v, a / 2.0, j / 6.0
    return cm


def piece_table_and_cases(pool):
    """-> table [(cm, T)], named indices, cases [(family, s, res, group, piece, pen)] (without references)"""
    table, names, groups = [], {}, []

    def add(name, cm, T):
        names[name] = len(table)
        table.append((np.asarray(cm, dtype=np.float64), float(T)))
        return names[name]

    for s in (3, 4):
        cm, T = _rest_to_rest(s, 700 + s)
        for i, nm in enumerate(("first", "p1", "p2")):
            add(f"s{s}_{nm}", cm[i], T[i])
        for Tv in (0.05, 1.0, 20.0):
            add(f"s{s}_p1_T{Tv:g}", cm[1], Tv)
    for s in (3, 4):
        for res in (1, 4):
            loud = [names[f"s{s}_p1"], names[f"s{s}_p2"]]
            extra = [names[f"s{s}_p1_T{Tv:g}"] for Tv in (0.05, 1.0, 20.0)] + [names[f"s{s}_first"]] if res == 4 else []
            groups.append((s, res, loud, extra))
    jobs = [(table[p][0], table[p][1], s, res) for (s, res, loud, extra) in groups for p in loud + extra]
    smp = iter(pool.map(_samples, jobs))
    cases = []
    for gi, (s, res, loud, extra) in enumerate(groups):
        vals = [next(smp) for _ in loud + extra]
        lv = np.concatenate(vals[:len(loud)])                    # (samples, 3): thr, cos tilt, |omg|^2 of the loud pieces
        av = np.concatenate(vals)
        thr_lo, thr_hi, cos_lo, b2_hi = lv[:, 0].min(), lv[:, 0].max(), lv[:, 1].min(), lv[:, 2].max()
        mu = min(0.01, 0.1 * b2_hi, 0.3 * (1.0 - cos_lo), 0.1 * (thr_hi - thr_lo))
        assert mu > 0.0, (s, res, mu)
        mid = 0.5 * (thr_lo + thr_hi)
        quiet = np.zeros((3, 8))
        quiet[2, 5] = 0.5 * (mid / fmp.LAUNCH[0] - fmp.LAUNCH[1])
        q = add(f"s{s}_r{res}_quiet", quiet, 2.0 ** -10)
        sets = {"none": (av[:, 0].min() - 1.0, av[:, 0].max() + 1.0, max(av[:, 1].min() - 0.1, -0.999), av[:, 2].max() + 1.0),
                "linear": (thr_lo + 2.5 * mu, thr_hi - 2.5 * mu, cos_lo + 2.5 * mu, b2_hi - 2.5 * mu),
                "cubic": (thr_lo + 0.5 * mu, thr_hi - 0.5 * mu, cos_lo + 0.5 * mu, b2_hi - 0.5 * mu)}
        for li, (lname, (tmin, tmax, cmax, b2max)) in enumerate(sets.items()):
            pen = WEIGHTS + (mu, tmin, tmax, math.acos(cmax), math.sqrt(b2max), res)
            # the zones, from the reference's sample values and the limits the kernel will hold
            x = np.stack([lv[:, 0] - tmax, tmin - lv[:, 0], math.cos(pen[6]) - lv[:, 1], lv[:, 2] - pen[7] ** 2], 1)
            if lname == "none":
                assert (x < -0.05).all(), (s, res, x.max())
            elif lname == "linear":
                assert ((x > 2.0 * mu).any(0)).all(), (s, res, x / mu)
            else:
                assert (((x > 0.2 * mu) & (x < 0.8 * mu)).any(0)).all(), (s, res, x / mu)
            for p in loud + extra + [q]:
                kind = "loud" if p in loud else "quiet" if p == q else [k for k, v in names.items() if v == p][0][3:]
                cases.append((f"{lname}/{kind}", s, res, 3 * gi + li, p, pen))
    return table, names, cases


# ---- trajectories -------------------------------------------------------------------------------------------
def traj_cases(table, names):
    rng = np.random.default_rng(20250118)
    out = []

    def add(name, cm, T):
        names[name] = len(table)
        table.append((np.asarray(cm, dtype=np.float64), float(T)))
        return names[name]

    def finish(fam, s, pcs):
        T = np.array([table[p][1] for p in pcs])
        tot = T.sum()
        tq = np.r_[0.0, T[0], tot, tot + 0.3, rng.uniform(0.0, 1.0, 5) * tot]
        out.append((fam, s, pcs, tq))

    g = fmp.LAUNCH[1]
    for ti, th in enumerate((1e-2, 1e-4, 1e-6, 1e-8)):
        pcs = []
        for k in range(3):
            f = rng.uniform(-math.pi, math.pi)
            a = np.array([g * th * math.cos(f), g * th * math.sin(f), rng.uniform(-1.0, 1.0)])
            pcs.append(add(f"hold{ti}_{k}", _state_piece(np.zeros(3), a, np.zeros(3)), rng.uniform(0.3, 1.0)))
        finish("smalltilt", 0, pcs)
    finish("hover", 0, [add(f"rest_{k}", np.zeros((3, 8)), rng.uniform(0.3, 1.0)) for k in range(3)])
    for ti, deltas in enumerate(((0.5, 0.1, 0.01), (1e-3, 0.1, 0.5))):
        pcs = []
        for k, dl in enumerate(deltas):
            v, j = rng.uniform(-4.0, 4.0, 3), rng.standard_normal(3) * 5.0
            pcs.append(add(f"tilted{ti}_{k}", _state_piece(v, _acc_for(_tilted_zu(rng, dl), v, fmp.LAUNCH), j), 0.05))
        finish("tilted", 0, pcs)
    for s in (3, 4):
        n = lambda k: names[f"s{s}_{k}"]
        for pcs in ([n("first"), n("p1"), n("p2")], [n("p1"), n("p2"), n("r4_quiet")], [n("p1_T0.05"), n("p1_T1"), n("p2")],
                    [n("p2"), n("p1_T20"), n("first")], [n("p1"), n("first"), n("p1_T0.05")]):
            finish("solve", s, pcs)
    return out


def locate(T, t):
    """Trajectory::locatePieceIdx in the double arithmetic it is written in (part of the modelled behaviour)."""
    N, t, idx = len(T), float(t), 0
    while idx < N and t > float(T[idx]):
        t -= float(T[idx])
        idx += 1
    if idx == N:
        idx -= 1
        t += float(T[idx])
    return idx, t


def _traj_ref(job):
    """states at the queries and extrema over the closed sample set"""
    import mpmath
    cms, T, tq = job
    st, ss, sd = [], [], []
    for t in tq:
        idx, tl = locate(T, t)
        Y, sc, dl = fmp.state_mp(cms[idx], tl, fmp.LAUNCH)
        st.append(Y[STATE_FIELDS]); ss.append(sc[STATE_FIELDS]); sd.append(dl)
    fmp._need_mp()
    Ys, Ss, Ds = [], [], []
    for i in range(len(T)):
        for j in range(EXT_RES + 1):
            # the exact sample time j T / res, handed over at working precision
            Y, sc, dl = fmp.state_mp(cms[i], mpmath.mpf(j) * mpmath.mpf(float(T[i])) / EXT_RES, fmp.LAUNCH)
            Ys.append(Y); Ss.append(sc); Ds.append(dl)
    Ys, Ss = np.array(Ys), np.array(Ss)
    ext = np.array([Ys[:, 0].min(), Ys[:, 0].max(), Ys[:, 11].max(), Ys[:, 13].max()])
    esc = np.array([Ss[:, 0].max(), Ss[:, 0].max(), Ss[:, 11].max(), Ss[:, 13].max()])
    return np.array(st), np.array(ss), np.array(sd), ext, esc, min(Ds)


def generate(procs=8):
    import multiprocessing as mp
    with mp.Pool(procs) as pool:
        pts = pointwise_cases()
        prefs = pool.map(pointwise_ref, pts, chunksize=2)
        table, names, pcs = piece_table_and_cases(pool)
        crefs = pool.map(_piece_ref, [(table[p][0], table[p][1], s, pen) for (_, s, _, _, p, pen) in pcs], chunksize=1)
        trs = traj_cases(table, names)
        trefs = pool.map(_traj_ref, [([table[p][0] for p in pc], np.array([table[p][1] for p in pc]), tq)
                                     for (_, _, pc, tq) in trs], chunksize=1)
    col = lambda rs, k: np.array([r[k] for r in rs])
    data = dict(
        vehicles=VEHICLES,
        pt_family=np.array([c[0] for c in pts]), pt_yaw=np.array([c[1] for c in pts]),
        pt_veh=np.array([c[2] for c in pts], dtype=np.int8), pt_v=col(pts, 3), pt_a=col(pts, 4), pt_j=col(pts, 5),
        pt_psi=col(pts, 6), pt_dpsi=col(pts, 7), pt_g=col(pts, 8),
        pt_fwd=col(prefs, "fwd")[:, :fmp.N_MAP], pt_fwd_scale=f32_up(col(prefs, "fwd_scale")[:, :fmp.N_MAP]),
        pt_adj=col(prefs, "adj"), pt_adj_scale=f32_up(col(prefs, "adj_scale")), pt_delta=col(prefs, "delta"),
        pc_cm=np.array([t[0] for t in table]), pc_T=np.array([t[1] for t in table]),
        pn_family=np.array([c[0] for c in pcs]), pn_s=np.array([c[1] for c in pcs], dtype=np.int8),
        pn_res=np.array([c[2] for c in pcs], dtype=np.int8), pn_group=np.array([c[3] for c in pcs], dtype=np.int8),
        pn_piece=np.array([c[4] for c in pcs], dtype=np.int16), pn_pen=np.array([c[5] for c in pcs], dtype=np.float64),
        pn_pc=col(crefs, "pc"), pn_gT=col(crefs, "gT"), pn_delta=col(crefs, "delta"),
        pn_pc_scale=f32_up(col(crefs, "pc_scale")), pn_gT_scale=f32_up(col(crefs, "gT_scale")),
        tr_family=np.array([c[0] for c in trs]), tr_s=np.array([c[1] for c in trs], dtype=np.int8),
        tr_piece=np.array([c[2] for c in trs], dtype=np.int16), tr_tq=col(trs, 3),
        tr_state=col(trefs, 0), tr_state_scale=f32_up(col(trefs, 1)), tr_state_delta=col(trefs, 2),
        tr_ext=col(trefs, 3), tr_ext_scale=f32_up(col(trefs, 4)), tr_ext_delta=col(trefs, 5))
    gC, gCs = np.zeros((len(pcs), 3, 8)), np.zeros((len(pcs), 3, 8))
    for i, (c, r) in enumerate(zip(pcs, crefs)):
        gC[i, :, 8 - 2 * c[1]:], gCs[i, :, 8 - 2 * c[1]:] = r["gC"], r["gC_scale"]
    data.update(pn_gC=gC, pn_gC_scale=f32_up(gCs))
    # what the families promise, from the reference itself
    quiet = np.array(["quiet" in f or f == "none/loud" for f in data["pn_family"]])
    assert (data["pn_pc"][quiet] == 0.0).all()
    for grp in np.unique(data["pn_group"][data["pn_group"] % 3 != 0]):           # the linear and the cubic sets
        assert (data["pn_pc"][(data["pn_group"] == grp) & ~quiet] > 0.0).any(), grp
    return data


if __name__ == "__main__":
    procs = int(sys.argv[sys.argv.index("--procs") + 1]) if "--procs" in sys.argv else min(16, os.cpu_count() or 1)
    data = generate(procs)
    if "--check" in sys.argv:
        with open(OUT, "rb") as f:
            assert f.read() == npz_bytes(data), "the generator no longer reproduces " + OUT
        print("fixture reproduced byte for byte")
    else:
        with open(OUT, "wb") as f:
            f.write(npz_bytes(data))
    fam, cnt = np.unique(data["pt_family"], return_counts=True)
    print(len(data["pt_delta"]), "pointwise", dict(zip(fam.tolist(), cnt.tolist())), len(data["pn_pc"]), "piece cases on",
          len(data["pc_T"]), "pieces,", len(data["tr_s"]), "trajectories,", os.path.getsize(OUT), "bytes")
