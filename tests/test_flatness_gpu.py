"""Differential flatness on the GPU against the torch restatement of tests/flatness_np.py (checked on its own in
tests/test_flatness_cpu.py): the pointwise map and its adjoint, states and sampled extrema along trajectories, the thrust /
tilt / body-rate penalty with its partial and total gradients, the accumulate contract, the torch layer, the host L-BFGS on
the composed objective and the C++ facade.

In tests 1 to 11 states are drawn inside the planner's boxes (|v| <= 4, |a| <= 6 per axis) and trajectories are slowed down
until they stay inside them, so zu_3 >= 0.8 > 0 everywhere and no case has to be left out for the singular attitude.  Tests
12 to 14 leave the boxes: they compare all five kernels with the 70-digit reference of tests/flatness_mp.py on the families
of tests/golden/flatness_cases.npz (hover, small tilt, fast, slow, free fall, towards inversion, other vehicles), every
output against a bound derived before any run."""
import json
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import flatness_mp as fmp
from tests import flatness_np as fnp
from tests.util import random_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _params():
    import allocnet_amd as aa
    return aa.make_flat_params()           # the launch file's vehicle, fnp.LAUNCH


def _bm(a, ld, fill=0.0):
    """(n, f) or (n,) numpy -> batch-minor torch tensor (f, ld) or (ld,) on the device."""
    a = np.asarray(a, dtype=np.float64)
    t = torch.full((a.shape[1] if a.ndim == 2 else 1, ld), fill, dtype=torch.float64)
    t[:, :a.shape[0]] = torch.from_numpy(a.reshape(a.shape[0], -1)).T
    t = t.to(DEV)
    return t if a.ndim == 2 else t[0]


def _states(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-4.0, 4.0, (n, 3)), rng.uniform(-6.0, 6.0, (n, 3)), rng.normal(size=(n, 3)) * 5.0,
            rng.uniform(-math.pi, math.pi, n), rng.normal(size=n))


def _close(got, ref, tol, what):
    got, ref = np.asarray(got), np.asarray(ref)
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print(f"{what}: worst {err.max():.3e} (bar {tol:g})")
    assert err.max() <= tol, (what, err.max())


def _trajectories(anet_ctx, s, N, B, seed):
    """Rest-to-rest random-walk problems (SURVEY config 2's generator), durations scaled per trajectory by a common factor until the
    restatement's sampled |v|, |a| are inside the planner's boxes."""
    import allocnet_amd as aa
    rng = np.random.default_rng(seed)
    c = min(s, 3)
    head, tail, wps, T = random_problem(rng, B, N, c, rest=True)
    T, co = fnp.scale_into_limits(lambda t: aa.minco_solve(head, tail, wps, t, s, ctx=anet_ctx)[0], T)
    return head, tail, wps, T, co


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yaw", [True, False])
def test_flat_forward_matches_the_restatement(anet_ctx, yaw):
    import allocnet_amd as aa
    n = 100_000
    v, a, j, psi, dpsi = _states(n, 21)
    ld = aa.recommended_ld(n)
    thr, quat, omg = aa.flat_forward_dev(_params(), _bm(v, ld), _bm(a, ld), _bm(j, ld), _bm(psi, ld) if yaw else None,
                                         _bm(dpsi, ld) if yaw else None, n=n, ctx=anet_ctx)
    rt, rq, ro, _ = fnp.forward(v, a, j, psi if yaw else None, dpsi if yaw else None)
    _close(thr[:n].cpu().numpy(), rt.numpy(), 1e-12, "thr")
    _close(quat[:, :n].T.cpu().numpy(), rq.numpy(), 1e-12, "quat")
    _close(omg[:, :n].T.cpu().numpy(), ro.numpy(), 1e-12, "omg")
    # the host entry point and the single-state mirror answer the same
    ht, hq, ho = aa.flat_forward(_params(), v[:257], a[:257], j[:257], psi[:257] if yaw else None, dpsi[:257] if yaw else None,
                                 ctx=anet_ctx)
    assert np.array_equal(ht, thr[:257].cpu().numpy()) and np.array_equal(hq, quat[:, :257].T.cpu().numpy())
    fm = aa.FlatnessMap(ctx=anet_ctx)
    fm.reset(1.0, 9.8, 0.7, 0.8, 0.01, 1e-4)
    t1, q1, o1 = fm.forward(v[3], a[3], j[3], psi[3] if yaw else 0.0, dpsi[3] if yaw else 0.0)
    _close(np.r_[t1, q1, o1], np.r_[ht[3], hq[3], ho[3]], 1e-12, "FlatnessMap.forward")


# 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yaw", [True, False])
def test_flat_backward_matches_autograd(anet_ctx, yaw):
    import allocnet_amd as aa
    n = 20_000
    v, a, j, psi, dpsi = _states(n, 22)
    if not yaw:
        psi, dpsi = np.zeros(n), np.zeros(n)
    rng = np.random.default_rng(23)
    gt, gq, go = rng.normal(size=n), rng.normal(size=(n, 4)), rng.normal(size=(n, 3))
    gp, gv = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    ld = aa.recommended_ld(n)
    out = aa.flat_backward_dev(_params(), _bm(v, ld), _bm(a, ld), _bm(j, ld), _bm(psi, ld) if yaw else None,
                               _bm(dpsi, ld) if yaw else None, _bm(gp, ld), _bm(gv, ld), _bm(gt, ld), _bm(gq, ld), _bm(go, ld),
                               n=n, ctx=anet_ctx)
    pt, vt, at, jt, pst, dpt = [(t[:, :n].T if t.dim() == 2 else t[:n]).cpu().numpy() for t in out]
    rv, ra, rj, rpsi, rdpsi = fnp.backward(v, a, j, psi, dpsi, gt, gq, go)
    assert np.array_equal(pt, gp)                                        # pos_grad passes through
    _close(vt, rv + gv, 1e-10, "vel_total")                              # vel_grad passes through additively
    _close(at, ra, 1e-10, "acc_total")
    _close(jt, rj, 1e-10, "jer_total")
    _close(pst, rpsi, 1e-10, "psi_total")
    _close(dpt, rdpsi, 1e-10, "dpsi_total")
    # FlatnessMap.backward applies to the last forward's inputs
    fm = aa.FlatnessMap(ctx=anet_ctx)
    fm.forward(v[5], a[5], j[5], psi[5], dpsi[5])
    one = fm.backward(gp[5], gv[5], gt[5], gq[5], go[5])
    for got, ref in zip(one, (gp[5], rv[5] + gv[5], ra[5], rj[5], rpsi[5], rdpsi[5])):
        _close(got, ref, 1e-10, "FlatnessMap.backward")


# 3 ---------------------------------------------------------------------------------------------
SHAPES = [(2, 3), (3, 5), (3, 16), (4, 5), (4, 8)]


@pytest.mark.parametrize("s,N", SHAPES)
def test_traj_flat_states(anet_ctx, s, N):
    import allocnet_amd as aa
    B = 64
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, B, 300 + 10 * s + N)
    rng = np.random.default_rng(31)
    tot = T.sum(1)
    knot = np.cumsum(T, 1)[:, N // 2 - 1] if N > 1 else T[:, 0]
    tq = np.stack([np.zeros(B), knot, tot, tot + 0.3] + [rng.uniform(0.0, 1.0, B) * tot for _ in range(5)], 1)
    fm = aa.FlatnessMap(ctx=anet_ctx)
    got = aa.traj_flat_states(fm, co, T, tq, ctx=anet_ctx)
    v, a, j = (aa.traj_eval(co, T, tq, d, ctx=anet_ctx) for d in (1, 2, 3))
    rt, rq, ro, _ = fnp.forward(v, a, j)
    ref = np.concatenate([rt.numpy()[..., None], rq.numpy(), ro.numpy(), np.linalg.norm(v, axis=-1)[..., None],
                          fnp.tilt_of_quat(rq).numpy()[..., None],
                          np.linalg.norm(ro.numpy(), axis=-1)[..., None]], -1)
    _close(got, ref, 1e-12, f"states s={s} N={N}")
    # Trajectory.getFlatState is the same call for one trajectory
    tr = aa.Trajectory(T[2], co[2], ctx=anet_ctx)
    st = tr.getFlatState(tq[2, 5], fm)
    assert st["thr"] == got[2, 5, 0] and np.array_equal(st["quat"], got[2, 5, 1:5]) and st["tilt"] == got[2, 5, 9]


# 4 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,N", SHAPES)
def test_traj_flat_extrema_and_limits(anet_ctx, s, N):
    import allocnet_amd as aa
    B, res = 70, 20
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, B, 400 + 10 * s + N)
    fm = aa.FlatnessMap(ctx=anet_ctx)
    got = aa.traj_flat_extrema(fm, co, T, res, ctx=anet_ctx)
    sm = fnp.traj_samples(co, T, res, closed=True)
    ref = np.stack([sm["thr"].amin((1, 2)).numpy(), sm["thr"].amax((1, 2)).numpy(),
                    fnp.tilt_of_quat(sm["quat"]).amax((1, 2)).numpy(), torch.sqrt(sm["bdr2"].amax((1, 2))).numpy()], 1)
    _close(got, ref, 1e-12, f"extrema s={s} N={N}")
    tr = aa.Trajectory(T[1], co[1], ctx=anet_ctx)
    lo, hi, tilt, bdr = tr.getFlatExtrema(fm, res)
    assert (lo, hi, tilt, bdr) == tuple(got[1])
    up, dn = 1.0 + 1e-9, 1.0 - 1e-9
    assert tr.checkFlatLimits(fm, lo * dn, hi * up, tilt * up, bdr * up, res)
    assert not tr.checkFlatLimits(fm, lo * up, hi * up, tilt * up, bdr * up, res)     # thrust drops below the minimum
    assert not tr.checkFlatLimits(fm, lo * dn, hi * dn, tilt * up, bdr * up, res)     # thrust exceeds the maximum
    assert not tr.checkFlatLimits(fm, lo * dn, hi * up, tilt * dn, bdr * up, res)     # tilt
    assert not tr.checkFlatLimits(fm, lo * dn, hi * up, tilt * up, bdr * dn, res)     # body rate


# 5 ---------------------------------------------------------------------------------------------
def _limits_from(co, T, res, weights=(30.0, 200.0, 10.0)):
    """Limits at the 70th / 30th percentiles of the restatement's sampled values over the set, smooth_mu a tenth of the smallest
    spread; asserts that every row type is active on >= 10 % and inactive on >= 10 % of the samples."""
    sm = fnp.traj_samples(co, T, res)
    thr, ct, b2 = (sm[k].numpy().ravel() for k in ("thr", "cos_tilt", "bdr2"))
    thr_max, thr_min = np.percentile(thr, 70), np.percentile(thr, 30)
    cos_max, b2_max = np.percentile(ct, 30), np.percentile(b2, 70)
    spreads = [thr_max - thr_min, np.percentile(ct, 70) - cos_max, b2_max - np.percentile(b2, 30)]
    mu = 0.1 * min(spreads)
    assert mu > 0.0
    for name, active in (("max thrust", thr > thr_max), ("min thrust", thr < thr_min), ("tilt", ct < cos_max), ("body rate", b2 > b2_max)):
        frac = active.mean()
        print(f"{name}: active on {100 * frac:.1f} % of {active.size} samples")
        assert 0.1 <= frac <= 0.9, (name, frac)
    return dict(w_thr=weights[0], w_tilt=weights[1], w_bdr=weights[2], mu=mu, thr_min=thr_min, thr_max=thr_max,
                tilt_max=math.acos(cos_max), bdr_max=math.sqrt(b2_max))


def _penalty_of(kw, res):
    import allocnet_amd as aa
    return aa.make_flat_penalty(w_thrust=kw["w_thr"], w_tilt=kw["w_tilt"], w_bdr=kw["w_bdr"], smooth_mu=kw["mu"],
                                min_thrust=kw["thr_min"], max_thrust=kw["thr_max"], max_tilt=kw["tilt_max"], max_bdr=kw["bdr_max"],
                                res=res)


def _flat_partials(anet_ctx, pen, s, N, B, co, T, accumulate=False, into=None, fill=float("nan")):
    """anet_minco_flat_partial_grads_dev on trajectory-major numpy inputs -> the device tensors gdC, gdT, piece_cost (whole rows,
    padding lanes included) and ld."""
    import allocnet_amd as aa
    ld = aa.recommended_ld(B) if B > 1 else 1
    d_co, d_T = _bm(co.reshape(B, -1), ld), _bm(T, ld, fill=1.0)
    if into is None:
        into = tuple(torch.full((r, ld), fill, dtype=torch.float64, device=DEV) for r in (N * 3 * 2 * s, N, N))
    aa.minco_flat_partial_grads_dev(_params(), pen, s, N, B, d_co, d_T, into[0], into[1], into[2], accumulate=accumulate, ctx=anet_ctx)
    torch.cuda.synchronize()
    return into, ld, d_co, d_T


@pytest.mark.parametrize("res", [5, 20])
@pytest.mark.parametrize("s,N,B", [(3, 5, 1), (3, 16, 300), (4, 5, 4096), (4, 8, 4096)])
def test_flat_partial_grads_match_autograd(anet_ctx, s, N, B, res):
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, B, 500 + 100 * s + N)
    kw = _limits_from(co, T, res)
    (gC, gT, pc), ld, _, _ = _flat_partials(anet_ctx, _penalty_of(kw, res), s, N, B, co, T)
    rpc, rgC, rgT = fnp.j_flat_grads(co, T, res, **kw)
    cost, rcost = pc[:, :B].sum(0).cpu().numpy(), rpc.sum(1)
    rel = np.abs(cost - rcost) / np.maximum(np.abs(rcost), 1e-300)
    rel[rcost == 0.0] = np.abs(cost[rcost == 0.0])
    print(f"cost: worst relative {rel.max():.3e} (bar 1e-9)")
    assert rel.max() <= 1e-9
    g = gC[:, :B].T.cpu().numpy().reshape(B, N, 3, 2 * s)
    eC = np.abs(g - rgC).max() / max(1.0, np.abs(rgC).max())
    eT = np.abs(gT[:, :B].T.cpu().numpy() - rgT).max() / max(1.0, np.abs(rgT).max())
    print(f"gdC: {eC:.3e}, gdT: {eT:.3e} (bar 1e-7); |gdC| max {np.abs(rgC).max():.3e}, |gdT| max {np.abs(rgT).max():.3e}")
    assert np.abs(rgC).max() > 0.0 and np.abs(rgT).max() > 0.0
    assert eC <= 1e-7 and eT <= 1e-7


# 6 ---------------------------------------------------------------------------------------------
def test_minco_flat_cost_grad_finite_differences(anet_ctx):
    import allocnet_amd as aa
    s, c, N, B, res = 4, 3, 6, 8, 7
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, B, 61)
    kw = _limits_from(co, T, res)
    fpen = _penalty_of(kw, res)
    pen = aa.make_penalty(rho=2.0, w_vel=25.0, w_acc=9.0, smooth_mu=0.05, max_vel=1.5, max_acc=2.5, res=9)
    fm = aa.FlatnessMap(ctx=anet_ctx)
    f = lambda w, t: aa.minco_flat_cost_grad(head, tail, w, t, s, fm, fpen, penalty=pen, ctx=anet_ctx)
    cost, gP, gT = f(wps, T)
    base = aa.minco_cost_grad(head, tail, wps, T, s, penalty=pen, ctx=anet_ctx)[0]
    jf = fnp.j_flat(co, T, res, **kw).sum(1).numpy()
    assert (jf > 0.0).any()
    rel = np.abs(cost - (base + jf)) / np.abs(base + jf)
    print(f"cost against minco_cost_grad + J_flat: worst relative {rel.max():.3e} (bar 1e-9)")
    assert rel.max() <= 1e-9
    h = 1e-6
    for (k, ax) in [(0, 0), (2, 1), (4, 2)]:
        wp = wps.copy(); wp[:, k, ax] += h; wm = wps.copy(); wm[:, k, ax] -= h
        fd = (f(wp, T)[0] - f(wm, T)[0]) / (2 * h)
        err = np.abs(fd - gP[:, k, ax]).max() / max(1.0, np.abs(gP[:, k, ax]).max())
        print(f"gradP[{k},{ax}]: {err:.3e} (bar 2e-5)")
        assert err <= 2e-5
    for i in (0, 3, 5):
        tp = T.copy(); tp[:, i] += h; tm = T.copy(); tm[:, i] -= h
        fd = (f(wps, tp)[0] - f(wps, tm)[0]) / (2 * h)
        err = np.abs(fd - gT[:, i]).max() / max(1.0, np.abs(gT[:, i]).max())
        print(f"gradT[{i}]: {err:.3e} (bar 2e-5)")
        assert err <= 2e-5


# 7 ---------------------------------------------------------------------------------------------
def test_accumulate_contract(anet_ctx):
    """accumulate = 1 after anet_minco_partial_grads_dev equals the sum of the two separate results TO THE LAST BIT: the kernel
    forms its own share completely, exactly as it does for accumulate = 0, and adds it to the stored value with one addition the
    compiler may not fuse with the products before it -- the same two roundings as adding the separate results.  accumulate = 0
    overwrites a poisoned buffer, and lanes in [batch, ld) are never touched."""
    import ctypes
    import allocnet_amd as aa
    s, N, B, res = 4, 8, 1000, 20
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, B, 71)
    fpen = _penalty_of(_limits_from(co, T, res), res)
    (fC, fT, fpc), ld, d_co, d_T = _flat_partials(anet_ctx, fpen, s, N, B, co, T)          # onto NaN
    assert ld > B
    for t in (fC, fT, fpc):
        assert torch.isfinite(t[:, :B]).all() and torch.isnan(t[:, B:]).all()
    pen = aa.make_penalty(rho=0.0, w_vel=25.0, w_acc=9.0, smooth_mu=0.05, max_vel=1.5, max_acc=2.5, res=res)
    eC, eT, epc = (torch.full_like(t, 123.0) for t in (fC, fT, fpc))
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    anet_ctx.check(anet_ctx.lib.anet_minco_partial_grads_dev(anet_ctx.handle, s, N, B, ld, q(d_co), q(d_T), None,
                                                             ctypes.cast(ctypes.pointer(pen), ctypes.c_void_p), 1, q(eC), q(eT), q(epc), st))
    torch.cuda.synchronize()
    sums = [e[:, :B] + f[:, :B] for e, f in ((eC, fC), (eT, fT), (epc, fpc))]
    assert float(epc[:, :B].sum()) > 0.0 and float(fpc[:, :B].sum()) > 0.0
    _flat_partials(anet_ctx, fpen, s, N, B, co, T, accumulate=True, into=(eC, eT, epc))
    for got, ref in zip((eC, eT, epc), sums):
        assert torch.equal(got[:, :B], ref)
        assert (got[:, B:] == 123.0).all()


# 8 ---------------------------------------------------------------------------------------------
def test_unreachable_limits_cost_nothing(anet_ctx):
    import allocnet_amd as aa
    s, N, B = 3, 5, 130
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, B, 81)
    pen = aa.make_flat_penalty(w_thrust=30.0, w_tilt=200.0, w_bdr=10.0, smooth_mu=0.01, min_thrust=-1e6, max_thrust=1e6,
                               max_tilt=3.1, max_bdr=1e6, res=20)
    (gC, gT, pc), ld, _, _ = _flat_partials(anet_ctx, pen, s, N, B, co, T)
    for t in (gC, gT, pc):
        assert (t[:, :B] == 0.0).all()


# 9 ---------------------------------------------------------------------------------------------
def test_flat_layer_gradcheck(anet_ctx):
    from allocnet_amd.torch_layer import flat_layer
    n = 8
    v, a, j, psi, dpsi = _states(n, 91)
    ins = [torch.tensor(x.T if x.ndim == 2 else x, dtype=torch.float64, device=DEV).contiguous().requires_grad_(True)
           for x in (v, a, j, psi, dpsi)]
    assert torch.autograd.gradcheck(lambda *x: flat_layer(*x, _params(), ctx=anet_ctx), ins, eps=1e-6, atol=1e-6, rtol=1e-5)


# 10 --------------------------------------------------------------------------------------------
def test_host_lbfgs_on_the_composed_objective(anet_ctx):
    """One 5-piece jerk problem whose start violates the tilt limit: the host L-BFGS with minco_flat_cost_grad as the objective
    ends with a non-negative status and a lower cost.  Nothing is asserted about the tilt itself (the energy may trade against it)."""
    import allocnet_amd as aa
    s, N = 3, 5
    head, tail, wps, T, co = _trajectories(anet_ctx, s, N, 1, 101)
    fm = aa.FlatnessMap(ctx=anet_ctx)
    lo, hi, tilt, bdr = aa.traj_flat_extrema(fm, co, T, 20, ctx=anet_ctx)[0]
    fpen = aa.make_flat_penalty(w_thrust=10.0, w_tilt=1e3, w_bdr=1.0, smooth_mu=1e-3, min_thrust=0.5 * lo, max_thrust=2.0 * hi,
                                max_tilt=0.6 * tilt, max_bdr=3.0 * bdr, res=20)
    pen = aa.make_penalty(rho=5.0, res=20)
    nw = 3 * (N - 1)

    def evaluate(x):
        t = np.exp(x[nw:])[None]
        f, gP, gT = aa.minco_flat_cost_grad(head, tail, x[:nw].reshape(1, N - 1, 3), t, s, fm, fpen, penalty=pen, ctx=anet_ctx)
        return float(f[0]), np.r_[gP.reshape(-1), gT[0] * t[0]]
    x0 = np.r_[wps.reshape(-1), np.log(T[0])]
    j0 = evaluate(x0)[0]
    base = aa.minco_cost_grad(head, tail, wps, T, s, penalty=pen, ctx=anet_ctx)[0][0]
    assert j0 > base * (1.0 + 1e-6)                                      # the tilt row is active at the start
    ret, x, f, iters, evals = aa.lbfgs_optimize(x0, evaluate, param=aa.lbfgs_parameter_t(max_iterations=60), ctx=anet_ctx)
    print(f"status {ret} ({aa.lbfgs_strerror(ret)}), J {j0:.6g} -> {f:.6g} in {iters} iterations, {evals} evaluations")
    assert ret >= 0
    assert f < j0


# 11 --------------------------------------------------------------------------------------------
def test_cpp_flatness_program(anet_ctx):
    import allocnet_amd as aa
    src = os.path.join(ROOT, "tests", "cpp", "test_flatness.cpp")
    lib = os.path.join(ROOT, "allocnet_amd", "lib")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "test_flatness")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", lib, "-lallocnet_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
        res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    rows = np.array(json.loads(res.stdout)["rows"])
    assert rows.shape == (5, 3 + 9 + 8 + 14)
    # SURVEY config 1 through the Python facade
    N = 8
    goal = np.array([8.0, 3.0, 1.0])
    head = np.zeros((1, 3, 3)); tail = np.zeros((1, 3, 3)); tail[0, :, 0] = goal
    wps = (goal[None] * (np.arange(1, N)[:, None] / N))[None]
    T = np.ones((1, N))
    co, _ = aa.minco_solve(head, tail, wps, T, 4, ctx=anet_ctx)
    tq = rows[:, 0][None]
    v, a, j = (aa.traj_eval(co, T, tq, d, ctx=anet_ctx)[0] for d in (1, 2, 3))
    assert np.array_equal(rows[:, 3:12], np.concatenate([v, a, j], 1))
    psi, dpsi = rows[:, 1], rows[:, 2]
    thr, quat, omg = aa.flat_forward(_params(), v, a, j, psi, dpsi, ctx=anet_ctx)
    _close(rows[:, 12:20], np.concatenate([thr[:, None], quat, omg], 1), 1e-12, "C++ forward")
    ones = np.ones((5, 1))
    back = aa.flat_backward(_params(), v, a, j, psi, dpsi, ones * [0.25, -0.5, 0.75], ones * [-1.0, 0.5, 0.125], np.full(5, 1.25),
                            ones * [0.5, -1.5, 0.75, 2.0], ones * [0.3, -0.7, 1.1], ctx=anet_ctx)
    _close(rows[:, 20:], np.concatenate([back[0], back[1], back[2], back[3], back[4][:, None], back[5][:, None]], 1), 1e-10,
           "C++ backward")
    # ... and the Python facade is the restatement's map at these states
    rt, rq, ro, _ = fnp.forward(v, a, j, psi, dpsi)
    _close(np.concatenate([thr[:, None], quat, omg], 1), np.concatenate([rt.numpy()[:, None], rq.numpy(), ro.numpy()], 1), 1e-12,
           "facade against the restatement")


# 12 --------------------------------------------------------------------------------------------
# The kernels against the 70-digit reference of tests/flatness_mp.py, read from tests/golden/flatness_cases.npz: every output of
# every lane within K eps scale (1 + 1/delta) of its own reference (K by counting roundings, scale and delta from the reference
# alone; flatness_mp's docstring and DESIGN.md 8f).  Nothing is compared relative to a batch maximum and no case is left out.

@pytest.fixture(scope="module")
def fx():
    return fmp.load()


def _cycled(n_cases, n_lanes, shift=0):
    """lane -> case with a stride coprime to the number of cases: every case on some lane, neighbours differ"""
    stride = next(p for p in (7, 11, 13, 17, 5, 3, 1) if math.gcd(p, n_cases) == 1)
    return (np.arange(n_lanes) * stride + shift) % n_cases


def _ratios(got, ref, scale, delta, K):
    """|got - ref| / bound per entry; a zero bound asks for equality; anything not finite is inf"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bnd = np.broadcast_to(fmp.flat_bound(scale, delta, K), ref.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bnd > 0.0, err / bnd, np.where(err == 0.0, 0.0, np.inf))
    return np.where(np.isfinite(got), r, np.inf)


def _report(what, fams, r, check=True):
    """r (lanes, ...) -> prints the worst ratio per family and returns them; check: asserts all <= 1"""
    r = np.asarray(r).reshape(len(fams), -1).max(1)
    worst = {}
    for f, x in zip(fams, r):
        worst[str(f)] = max(worst.get(str(f), 0.0), float(x))
    print(what + ", error / bound: " + ", ".join(f"{f} {x:.3g}" for f, x in worst.items()))
    assert not check or max(worst.values()) <= 1.0, (what, worst)
    return worst


@pytest.mark.parametrize("yaw", [True, False])
def test_flat_forward_backward_meet_the_mp_bounds(anet_ctx, fx, yaw):
    import allocnet_amd as aa
    n = 263                                                              # one full 256-lane block and a 7-lane tail
    ld = aa.recommended_ld(n)
    seen = 0
    for veh in range(len(fx["vehicles"])):
        cases = np.flatnonzero((fx["pt_veh"] == veh) & (fx["pt_yaw"] == yaw))
        seen += len(cases)
        k = cases[_cycled(len(cases), n)]
        par = aa.make_flat_params(*fx["vehicles"][veh])
        v, a, j, g = fx["pt_v"][k], fx["pt_a"][k], fx["pt_j"][k], fx["pt_g"][k]
        psi, dpsi = (fx["pt_psi"][k], fx["pt_dpsi"][k]) if yaw else (None, None)
        dv, da, dj = _bm(v, ld), _bm(a, ld), _bm(j, ld)
        dps, ddp = (_bm(psi, ld), _bm(dpsi, ld)) if yaw else (None, None)
        thr, quat, omg = aa.flat_forward_dev(par, dv, da, dj, dps, ddp, n=n, ctx=anet_ctx)
        got = np.c_[thr[:n].cpu().numpy(), quat[:, :n].T.cpu().numpy(), omg[:, :n].T.cpu().numpy()]
        dl = fx["pt_delta"][k][:, None]
        _report(f"forward yaw={yaw} vehicle {veh}", fx["pt_family"][k], _ratios(got, fx["pt_fwd"][k], fx["pt_fwd_scale"][k], dl, fmp.K_FWD))
        out = aa.flat_backward_dev(par, dv, da, dj, dps, ddp, None, None, _bm(g[:, 0], ld), _bm(g[:, 1:5], ld), _bm(g[:, 5:8], ld),
                                   n=n, ctx=anet_ctx)
        _, vt, at, jt, pst, dpt = [(t[:, :n].T if t.dim() == 2 else t[:n]).cpu().numpy() for t in out]
        gad = np.c_[vt, at, jt, pst, dpt]
        _report(f"adjoint yaw={yaw} vehicle {veh}", fx["pt_family"][k], _ratios(gad, fx["pt_adj"][k], fx["pt_adj_scale"][k], dl, fmp.K_ADJ))
        # exact hover: v = a = 0 and j != 0 give thr = m g and the tilt quaternion (1, 0, 0, 0) with no rounding at all
        hov = np.flatnonzero((fx["pt_family"][k] == "hover") & (np.abs(v).sum(1) + np.abs(a).sum(1) == 0.0))
        if veh == 0:
            assert len(hov) >= 1 and np.abs(j[hov]).min() > 0.0
            assert (got[hov, 0] == fx["vehicles"][0][0] * fx["vehicles"][0][1]).all() and (got[hov, 0] == fx["pt_fwd"][k][hov, 0]).all()
            assert (got[hov, 2] == 0.0).all() and (got[hov, 3] == 0.0).all()
            if not yaw:
                assert (got[hov, 1:5] == [1.0, 0.0, 0.0, 0.0]).all()
        # the host forms: the same bits at n = 1 and n = 3
        for m in (1, 3):
            ht, hq, ho = aa.flat_forward(par, v[:m], a[:m], j[:m], psi[:m] if yaw else None, dpsi[:m] if yaw else None, ctx=anet_ctx)
            assert np.array_equal(np.c_[ht, hq, ho], got[:m])
            hb = aa.flat_backward(par, v[:m], a[:m], j[:m], psi[:m] if yaw else None, dpsi[:m] if yaw else None, None, None,
                                  g[:m, 0], g[:m, 1:5], g[:m, 5:8], ctx=anet_ctx)
            assert np.array_equal(np.c_[hb[1], hb[2], hb[3], hb[4], hb[5]], gad[:m])
    assert seen == 64                                                    # every case of this half went through a launch


# 13 --------------------------------------------------------------------------------------------
def _piece_launch(anet_ctx, fx, s, cases, lane_case, B, N, accumulate=False, into=None):
    """One launch of anet_minco_flat_partial_grads_dev with slot (b, i) holding the fixture case cases[lane_case[b, i]] (all of
    one limit set) -> gC (B, N, 3, D), gT (B, N), pc (B, N) and the case of every slot."""
    D = 2 * s
    which = cases[lane_case]                                              # (B, N)
    pieces = fx["pn_piece"][which]
    co = fx["pc_cm"][pieces][..., 8 - D:]                                 # (B, N, 3, D)
    T = fx["pc_T"][pieces]
    pen = fx["pn_pen"][cases[0]]
    assert (fx["pn_pen"][cases] == pen).all()
    kw = dict(w_thr=pen[0], w_tilt=pen[1], w_bdr=pen[2], mu=pen[3], thr_min=pen[4], thr_max=pen[5], tilt_max=pen[6], bdr_max=pen[7])
    (gC, gT, pc), ld, _, _ = _flat_partials(anet_ctx, _penalty_of(kw, int(pen[8])), s, N, B, np.ascontiguousarray(co), T,
                                            accumulate=accumulate, into=into)
    return (gC[:, :B].T.cpu().numpy().reshape(B, N, 3, D), gT[:, :B].T.cpu().numpy(), pc[:, :B].T.cpu().numpy(), which, (gC, gT, pc), ld)


def _check_pieces(what, fx, s, out):
    gC, gT, pc, which = out[:4]
    D = 2 * s
    dl = fx["pn_delta"][which]
    r = np.concatenate([_ratios(gC, fx["pn_gC"][which][..., 8 - D:], fx["pn_gC_scale"][which][..., 8 - D:], dl[..., None, None],
                                fmp.K_PIECE).reshape(which.size, -1),
                        _ratios(gT, fx["pn_gT"][which], fx["pn_gT_scale"][which], dl, fmp.K_PIECE).reshape(-1, 1),
                        _ratios(pc, fx["pn_pc"][which], fx["pn_pc_scale"][which], dl, fmp.K_PIECE).reshape(-1, 1)], 1)
    _report(what, fx["pn_family"][which].ravel(), r)


@pytest.mark.parametrize("res", [1, 4])
@pytest.mark.parametrize("s", [3, 4])
def test_flat_partial_grads_meet_the_mp_bounds(anet_ctx, fx, s, res):
    """piece_cost, every gdC entry and gdT of every (lane, piece) against their own bounds, one launch per limit set, in two
    arrangements: cycled (every 64-lane wave mixes pieces with and without an active row) and sorted (lanes 0..127, two whole
    waves, hold only pieces without an active row, so those waves take the wave-uniform skip of the adjoint, next to whole
    waves of active pieces)."""
    B, N = 263, 3
    groups = np.unique(fx["pn_group"][(fx["pn_s"] == s) & (fx["pn_res"] == res)])
    assert len(groups) == 3
    skipping_waves = 0
    for grp in groups:
        cases = np.flatnonzero(fx["pn_group"] == grp)
        nc = len(cases)
        name = str(fx["pn_family"][cases[0]]).split("/")[0]
        cyc = (_cycled(nc, B)[:, None] + np.arange(N)[None]) % nc
        _check_pieces(f"pieces s={s} res={res} {name} cycled", fx, s, _piece_launch(anet_ctx, fx, s, cases, cyc, B, N))
        quiet = np.flatnonzero(fx["pn_pc"][cases] == 0.0)
        loud = np.flatnonzero(fx["pn_pc"][cases] > 0.0)
        if len(quiet) and len(loud):
            srt = np.empty((B, N), dtype=np.int64)
            srt[:128] = quiet[(_cycled(len(quiet), 128)[:, None] + np.arange(N)[None]) % len(quiet)]
            srt[128:] = loud[(_cycled(len(loud), B - 128)[:, None] + np.arange(N)[None]) % len(loud)]
            out = _piece_launch(anet_ctx, fx, s, cases, srt, B, N)
            _check_pieces(f"pieces s={s} res={res} {name} sorted", fx, s, out)
            assert (out[2][:128] == 0.0).all() and (out[0][:128] == 0.0).all() and (out[2][128:192] > 0.0).any()
            skipping_waves += 1
        if name == "linear":
            # accumulate = 1 onto a known buffer: one unfused addition of the same share
            plain = _piece_launch(anet_ctx, fx, s, cases, cyc, B, N)
            ld = plain[5]
            into = tuple(torch.full((r, ld), 0.625, dtype=torch.float64, device=DEV) for r in (N * 3 * 2 * s, N, N))
            _piece_launch(anet_ctx, fx, s, cases, cyc, B, N, accumulate=True, into=into)
            for acc, share in zip(into, plain[4]):
                assert torch.equal(acc[:, :B], 0.625 + share[:, :B]) and (acc[:, B:] == 0.625).all()
            # one trajectory, ld = 1
            one = np.flatnonzero(fx["pn_pc"][cases] > 0.0)[:1]
            _check_pieces(f"pieces s={s} res={res} {name} B=1", fx, s, _piece_launch(anet_ctx, fx, s, cases, np.repeat(one, N)[None], 1, N))
    assert skipping_waves >= 2                                           # the linear and the cubic set


# 14 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [71, 263])
@pytest.mark.parametrize("s", [3, 4])
def test_traj_flat_states_and_extrema_meet_the_mp_bounds(anet_ctx, fx, s, B):
    """Every field of every query and all four extrema (64 x 4 workgroups with their LDS reduction, and a tail), tilt and speed
    included; nothing is NaN on any family, the tilted one (delta down to 1e-3) included."""
    import allocnet_amd as aa
    D = 2 * s
    trs = np.flatnonzero((fx["tr_s"] == 0) | (fx["tr_s"] == s))
    assert len(trs) == 12
    k = trs[_cycled(len(trs), B)]
    pieces = fx["tr_piece"][k]                                             # (B, 3)
    co, T, tq = np.ascontiguousarray(fx["pc_cm"][pieces][..., 8 - D:]), fx["pc_T"][pieces], fx["tr_tq"][k]
    fm = aa.FlatnessMap(ctx=anet_ctx)
    got = aa.traj_flat_states(fm, co, T, tq, ctx=anet_ctx)
    ext = aa.traj_flat_extrema(fm, co, T, 4, ctx=anet_ctx)
    print(f"not finite: {int((~np.isfinite(got)).sum())} state fields, {int((~np.isfinite(ext)).sum())} extrema")
    ws = _report(f"states s={s} B={B}", fx["tr_family"][k], check=False,
                 r=_ratios(got, fx["tr_state"][k], fx["tr_state_scale"][k], fx["tr_state_delta"][k][..., None], fmp.K_TRAJ))
    we = _report(f"extrema s={s} B={B}", fx["tr_family"][k], check=False,
                 r=_ratios(ext, fx["tr_ext"][k], fx["tr_ext_scale"][k], fx["tr_ext_delta"][k][:, None], fmp.K_TRAJ))
    assert np.isfinite(got).all() and np.isfinite(ext).all()
    assert max(ws.values()) <= 1.0 and max(we.values()) <= 1.0, (ws, we)
    hov = np.flatnonzero(fx["tr_family"][k] == "hover")
    assert len(hov) and (got[hov][:, :, 9] == 0.0).all() and (ext[hov, 2] == 0.0).all()      # no tilt at exact hover
