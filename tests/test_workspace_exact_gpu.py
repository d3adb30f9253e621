"""Every entry point that takes a caller's workspace stays inside exactly what its anet_*_workspace() function asks for.

Through ctx.lib directly: the workspace of exactly that many doubles lies between two guard bands of 4096 doubles holding a
sentinel bit pattern; one run; both bands untouched; and the outputs equal those of the same call on a workspace twice the size --
bitwise where the project asserts run-to-run bit equality already (the interior-point QP, the one-launch MINCO L-BFGS, cost +
gradient), else within the tolerance of the entry point's own GPU test.  The shapes are the smallest that reach each carve of
csrc/workspace.h.  Launch forms the environment selects (tuning() reads it once per process) run in a fresh python each,
started here with a time limit of its own; the cases of this process run under the suite's per-test limit."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from allocnet_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
SENTINEL = 0x7FF85EA1ED00C0DE       # (a NaN as a double: a kernel that reads workspace it never wrote shows in the outputs too)
PEN = dict(rho=50.0, w_corridor=1e4, w_vel=1e3, w_acc=1e3, smooth_mu=1e-2, max_vel=4.0, max_acc=6.0, res=20)
# How the outputs on the exact and on the double workspace are compared.  BITWISE: test_qp_launch_forms_gpu (three and two per CU
# agree), test_minco_lbfgs_two_launch_form_returns_the_same_bits, test_edge_cases_gpu (cost + gradient replayed from a graph).
# Else the bound of the entry point's own test, as (kind, bound): "max" = largest difference <= bound x max(1, largest magnitude)
# (FIRI: test_device_pointer_entry_point; lockstep L-BFGS: test_minco_lbfgs_one_launch_agrees_with_lockstep, its tightest);
# "allclose" = numpy.allclose(rtol = bound, atol = bound / 100) (ADMM: qp_solve_dev against the host call in test_qp_solve_gpu).
BITWISE, LOCKSTEP_TOL, ADMM_TOL, FIRI_TOL = ("bits", 0.0), ("max", 1e-10), ("allclose", 1e-9), ("max", 1e-9)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _to_bm(torch, a, B, ld, dev):
    """(B, ...) host array -> batch-minor (fields, ld) device tensor"""
    t = torch.zeros(int(np.prod(a.shape[1:])), ld, device=dev, dtype=torch.float64)
    t[:, :B] = torch.from_numpy(np.ascontiguousarray(a.reshape(B, -1).T)).to(dev)
    return t


def _struct(s):
    return ctypes.cast(ctypes.pointer(s), ctypes.c_void_p)


def _qp_case(aa, ctx, torch, dev, B, method):
    s, N, res, M = 3, 2, 2, 4
    rng = np.random.default_rng(5)
    head, tail, wps, T = synth.random_problem(rng, B, N, 3, rest=True)
    pts = np.concatenate([head[:, None, :, 0], wps, tail[:, None, :, 0]], axis=1)
    hp = np.zeros((B, N, M, 4))          # four rows: a box in x and y around each segment
    lo, hi = np.minimum(pts[:, :-1], pts[:, 1:]) - 1.5, np.maximum(pts[:, :-1], pts[:, 1:]) + 1.5
    for ax in range(2):
        hp[:, :, 2 * ax, ax] = 1.0; hp[:, :, 2 * ax, 3] = hi[:, :, ax]
        hp[:, :, 2 * ax + 1, ax] = -1.0; hp[:, :, 2 * ax + 1, 3] = -lo[:, :, ax]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    state, tT, thp = t(np.stack([head, tail], axis=1)[..., :3]), t(T * 1.5), t(hp)
    st = aa.qp_settings(method=method)
    n_work = int(ctx.lib.anet_qp_solve_workspace(s, N, B, res, M))
    form = int(ctx.lib.anet_qp_ipm_launch_form(ctx.handle, s, N, B, res, M, 0))

    def run(work):
        out = dict(coeffs=torch.empty((B, N, 3, 2 * s), device=dev, dtype=torch.float64), obj=torch.empty(B, device=dev, dtype=torch.float64),
                   status=torch.empty(B, device=dev, dtype=torch.int32), iters=torch.empty(B, device=dev, dtype=torch.int32))
        # residuals NULL: the solver keeps them in the workspace (the interior point inside the front, ADMM behind it)
        ctx.check(ctx.lib.anet_qp_solve_dev(ctx.handle, s, N, B, res, M, 4.0, 6.0, 1400.0, _vp(state), _vp(tT), _vp(thp), _struct(st),
                                            _vp(work), _vp(out["coeffs"]), _vp(out["obj"]), _vp(out["status"]), _vp(out["iters"]), None,
                                            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return out
    return n_work, run, dict(form=form)


def _lbfgs_case(aa, ctx, torch, dev, N, B, opt, max_evals):
    s, c, M = 3, 3, 8
    ld = aa.recommended_ld(B)
    head, tail, wps, T, hp = synth.corridor_problem(np.random.default_rng(7), B, N, c, M)
    pen = aa.make_penalty(poly_rows=M, **PEN)
    prm = aa.lbfgs_parameter_t()
    n_work = int(ctx.lib.anet_lbfgs_minco_workspace(s, N, ld, _struct(prm)))

    def run(work):
        th, tt, tw, tT, thp = (_to_bm(torch, x, B, ld, dev) for x in (head, tail, wps, T, hp))   # (wps and T are updated in place)
        out = dict(cost=torch.empty(ld, device=dev, dtype=torch.float64), coeffs=torch.empty(N * 18, ld, device=dev, dtype=torch.float64),
                   **{k: torch.zeros(ld, device=dev, dtype=torch.int32) for k in ("status", "iters", "evals")})
        ctx.check(ctx.lib.anet_lbfgs_minco_dev(ctx.handle, s, c, N, B, ld, _vp(th), _vp(tt), _vp(tw), _vp(tT), _vp(thp), _struct(pen),
                                               _struct(prm), opt, max_evals, _vp(work), _vp(out["cost"]), _vp(out["coeffs"]),
                                               _vp(out["status"]), _vp(out["iters"]), _vp(out["evals"]),
                                               ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        out.update(wps=tw, T=tT)
        return {k: v[..., :B] for k, v in out.items()}
    return n_work, run, {}


def _cost_grad_case(aa, ctx, torch, dev, s):
    c, N, B, M = min(s, 3), 2, 3, 8
    ld = aa.recommended_ld(B)
    head, tail, wps, T, hp = synth.corridor_problem(np.random.default_rng(11), B, N, c, M)
    th, tt, tw, tT, thp = (_to_bm(torch, x, B, ld, dev) for x in (head, tail, wps, T, hp))
    pen = aa.make_penalty(poly_rows=M, **PEN)
    n_work = int(ctx.lib.anet_minco_cost_grad_workspace(s, N, ld))
    launches = int(ctx.lib.anet_minco_cost_grad_launches(ctx.handle, s, c, N, B, _struct(pen)))

    def run(work):
        out = dict(cost=torch.empty(ld, device=dev, dtype=torch.float64), gradP=torch.empty(3 * (N - 1), ld, device=dev, dtype=torch.float64),
                   gradT=torch.empty(N, ld, device=dev, dtype=torch.float64))
        # coeffs_out NULL: the coefficients live in the workspace
        ctx.check(ctx.lib.anet_minco_cost_grad_dev(ctx.handle, s, c, N, B, ld, _vp(th), _vp(tt), _vp(tw), _vp(tT), _vp(thp), _struct(pen),
                                                   _vp(work), _vp(out["cost"]), _vp(out["gradP"]), _vp(out["gradT"]), None,
                                                   ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return {k: v[..., :B] for k, v in out.items()}
    return n_work, run, dict(launches=launches)


def _firi_case(aa, ctx, torch, dev, max_points):
    B, H = 3, 12
    rng = np.random.default_rng(13)
    bd, pts, npts, a, b = synth.firi_pack([synth.firi_scene(rng, n) for n in ((5, 2, 0) if max_points else (0, 0, 0))])
    pc = np.zeros((B, max(max_points, 1), 3))           # exactly max_points per corridor (a scene may return fewer than asked)
    pc[:, :pts.shape[1]] = pts[:, :max_points] if max_points else 0.0
    t = lambda x, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dtype=dt)
    tbd, tpc, tnp, ta, tb = t(bd), t(pc), t(np.minimum(npts, max_points), torch.int32), t(a), t(b)
    n_work = int(ctx.lib.anet_firi_workspace(B, max_points, H))

    def run(work):
        out = dict(hpoly=torch.empty((B, H, 4), device=dev, dtype=torch.float64), ellipsoid=torch.empty((B, 15), device=dev, dtype=torch.float64),
                   n_rows=torch.empty(B, device=dev, dtype=torch.int32), ok=torch.empty(B, device=dev, dtype=torch.int32))
        ctx.check(ctx.lib.anet_firi_dev(ctx.handle, B, bd.shape[1], max_points, H, _vp(tbd), _vp(tpc) if max_points else None,
                                        _vp(tnp) if max_points else None, _vp(ta), _vp(tb), None, _vp(work), _vp(out["hpoly"]),
                                        _vp(out["n_rows"]), _vp(out["ok"]), _vp(out["ellipsoid"]),
                                        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return out
    return n_work, run, {}


def _cases(aa):
    L = aa.lbfgs
    return {
        "qp_ipm": (lambda *a: _qp_case(*a, 3, aa.qp.QP_METHOD_INTERIOR_POINT), BITWISE),
        "qp_admm": (lambda *a: _qp_case(*a, 3, aa.qp.QP_METHOD_ADMM), ADMM_TOL),
        "qp_ipm_two_launches": (lambda *a: _qp_case(*a, 5, aa.qp.QP_METHOD_INTERIOR_POINT), BITWISE),
        "lbfgs_both": (lambda *a: _lbfgs_case(*a, 2, 3, L.OPT_WAYPOINTS | L.OPT_TIMES, 200), BITWISE),
        "lbfgs_waypoints": (lambda *a: _lbfgs_case(*a, 2, 3, L.OPT_WAYPOINTS, 200), BITWISE),
        "lbfgs_times": (lambda *a: _lbfgs_case(*a, 2, 3, L.OPT_TIMES, 200), BITWISE),
        "lbfgs_two_launches": (lambda *a: _lbfgs_case(*a, 10, 5, L.OPT_WAYPOINTS | L.OPT_TIMES, 60), BITWISE),
        "lbfgs_lockstep": (lambda *a: _lbfgs_case(*a, 2, 3, L.OPT_WAYPOINTS | L.OPT_TIMES | L.OPT_LOCKSTEP, 200), LOCKSTEP_TOL),
        "cost_grad_2": (lambda *a: _cost_grad_case(*a, 2), BITWISE),
        "cost_grad_3": (lambda *a: _cost_grad_case(*a, 3), BITWISE),
        "cost_grad_4": (lambda *a: _cost_grad_case(*a, 4), BITWISE),
        "firi_no_points": (lambda *a: _firi_case(*a, 0), FIRI_TOL),
        "firi_points": (lambda *a: _firi_case(*a, 5), FIRI_TOL),
    }


def run_case(name):
    """One case in this process: bands untouched?, per output the largest difference between the exact-size and the double-size
    workspace relative to the output's largest magnitude, whether the bits agree, and what the case reports about its form."""
    import torch
    import allocnet_amd as aa
    ctx = aa.default_context(0)
    dev = torch.device("cuda", 0)
    build, tol = _cases(aa)[name]
    n_work, run, info = build(aa, ctx, torch, dev)
    buf = torch.full((n_work + 2 * GUARD,), SENTINEL, device=dev, dtype=torch.int64)
    got = {k: v.cpu().numpy() for k, v in run(buf[GUARD:GUARD + n_work].view(torch.float64)).items()}
    torch.cuda.synchronize()
    bands = bool((buf[:GUARD] == SENTINEL).all().item() and (buf[GUARD + n_work:] == SENTINEL).all().item())
    big = torch.full((2 * n_work,), SENTINEL, device=dev, dtype=torch.int64)
    ref = {k: v.cpu().numpy() for k, v in run(big.view(torch.float64)).items()}
    diff, bits, close = {}, {}, {}
    for k in ref:
        bits[k] = bool(np.array_equal(got[k], ref[k], equal_nan=got[k].dtype.kind == "f"))
        close[k] = bool(np.allclose(got[k], ref[k], rtol=tol[1], atol=tol[1] / 100, equal_nan=True))
        both = np.isfinite(ref[k].astype(np.float64)) & np.isfinite(got[k].astype(np.float64))
        same_kind = bool(np.array_equal(np.isfinite(got[k].astype(np.float64)), np.isfinite(ref[k].astype(np.float64))))
        d = np.abs(got[k].astype(np.float64) - ref[k].astype(np.float64))[both]
        diff[k] = (float(d.max()) / max(1.0, float(np.abs(ref[k][both]).max())) if d.size else 0.0) if same_kind else float("inf")
    return dict(name=name, n_work=n_work, bands=bands, diff=diff, bits=bits, close=close, tol=list(tol), info=info)


def _verdict(r):
    print(json.dumps(r))            # (every figure before the assertion)
    assert r["bands"], "a guard band around the workspace of %d doubles was written" % r["n_work"]
    kind, bound = r["tol"]
    for k, ok in r["bits"].items():
        if kind == "bits" or k in ("status", "iters", "evals", "n_rows", "ok"):
            assert ok, (r["name"], k, r["diff"][k])
        elif kind == "allclose":
            assert r["close"][k], (r["name"], k, r["diff"][k])
        else:
            assert r["diff"][k] <= bound, (r["name"], k, r["diff"][k])


def _child(name, env_over, timeout=300):
    """The case in a fresh python with these switches; a child that fails or runs out of time fails the test here."""
    code = "import sys, json; sys.path.insert(0, %r); from tests.test_workspace_exact_gpu import run_case; print(json.dumps(run_case(%r)))" % (ROOT, name)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **env_over))
    assert p.returncode == 0, (name, env_over, p.returncode, p.stdout[-1000:], p.stderr[-3000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("name", ["qp_ipm", "qp_admm", "lbfgs_both", "lbfgs_waypoints", "lbfgs_times", "lbfgs_lockstep",
                                  "cost_grad_2", "cost_grad_3", "cost_grad_4", "firi_no_points", "firi_points"])
def test_exact_workspace_default_forms(anet_ctx, name):
    r = run_case(name)
    if name == "cost_grad_3" or name == "cost_grad_4":
        assert r["info"]["launches"] == 1
    _verdict(r)


def test_exact_workspace_qp_two_launch_form():
    r = _child("qp_ipm_two_launches", dict(ANET_IPM_SPLIT_MIN_BATCH="1", ANET_IPM_TWO_PER_CU_MIN_BATCH="1"))
    assert r["info"]["form"] & 0x20, r["info"]        # ANET_QP_IPM_FORM_TWO_LAUNCHES
    _verdict(r)


def test_exact_workspace_lbfgs_two_launch_form():
    _verdict(_child("lbfgs_two_launches", dict(ANET_LBFGS_SPLIT_MIN_BATCH="1", ANET_LBFGS_SPLIT_EVALS="20")))


@pytest.mark.parametrize("s", [2, 3, 4])
def test_exact_workspace_cost_grad_in_three_launches(s):
    r = _child("cost_grad_%d" % s, dict(ANET_FUSED_MAX_GROUPS="0"))
    assert r["info"]["launches"] == 3
    _verdict(r)
