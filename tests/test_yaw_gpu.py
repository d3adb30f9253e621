"""Yaw trajectories on the device (anet_minco_solve_scalar[_dev], anet_minco_propagate_grad_scalar_dev,
anet_minco_yaw_partial_grads_dev, anet_traj_yaw_margin[_dev], anet_traj_states_yaw and the facades) against the restatement of
tests/yaw_np.py: the one-axis MINCO against the collocation solve and against the three-axis kernels, the penalty's values and
contracts, the sampled margin, flat states with the yaw, the composed objective end to end and under the lockstep L-BFGS, and the
C++ facade.  The cases are those of tests/test_yaw_cpu.py (make_case), where their conditions are asserted without a GPU."""
import ctypes
import json
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import yaw_np as yn
from tests.test_voxel_distance_gpu import DEV, _bm
from tests.test_yaw_cpu import GPU_SHAPES, SPEED_EPS, make_case

pytestmark = pytest.mark.gpu


class Case:
    _cache = {}

    def __init__(self, name):
        self.s, self.sy, self.N, self.B, self.res = GPU_SHAPES[name]
        self.co, self.cy, self.T, self.kw, self.frac_look, self.frac_rate = make_case(*GPU_SHAPES[name], seed=1)
        self.ref = yn.j_yaw_grads(self.co, self.cy, self.T, **self.kw)

    @classmethod
    def get(cls, name):
        """the case of a shape, and its reference, computed once and shared (never written to)"""
        if name not in cls._cache:
            cls._cache[name] = cls(name)
        return cls._cache[name]

    def penalty(self, **over):
        import allocnet_amd as aa
        k = dict(self.kw, **over)
        return aa.make_yaw_penalty(**k)

    def device(self, ld=None, co=None, cy=None, T=None):
        import allocnet_amd as aa
        co, cy, T = (self.co if co is None else co), (self.cy if cy is None else cy), (self.T if T is None else T)
        B = len(T)
        ld = ld or (aa.recommended_ld(B) if B > 1 else 1)
        return dict(ld=ld, B=B, co=_bm(co.reshape(B, -1), ld), cy=_bm(cy.reshape(B, -1), ld), T=_bm(T, ld, fill=1.0))

    def launch(self, anet_ctx, d=None, pen=None, accumulate=False, into=None, fill=float("nan")):
        """-> the device tensors gdC, gdCy, gdT, piece_cost (whole rows, padding lanes included)."""
        import allocnet_amd as aa
        d = d or self.device()
        ld = d["ld"]
        if into is None:
            into = tuple(torch.full(shape, fill, dtype=torch.float64, device=DEV)
                         for shape in ((self.N * 3 * 2 * self.s, ld), (self.N * 2 * self.sy, ld), (self.N, ld), (self.N, ld)))
        aa.minco_yaw_partial_grads_dev(pen or self.penalty(), self.s, self.sy, self.N, d["B"], d["co"], d["cy"], d["T"], into[0],
                                       into[1], into[2], into[3], accumulate=accumulate, ctx=anet_ctx)
        torch.cuda.synchronize()
        return into

    def numpy(self, out, B=None):
        """-> piece_cost (B, N), gdC (B, N, 3, D), gdCy (B, N, DY), gdT (B, N): the order of the restatement"""
        B, N = B or self.B, self.N
        gC, gCy, gT, pc = out
        t = lambda x: x[:, :B].T.cpu().numpy()
        return t(pc), t(gC).reshape(B, N, 3, 2 * self.s), t(gCy).reshape(B, N, 2 * self.sy), t(gT)


def _scaled(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


# ---------------------------------------------------------------------------------------------
# the penalty against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GPU_SHAPES))
def test_kernel_matches_the_restatement(anet_ctx, name):
    """cost 1e-9 relative; gdC, gdCy and gdT 1e-7 scaled by max(1, max|ref|): the bars of the obstacle and stop terms.  No reference
    block is all zero; the z rows of gdC are exactly zero."""
    case = Case.get(name)
    d = case.device()
    assert d["ld"] > case.B or name != "wide"
    pc, gC, gCy, gT = case.numpy(case.launch(anet_ctx, d=d))
    rpc, rgC, rgCy, rgT = case.ref
    cost, rcost = pc.sum(1), rpc.sum(1)
    rel = np.abs(cost - rcost) / np.abs(rcost)
    errs = {n: _scaled(g, r) for n, g, r in (("gdC", gC, rgC), ("gdCy", gCy, rgCy), ("gdT", gT, rgT))}
    print(f"{name} (s={case.s}, sy={case.sy}) cost: worst relative {rel.max():.3e} (bar 1e-9); " +
          ", ".join(f"{n}: {e:.3e}" for n, e in errs.items()) + f" (bar 1e-7); max |ref| {np.abs(rgC).max():.3e}, "
          f"{np.abs(rgCy).max():.3e}, {np.abs(rgT).max():.3e}; look active {100 * case.frac_look:.0f} %, rate {100 * case.frac_rate:.0f} %")
    assert (rcost > 0.0).all() and all(np.abs(r).max() > 0.0 for r in (rgC[:, :, 0], rgC[:, :, 1], rgCy, rgT))
    assert (gC[:, :, 2] == 0.0).all() and (rgC[:, :, 2] == 0.0).all()
    assert rel.max() <= 1e-9
    assert all(e <= 1e-7 for e in errs.values()), errs


@pytest.mark.parametrize("name", ["quad", "top"])
def test_each_weight_disables_exactly_its_own_part(anet_ctx, name):
    """w_look = 0, then w_rate = 0, then w_energy = 0: the outputs are the restatement's with that weight at 0 (and differ from the
    full ones); with w_look = 0 the position gradient is exactly zero; all three zero give exact zeros everywhere."""
    case = Case.get(name)
    full = case.numpy(case.launch(anet_ctx))
    for off in ("w_look", "w_rate", "w_energy"):
        got = case.numpy(case.launch(anet_ctx, pen=case.penalty(**{off: 0.0})))
        ref = yn.j_yaw_grads(case.co, case.cy, case.T, **dict(case.kw, **{off: 0.0}))
        rel = np.abs(got[0].sum(1) - ref[0].sum(1)) / np.abs(ref[0].sum(1))
        errs = [_scaled(g, r) for g, r in zip(got[1:], ref[1:])]
        print(f"{name} {off} = 0: cost {rel.max():.3e}, gradients {max(errs):.3e}")
        assert rel.max() <= 1e-9 and max(errs) <= 1e-7
        assert not np.array_equal(got[0], full[0]) and not np.array_equal(got[2], full[2])
        if off == "w_look":
            assert (got[1] == 0.0).all()
    none = case.numpy(case.launch(anet_ctx, pen=case.penalty(w_look=0.0, w_rate=0.0, w_energy=0.0)))
    assert all((x == 0.0).all() for x in none)


@pytest.mark.parametrize("name", ["ragged", "rounds"])
def test_accumulate_adds_the_complete_share(anet_ctx, name):
    """After anet_minco_partial_grads_dev the accumulated gdC, gdT and piece_cost equal the sum of the two separate results to the
    last bit; gdCy is overwritten either way."""
    import allocnet_amd as aa
    case = Case.get(name)
    d = case.device()
    s, N, B, ld = case.s, case.N, case.B, d["ld"]
    pen = aa.make_penalty(rho=0.0, w_vel=10.0, w_acc=5.0, smooth_mu=0.05, max_vel=0.3, max_acc=0.5, res=7)
    base = tuple(torch.zeros(shape, dtype=torch.float64, device=DEV) for shape in ((N * 3 * 2 * s, ld), (N, ld), (N, ld)))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    anet_ctx.check(anet_ctx.lib.anet_minco_partial_grads_dev(anet_ctx.handle, s, N, B, ld, p(d["co"]), p(d["T"]), None,
                                                             ctypes.cast(ctypes.pointer(pen), ctypes.c_void_p), 1, p(base[0]),
                                                             p(base[1]), p(base[2]), st))
    torch.cuda.synchronize()
    assert all(float(x[:, :B].abs().max()) > 0.0 for x in base[:2])
    own = case.launch(anet_ctx, d=d)
    acc = (base[0].clone(), torch.full_like(own[1], 123.0), base[1].clone(), base[2].clone())
    case.launch(anet_ctx, d=d, accumulate=True, into=acc)
    for what, a, x, y in (("gdC", acc[0], base[0], own[0]), ("gdT", acc[2], base[1], own[2]), ("piece_cost", acc[3], base[2], own[3])):
        assert torch.equal(a[:, :B], (x + y)[:, :B]), what
    assert torch.equal(acc[1][:, :B], own[1][:, :B])
    if ld > B:
        assert torch.equal(acc[0][:, B:], base[0][:, B:]) and (acc[1][:, B:] == 123.0).all()


@pytest.mark.parametrize("name", ["ragged", "rounds", "wide"])
def test_same_bits_alone_in_a_batch_and_at_another_ld(anet_ctx, name):
    case = Case.get(name)
    whole = case.launch(anet_ctx)
    other = case.launch(anet_ctx, d=case.device(ld=case.B + 13))
    b = case.B - 1
    alone = case.launch(anet_ctx, d=case.device(co=case.co[b:b + 1], cy=case.cy[b:b + 1], T=case.T[b:b + 1]))
    for w, o, a in zip(whole, other, alone):
        assert torch.equal(w[:, :case.B], o[:, :case.B])
        assert torch.equal(w[:, b], a[:, 0])
    assert all(torch.isnan(o[:, case.B:]).all() for o in other)      # lanes in [batch, ld) are never touched


def test_nan_isolation(anet_ctx):
    """A non-finite position coefficient (a z one among them), a non-finite yaw coefficient, a duration <= 0 or not finite of
    trajectory b: all outputs of b are NaN, and only those."""
    case = Case.get("quad")
    clean = case.launch(anet_ctx)
    poisons = [("co", (1, 2, 0, 3), np.nan), ("co", (0, 1, 2, 0), np.inf), ("cy", (3, 0, 1), np.nan), ("cy", (2, 3, 5), -np.inf),
               ("T", (4, 1), 0.0), ("T", (1, 3), -0.5), ("T", (0, 0), np.inf), ("T", (2, 2), np.nan)]
    for what, idx, val in poisons:
        arrs = dict(co=case.co.copy(), cy=case.cy.copy(), T=case.T.copy())
        arrs[what][idx] = val
        out = case.launch(anet_ctx, d=case.device(**arrs), fill=5.0)
        b = idx[0]
        keep = [x for x in range(case.B) if x != b]
        for o, c in zip(out, clean):
            assert torch.isnan(o[:, b]).all(), (what, idx, val)
            assert torch.equal(o[:, keep], c[:, keep]), (what, idx, val)


def test_error_codes(anet_ctx):
    """ANET_ERR_UNSUPPORTED for an order 1 or 5 of either polynomial; ANET_ERR_INVALID for half_fov 0 or 2, a NULL pointer other
    than the optional outputs, ld < batch; batch == 0 touches nothing."""
    from allocnet_amd._lib import ANET_ERR_INVALID, ANET_ERR_UNSUPPORTED, ANET_OK
    case = Case.get("ragged")
    s, sy, N, B = case.s, case.sy, case.N, case.B
    d = case.device()
    ld = d["ld"]
    lib, h = anet_ctx.lib, anet_ctx.handle
    q = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    ref = lambda p: ctypes.cast(ctypes.pointer(p), ctypes.c_void_p)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gC = torch.full((N * 3 * 2 * s, ld), 7.0, dtype=torch.float64, device=DEV)
    gCy = torch.full((N * 2 * sy, ld), 7.0, dtype=torch.float64, device=DEV)
    gT, pc, m = (torch.full((N, ld), 7.0, dtype=torch.float64, device=DEV) for _ in range(3))
    host = dict(co=np.ascontiguousarray(case.co), cy=np.ascontiguousarray(case.cy), T=np.ascontiguousarray(case.T), m=np.empty((B, N)))
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None

    def grads(pen=None, s_=s, sy_=sy, N_=N, B_=B, ld_=ld, co=d["co"], cy=d["cy"], T=d["T"], out=gC, outy=gCy, outT=gT):
        return lib.anet_minco_yaw_partial_grads_dev(h, ref(pen or case.penalty()), s_, sy_, N_, B_, ld_, q(co), q(cy), q(T), 0, q(out),
                                                    q(outy), q(outT), q(pc), st)

    def margin_dev(pen=None, s_=s, sy_=sy, N_=N, B_=B, ld_=ld, co=d["co"], cy=d["cy"], T=d["T"], out=m, **_):
        return lib.anet_traj_yaw_margin_dev(h, ref(pen or case.penalty()), 0.1, s_, sy_, N_, B_, ld_, q(co), q(cy), q(T), q(out), None,
                                            None, st)

    def margin_host(pen=None, s_=s, sy_=sy, N_=N, B_=B, co=host["co"], cy=host["cy"], T=host["T"], out=host["m"], **_):
        return lib.anet_traj_yaw_margin(h, ref(pen or case.penalty()), 0.1, s_, sy_, N_, B_, hp(co), hp(cy), hp(T), hp(out), None, None)
    for fn in (grads, margin_dev, margin_host):
        assert fn() == ANET_OK
        for bad in (1, 5):
            assert fn(s_=bad) == ANET_ERR_UNSUPPORTED and fn(sy_=bad) == ANET_ERR_UNSUPPORTED, fn.__name__
        for fov in (0.0, 2.0):
            assert fn(pen=case.penalty(half_fov=fov)) == ANET_ERR_INVALID, fn.__name__
        assert fn(N_=0) == ANET_ERR_INVALID and fn(N_=17) == ANET_ERR_INVALID
        for arg in ("co", "cy", "T", "out"):
            assert fn(**{arg: None}) == ANET_ERR_INVALID, (fn.__name__, arg)
        assert fn(pen=case.penalty(res=0)) == ANET_ERR_INVALID
    for fn in (grads, margin_dev):
        assert fn(ld_=B - 1) == ANET_ERR_INVALID
    assert grads(outy=None) == ANET_ERR_INVALID and grads(outT=None) == ANET_ERR_INVALID
    for over in (dict(w_look=-1.0), dict(mu_look=0.0), dict(speed_eps=0.0), dict(mu_rate=0.0), dict(max_rate=0.0), dict(w_energy=-1.0),
                 dict(w_rate=float("inf"))):
        assert grads(pen=case.penalty(**over)) == ANET_ERR_INVALID, over
    assert grads(pen=case.penalty(max_rate=float("inf"))) == ANET_OK
    assert grads(pen=case.penalty(w_look=0.0, mu_look=0.0, speed_eps=0.0)) == ANET_OK        # not read when the weight is 0
    torch.cuda.synchronize()
    gC.fill_(7.0); gCy.fill_(7.0); gT.fill_(7.0); m.fill_(7.0)
    assert grads(B_=0) == ANET_OK and margin_dev(B_=0) == ANET_OK
    torch.cuda.synchronize()
    assert all((x == 7.0).all() for x in (gC, gCy, gT, m))
    # the one-axis MINCO: the checks of anet_minco_solve_dev
    hd, T1 = torch.zeros(2, 4, dtype=torch.float64, device=DEV), torch.ones(3, 4, dtype=torch.float64, device=DEV)
    w1, c1 = torch.zeros(2, 4, dtype=torch.float64, device=DEV), torch.zeros(3 * 4, 4, dtype=torch.float64, device=DEV)
    solve = lambda s_=2, c_=2, N_=3, B_=4, ld_=4, hd_=hd, w_=w1: lib.anet_minco_solve_scalar_dev(h, s_, c_, N_, B_, ld_, q(hd_), q(hd),
                                                                                                q(w_), q(T1), q(c1), None, st)
    assert solve() == ANET_OK
    assert [solve(s_=1), solve(s_=5), solve(c_=3), solve(N_=17), solve(ld_=3), solve(hd_=None), solve(w_=None)] == [ANET_ERR_INVALID] * 7
    gT1 = torch.zeros_like(T1)
    prop = lambda gd=c1, gp=w1: lib.anet_minco_propagate_grad_scalar_dev(h, 2, 2, 3, 4, 4, q(T1), q(c1), q(gd), None, q(gp), q(gT1), st)
    assert prop() == ANET_OK and prop(gd=None) == ANET_ERR_INVALID and prop(gp=None) == ANET_ERR_INVALID
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# the one-axis MINCO
# ---------------------------------------------------------------------------------------------
def _scalar_problem(s, c, N, B, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(B, c)), rng.normal(size=(B, c)), rng.normal(size=(B, N - 1)) * 1.5, rng.uniform(0.6, 1.6, (B, N))


def _embed(head, tail, wps):
    """the one-axis data as axis 0 of a three-axis problem, zeros in the other two"""
    B, c = head.shape
    h3, t3, w3 = np.zeros((B, 3, c)), np.zeros((B, 3, c)), np.zeros((B, wps.shape[1], 3))
    h3[:, 0], t3[:, 0], w3[:, :, 0] = head, tail, wps
    return h3, t3, w3


@pytest.mark.parametrize("s", [2, 3, 4])
def test_scalar_minco_solve(anet_ctx, s):
    """c = 1..s, N in {1, 2, 16}, B in {1, 65}: coefficients and energy within 1e-9 (scaled by max(1, max|ref|)) of the collocation
    restatement, the bar of tests/test_minco_gpu.py, and within 1e-12 scaled of anet_minco_solve_dev with the yaw data in axis 0
    and zeros in the other two.  The host form agrees with the device form to the bit.  Where 2 c + N - 1 < s the problem has no
    unique minimiser (fewer conditions than the order: every polynomial of degree < s through them has zero effort) and the
    collocation matrix is singular: those shapes -- (c, N) = (1, 1) at s = 3; (1, 1), (1, 2) at s = 4 -- are held to the three-axis
    kernel alone."""
    import allocnet_amd as aa
    worst_ref, worst_3, bitwise = 0.0, 0.0, []
    for c in range(1, s + 1):
        for N in (1, 2, 16):
            for B in (1, 65):
                head, tail, wps, T = _scalar_problem(s, c, N, B, seed=100 * s + 10 * c + N)
                ld = aa.recommended_ld(B) if B > 1 else 1
                d_T = _bm(T, ld, fill=1.0)
                co, en = aa.minco_solve_scalar_dev(_bm(head, ld), _bm(tail, ld), _bm(wps, ld) if N > 1 else None, d_T, s, c, N, B,
                                                   ctx=anet_ctx)
                torch.cuda.synchronize()
                co, en = co[:, :B].T.cpu().numpy().reshape(B, N, 2 * s), en[:B].cpu().numpy()
                hco, hen = aa.minco_solve_scalar(head, tail, wps, T, s, ctx=anet_ctx)
                assert np.array_equal(hco, co) and np.array_equal(hen, en)
                for b in range((B if B == 1 else 3) if 2 * c + N - 1 >= s else 0):
                    rco, ren = yn.minco_scalar(s, head[b], tail[b], wps[b], T[b])
                    worst_ref = max(worst_ref, _scaled(co[b], rco), abs(en[b] - ren) / max(1.0, abs(ren)))
                h3, t3, w3 = _embed(head, tail, wps)
                co3, en3 = aa.minco_solve(h3, t3, w3, T, s, ctx=anet_ctx)
                assert (co3[:, :, 1:] == 0.0).all()
                worst_3 = max(worst_3, _scaled(co, co3[:, :, 0]), _scaled(en, en3))
                bitwise.append(np.array_equal(co, co3[:, :, 0]) and np.array_equal(en, en3))
    print(f"s = {s}: against the collocation solve {worst_ref:.3e} (bar 1e-9); against anet_minco_solve {worst_3:.3e} (bar 1e-12), "
          f"to the bit in {sum(bitwise)} of {len(bitwise)} shapes")
    assert worst_ref <= 1e-9 and worst_3 <= 1e-12


@pytest.mark.parametrize("s", [2, 3, 4])
def test_scalar_adjoint(anet_ctx, s):
    """Within 1e-12, scaled, of anet_minco_propagate_grad_dev on the same embedding (random gdC in axis 0, zeros in the other two);
    gdT = NULL equals gdT = zeros to the bit."""
    import allocnet_amd as aa
    worst = 0.0
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    for c in range(1, s + 1):
        for N in (1, 2, 16):
            for B in (1, 65):
                head, tail, wps, T = _scalar_problem(s, c, N, B, seed=200 * s + 10 * c + N)
                rng = np.random.default_rng(N + B)
                gdC, gdT = rng.normal(size=(B, N, 2 * s)), rng.normal(size=(B, N))
                ld = aa.recommended_ld(B) if B > 1 else 1
                d_T = _bm(T, ld, fill=1.0)
                co, _ = aa.minco_solve_scalar_dev(_bm(head, ld), _bm(tail, ld), _bm(wps, ld) if N > 1 else None, d_T, s, c, N, B,
                                                  ctx=anet_ctx)
                d_gC, d_gT = _bm(gdC.reshape(B, -1), ld), _bm(gdT, ld)
                gP, gT = aa.minco_propagate_grad_scalar_dev(d_T, co, d_gC, d_gT, s, c, N, B, ctx=anet_ctx)
                gP0, gT0 = aa.minco_propagate_grad_scalar_dev(d_T, co, d_gC, torch.zeros_like(d_gT), s, c, N, B, ctx=anet_ctx)
                gPn, gTn = aa.minco_propagate_grad_scalar_dev(d_T, co, d_gC, None, s, c, N, B, ctx=anet_ctx)
                torch.cuda.synchronize()
                assert torch.equal(gP0[:, :B], gPn[:, :B]) and torch.equal(gT0[:, :B], gTn[:, :B])
                # the three-axis adjoint on the embedding
                h3, t3, w3 = _embed(head, tail, wps)
                co3 = np.zeros((B, N, 3, 2 * s))
                co3[:, :, 0] = co[:, :B].T.cpu().numpy().reshape(B, N, 2 * s)
                g3 = np.zeros((B, N, 3, 2 * s))
                g3[:, :, 0] = gdC
                gP3 = torch.zeros(max(3 * (N - 1), 1), ld, dtype=torch.float64, device=DEV)
                gT3 = torch.zeros(N, ld, dtype=torch.float64, device=DEV)
                st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                d_co3, d_g3 = _bm(co3.reshape(B, -1), ld), _bm(g3.reshape(B, -1), ld)
                anet_ctx.check(anet_ctx.lib.anet_minco_propagate_grad_dev(anet_ctx.handle, s, c, N, B, ld, p(d_T), p(d_co3), p(d_g3),
                                                                          p(d_gT), p(gP3), p(gT3), st))
                torch.cuda.synchronize()
                worst = max(worst, _scaled(gT[:, :B].cpu().numpy(), gT3[:, :B].cpu().numpy()))
                if N > 1:
                    ref = gP3[:3 * (N - 1), :B].cpu().numpy().reshape(N - 1, 3, B)
                    assert np.abs(ref[:, 0]).max() > 0.0
                    worst = max(worst, _scaled(gP[:N - 1, :B].cpu().numpy(), ref[:, 0]))
    print(f"s = {s}: against anet_minco_propagate_grad_dev {worst:.3e} (bar 1e-12)")
    assert worst <= 1e-12


# ---------------------------------------------------------------------------------------------
# the sampled margin
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GPU_SHAPES))
def test_margin_matches_the_restatement(anet_ctx, name):
    """margin and t within 1e-12 scaled by max(1, pi); rate within 1e-12 scaled by max(1, max|rate|) -- it is no angle: a Horner
    value of a polynomial whose coefficients are not bounded by pi, so its rounding error scales with its size (4500 ulps, the
    project's bar for one evaluation against numpy).  The host form equals the device form to the bit."""
    import allocnet_amd as aa
    case = Case.get(name)
    v_min = 0.15
    half_fov = case.kw["half_fov"]
    ref = yn.yaw_margin(case.co, case.cy, case.T, case.res, half_fov, v_min)
    d = case.device()
    dev = aa.traj_yaw_margin_dev(case.penalty(), v_min, case.s, case.sy, case.N, case.B, d["co"], d["cy"], d["T"], ctx=anet_ctx)
    torch.cuda.synchronize()
    dev = [x[:, :case.B].T.cpu().numpy() for x in dev]
    host = aa.traj_yaw_margin(case.co, case.cy, case.T, half_fov, v_min, case.res, ctx=anet_ctx)
    errs = []
    for what, g, hst, r in zip(("margin", "t", "rate"), dev, host, ref):
        assert np.array_equal(g, hst), what
        assert np.array_equal(np.isinf(g), np.isinf(r)), what
        fin = np.isfinite(r)
        scale = max(1.0, np.abs(r[fin]).max()) if what == "rate" else max(1.0, np.pi)
        errs.append(float(np.abs(g[fin] - r[fin]).max() / scale) if fin.any() else 0.0)
    print(f"{name}: margin {errs[0]:.3e}, t {errs[1]:.3e}, rate {errs[2]:.3e} (bar 1e-12); least margin {np.nanmin(ref[0]):.4f} rad, peak rate {np.nanmax(ref[2]):.3e} rad/s, "
          f"{int(np.isinf(ref[0]).sum())} pieces without a counted sample")
    assert max(errs) <= 1e-12


def test_margin_of_a_piece_at_rest_and_of_a_bad_piece(anet_ctx):
    """A piece at rest has no counted sample at v_min > 0: +inf and time 0, the rate still reported; at v_min = 0 every sample counts
    (a sample at rest has no direction: its angle is 0 and its margin half_fov).  A non-finite coefficient or a duration <= 0 gives NaN for that piece only."""
    import allocnet_amd as aa
    case = Case.get("ragged")
    co, cy, T = case.co.copy(), case.cy.copy(), case.T.copy()
    co[1, 2, :, :-1] = 0.0
    half_fov = 0.6
    m, t, r = aa.traj_yaw_margin(co, cy, T, half_fov, 0.2, case.res, ctx=anet_ctx)
    ref = yn.yaw_margin(co, cy, T, case.res, half_fov, 0.2)
    assert m[1, 2] == np.inf and t[1, 2] == 0.0 and abs(r[1, 2] - ref[2][1, 2]) <= 1e-12 and ref[2][1, 2] > 0.0
    assert np.isfinite(np.delete(m.reshape(-1), 1 * case.N + 2)).all()
    m0 = aa.traj_yaw_margin(co, cy, T, half_fov, 0.0, case.res, ctx=anet_ctx)[0]
    assert m0[1, 2] == half_fov
    co[0, 1, 2, 3], cy[2, 0, 1], T[1, 4] = np.nan, np.inf, 0.0
    out = aa.traj_yaw_margin(co, cy, T, half_fov, 0.2, case.res, ctx=anet_ctx)
    bad = np.zeros((case.B, case.N), dtype=bool)
    bad[0, 1] = bad[2, 0] = bad[1, 4] = True
    for o in out:
        assert np.array_equal(np.isnan(o), bad)


# ---------------------------------------------------------------------------------------------
# flat states with the yaw
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quad", "ragged", "top"])
def test_flat_states_with_the_yaw(anet_ctx, name):
    """Against the pointwise flat_forward fed with traj_eval's v, a, j and the restatement's psi, dpsi: 1e-12 scaled by
    max(1, max|ref|) per field group; with a zero yaw polynomial against traj_flat_states on the same inputs: 1e-12."""
    import allocnet_amd as aa
    case = Case.get(name)
    B, N = case.B, case.N
    fm = aa.make_flat_params()
    rng = np.random.default_rng(5)
    total = case.T.sum(1)
    tq = np.concatenate([rng.uniform(0.0, 1.0, (B, 6)) * total[:, None], np.zeros((B, 1)), total[:, None], case.T[:, :1]], 1)
    out = aa.traj_flat_states_yaw(fm, case.co, case.cy, case.T, tq, ctx=anet_ctx)
    v, a, j = (aa.traj_eval(case.co, case.T, tq, k, ctx=anet_ctx).reshape(-1, 3) for k in (1, 2, 3))
    psi, dpsi = yn.yaw_eval(case.cy, case.T, tq)
    thr, quat, omg = aa.flat_forward(fm, v, a, j, psi.reshape(-1), dpsi.reshape(-1), ctx=anet_ctx)
    got = out.reshape(-1, 11)
    errs = dict(thr=_scaled(got[:, 0], np.asarray(thr).reshape(-1)), quat=_scaled(got[:, 1:5], np.asarray(quat).reshape(-1, 4)),
                omg=_scaled(got[:, 5:8], np.asarray(omg).reshape(-1, 3)), speed=_scaled(got[:, 8], np.sqrt((v * v).sum(1))),
                bdr=_scaled(got[:, 10], np.sqrt((np.asarray(omg).reshape(-1, 3) ** 2).sum(1))))
    zero = aa.traj_flat_states_yaw(fm, case.co, np.zeros_like(case.cy), case.T, tq, ctx=anet_ctx)
    plain = aa.traj_flat_states(fm, case.co, case.T, tq, ctx=anet_ctx)
    errs["psi = 0"] = float(np.abs(zero - plain).max())
    print(f"{name}: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()) + " (bar 1e-12)")
    assert np.abs(psi).max() > 0.1 and np.abs(out[..., 1:5] - plain[..., 1:5]).max() > 1e-3       # the yaw does turn the attitude
    assert np.abs(out[..., 9] - plain[..., 9]).max() <= 1e-12                                    # ... and leaves the tilt alone
    assert all(e <= 1e-12 for e in errs.values()), errs


# ---------------------------------------------------------------------------------------------
# composed
# ---------------------------------------------------------------------------------------------
def _walk_problem(rng, B, N, c=3):
    """continuous random routes with PVA ends, the yaw's ends and waypoints at the tangent headings plus noise"""
    import allocnet_amd as aa
    steps = rng.normal(size=(B, N, 3)) * np.array([1.0, 1.0, 0.2]) + np.array([1.2, 0.0, 0.0])
    nodes = np.concatenate([np.zeros((B, 1, 3)), np.cumsum(steps, 1)], 1)
    head, tail = np.zeros((B, 3, c)), np.zeros((B, 3, c))
    head[:, :, 0], tail[:, :, 0] = nodes[:, 0], nodes[:, -1]
    head[:, :, 1], tail[:, :, 1] = rng.normal(size=(B, 3)) * 0.3, rng.normal(size=(B, 3)) * 0.3
    wps, T = nodes[:, 1:-1].copy(), rng.uniform(0.8, 1.6, (B, N))
    h0, hw, h1 = aa.heading_waypoints(wps, nodes[:, 0], nodes[:, -1])
    yhead, ytail = np.zeros((B, 2)), np.zeros((B, 2))
    yhead[:, 0], ytail[:, 0] = h0, h1
    return head, tail, wps, T, yhead, ytail, hw + 0.3 * rng.normal(size=hw.shape)


def test_minco_yaw_cost_grad_finite_differences(anet_ctx):
    """s = 4, sy = 2, N = 6, B = 8: the cost is minco_cost_grad + the restatement's J_yaw within 1e-9 relative; gradP, the
    yaw-waypoint gradient and gradT against central differences of the returned cost, h = 1e-6, bar 2e-5 scaled by max(1, max|g|).
    The limits follow the percentile rule on the solved trajectories; both terms are active on 10-90 % of the samples."""
    import allocnet_amd as aa
    s, sy, N, B, res = 4, 2, 6, 8, 20
    head, tail, wps, T, yhead, ytail, ywps = _walk_problem(np.random.default_rng(11), B, N)
    co, _ = aa.minco_solve(head, tail, wps, T, s, ctx=anet_ctx)
    cy, _ = aa.minco_solve_scalar(yhead, ytail, ywps, T, sy, ctx=anet_ctx)
    lim, frac_look, frac_rate = yn.limits_for(co, cy, T, res, SPEED_EPS)
    print(f"look active on {100 * frac_look:.1f} %, rate on {100 * frac_rate:.1f} %; {lim}")
    assert 0.1 <= frac_look <= 0.9 and 0.1 <= frac_rate <= 0.9
    kw = dict(res=res, w_look=30.0, w_rate=20.0, w_energy=0.0, speed_eps=SPEED_EPS, **lim)
    kw["w_energy"] = yn.energy_weight(co, cy, T, kw)
    ypen = aa.make_yaw_penalty(**kw)
    pen = aa.make_penalty(rho=2.0, w_vel=25.0, w_acc=9.0, smooth_mu=0.05, max_vel=1.5, max_acc=2.5, res=9)
    fn = lambda w, yw, t: aa.minco_yaw_cost_grad(head, tail, w, yhead, ytail, yw, t, s, sy, ypen, penalty=pen, ctx=anet_ctx)
    cost, gP, gPy, gT = fn(wps, ywps, T)
    base = aa.minco_cost_grad(head, tail, wps, T, s, penalty=pen, ctx=anet_ctx)[0]
    jy = yn.j_yaw(co, cy, T, **kw)
    assert (jy > 0.0).all()
    rel = np.abs(cost - (base + jy)) / np.abs(base + jy)
    print(f"cost against minco_cost_grad + J_yaw: worst relative {rel.max():.3e} (bar 1e-9); J_yaw / J between "
          f"{(jy / (base + jy)).min():.3f} and {(jy / (base + jy)).max():.3f}")
    assert rel.max() <= 1e-9
    h = 1e-6

    def check(what, fd, g):
        err = np.abs(fd - g).max() / max(1.0, np.abs(g).max())
        print(f"{what}: {err:.3e} (bar 2e-5), max |g| {np.abs(g).max():.3e}")
        assert err <= 2e-5
    for (k, ax) in [(0, 0), (2, 1), (4, 2)]:
        wp, wm = wps.copy(), wps.copy()
        wp[:, k, ax] += h
        wm[:, k, ax] -= h
        check(f"gradP[{k},{ax}]", (fn(wp, ywps, T)[0] - fn(wm, ywps, T)[0]) / (2 * h), gP[:, k, ax])
    for k in (0, 2, 4):
        yp, ym = ywps.copy(), ywps.copy()
        yp[:, k] += h
        ym[:, k] -= h
        check(f"gradPy[{k}]", (fn(wps, yp, T)[0] - fn(wps, ym, T)[0]) / (2 * h), gPy[:, k])
    for i in (0, 3, 5):
        tp, tm = T.copy(), T.copy()
        tp[:, i] += h
        tm[:, i] -= h
        check(f"gradT[{i}]", (fn(wps, ywps, tp)[0] - fn(wps, ywps, tm)[0]) / (2 * h), gT[:, i])


def test_lockstep_lbfgs_turns_the_heading_into_the_corner(anet_ctx):
    """Free space, no map: a rest-to-rest 4-piece jerk trajectory from (0, 0, 1) along +x to the corner (4, 0, 1) and along +y to
    (4, 4, 1), T = 1.5 each; yaw of order 2 with psi = 0 at the start (the first leg's direction) and pi / 2 at the end (the last
    leg's), every yaw waypoint at 0.  half_fov = 35 deg, max_rate = 1 rad/s, w_look = w_rate = 100, mu_look = 0.05 m/s,
    mu_rate = 0.05 (rad/s)^2, speed_eps = 0.01 m/s, w_energy = 0.01, rho = 1.  lbfgs_optimize_dev on yaw_objective_dev: every
    status >= 0, J_yaw falls by at least a factor 100, the worst look margin at v_min = 0.2 rises from below -0.5 rad to above
    -0.05 rad, and the peak sampled |dpsi| ends below 1.1 rad/s."""
    import allocnet_amd as aa
    s, c, sy, cy_, N, B, res = 3, 3, 2, 2, 4, 1, 20
    half_fov, max_rate, v_min = math.radians(35.0), 1.0, 0.2
    nodes = np.array([[[0.0, 0.0, 1.0], [2.0, 0.0, 1.0], [4.0, 0.0, 1.0], [4.0, 2.0, 1.0], [4.0, 4.0, 1.0]]])
    head, tail = np.zeros((B, 3, c)), np.zeros((B, 3, c))
    head[:, :, 0], tail[:, :, 0] = nodes[:, 0], nodes[:, -1]
    wps, T = nodes[:, 1:-1].copy(), np.full((B, N), 1.5)
    yhead, ytail, ywps = np.zeros((B, cy_)), np.zeros((B, cy_)), np.zeros((B, N - 1))
    ytail[:, 0] = 0.5 * np.pi
    kw = dict(res=res, w_look=100.0, mu_look=0.05, half_fov=half_fov, speed_eps=1e-2, w_rate=100.0, mu_rate=0.05, max_rate=max_rate,
              w_energy=0.01)
    ypen = aa.make_yaw_penalty(**kw)
    pen = aa.make_penalty(rho=1.0, res=res)

    def state(wp, yw, t):
        co, _ = aa.minco_solve(head, tail, wp, t, s, ctx=anet_ctx)
        cy, _ = aa.minco_solve_scalar(yhead, ytail, yw, t, sy, ctx=anet_ctx)
        jy = yn.j_yaw(co, cy, t, **kw)
        m, _, r = aa.traj_yaw_margin(co, cy, t, half_fov, v_min, res, ctx=anet_ctx)
        return dict(J_yaw=float(jy.sum()), margin=float(m.min()), rate=float(r.max()), total=float(t.sum())), co, cy
    before, co0, cy0 = state(wps, ywps, T)
    ld, nw, ny = 1, 3 * (N - 1), N - 1
    x = torch.zeros(nw + ny + N, ld, dtype=torch.float64, device=DEV)
    x[:nw, :B] = torch.from_numpy(wps.reshape(B, -1)).T.to(DEV)
    x[nw:nw + ny, :B] = torch.from_numpy(ywps).T.to(DEV)
    x[nw + ny:, :B] = torch.from_numpy(np.log(T)).T.to(DEV)
    ev = aa.yaw_objective_dev(_bm(head.reshape(B, -1), ld), _bm(tail.reshape(B, -1), ld), _bm(yhead, ld), _bm(ytail, ld), s, c, sy, cy_,
                              N, B, ypen, penalty=pen, ctx=anet_ctx)
    res_ = aa.lbfgs_optimize_dev(x, ev, batch=B, param=aa.lbfgs_parameter_t(past=3, delta=1e-5), max_evals=1500, ctx=anet_ctx)
    torch.cuda.synchronize()
    status = res_["status"].cpu().numpy()
    xs = x[:, :B].T.cpu().numpy()
    after, co1, cy1 = state(xs[:, :nw].reshape(B, N - 1, 3), xs[:, nw:nw + ny], np.exp(xs[:, nw + ny:]))
    print(f"status {status.tolist()}, evals {res_['evals'].cpu().numpy().tolist()}, iterations {res_['iters'].cpu().numpy().tolist()}")
    print("before", before)
    print("after ", after, "yaw waypoints", xs[0, nw:nw + ny].tolist(), "durations", np.exp(xs[0, nw + ny:]).tolist())
    assert (status >= 0).all()
    assert before["margin"] < -0.5 and before["J_yaw"] > 0.0
    assert after["J_yaw"] * 100.0 <= before["J_yaw"]
    assert after["margin"] > -0.05
    assert after["rate"] < 1.1
    # the facade of one trajectory reports the same margin
    traj = aa.Trajectory(T[0], co0[0], ctx=anet_ctx)
    yaw = aa.YawTrajectory(cy0[0], T[0])
    m, t, piece = traj.getYawMargin(yaw, half_fov, v_min, res)
    assert m == before["margin"] and 0 <= piece < N and 0.0 <= t <= T.sum() and not traj.checkYaw(yaw, half_fov, max_rate, v_min, res)


# ---------------------------------------------------------------------------------------------
# C++
# ---------------------------------------------------------------------------------------------
def test_cpp_facade_program(anet_ctx):
    """tests/cpp/test_yaw.cpp: MincoYaw<2>, getYawMargin and checkYaw on a three-piece quintic trajectory through the C ABI; the
    program compares margin, time, piece, energy, psi and dpsi at a query time with the restatement's numbers, given on its command
    line, within 1e-9 scaled; checkYaw turns at the margin and at the rate limit."""
    import allocnet_amd as aa
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, lib = os.path.join(root, "tests", "cpp", "test_yaw.cpp"), os.path.join(root, "allocnet_amd", "lib")
    half_fov, max_rate, v_min, res, tq = 0.5, 0.8, 0.1, 12, 1.7
    head, tail = np.zeros((1, 3, 3)), np.zeros((1, 3, 3))
    head[0, :, 0], tail[0, :, 0] = (-0.2, 0.8, 1.0), (4.2, 3.1, 2.4)
    wps = np.array([[[1.0, 1.5, 1.2], [2.6, 2.4, 1.9]]])
    T = np.array([[1.1, 0.9, 1.3]])
    co, _ = aa.minco_solve(head, tail, wps, T, 3, ctx=anet_ctx)
    h0, hw, h1 = aa.heading_waypoints(wps[0], head[0, :, 0], tail[0, :, 0])
    yhead, ytail, ywps = np.array([h0, 0.1]), np.array([h1, -0.2]), hw + np.array([0.3, -0.4])
    cy, energy = yn.minco_scalar(2, yhead, ytail, ywps, T[0])
    m, t, r = yn.yaw_margin(co, cy[None], T, res, half_fov, v_min)
    piece = int(m[0].argmin())
    psi, dpsi = yn.yaw_eval(cy[None], T, np.array([[tq]]))
    want = [m[0, piece], T[0, :piece].sum() + t[0, piece], piece, energy, psi[0, 0], dpsi[0, 0]]
    assert np.isfinite(m).all() and half_fov - m[0, piece] + 1e-3 <= 0.5 * np.pi and r.max() > 1e-3
    ok = bool((m >= 0.0).all() and (r <= max_rate).all())
    with tempfile.TemporaryDirectory() as td:
        exe, case = os.path.join(td, "test_yaw"), os.path.join(td, "case.txt")
        with open(case, "w") as fh:
            fh.write("%.17g %.17g %.17g %d %.17g %d\n" % (half_fov, max_rate, v_min, res, tq, T.shape[1]))
            for i in range(T.shape[1]):
                fh.write("%.17g " % T[0, i] + " ".join("%.17g" % x for x in co[0, i].reshape(-1)) + "\n")
            fh.write(" ".join("%.17g" % x for x in (*yhead, *ytail, *ywps)) + "\n")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"), src, "-o", exe,
                        "-L", lib, "-lallocnet_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
        res_ = subprocess.run([exe, case] + ["%.17g" % x if not isinstance(x, int) else str(x) for x in want], capture_output=True,
                              text=True, timeout=120)
    print(res_.stdout.strip())
    assert res_.returncode == 0, res_.stdout + res_.stderr
    out = json.loads(res_.stdout)
    assert out["piece"] == piece and abs(out["total"] - T.sum()) < 1e-12
    traj, yaw = aa.Trajectory(T[0], co[0], ctx=anet_ctx), aa.YawTrajectory(cy, T[0])
    pm, pt, pp = traj.getYawMargin(yaw, half_fov, v_min, res)
    assert abs(out["margin"] - pm) <= 1e-9 and abs(out["t"] - pt) <= 1e-9 and pp == piece
    assert (out["ok"], out["ok_loose"], out["ok_tight"], out["ok_slow"]) == (int(ok), 1, 0, 0)
