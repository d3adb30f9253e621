"""k_minco_avoid on the device (anet_minco_avoid_partial_grads_dev and what is composed from it) against the float64 restatement of
tests/avoid_np.py: values, padding and the location rule, the bit contracts, exact zeros and NaN isolation, the composed
objective end to end and under the lockstep L-BFGS."""
import ctypes

import numpy as np
import pytest
import torch

from tests import avoid_np as av

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bm(a, ld, fill=0.0):
    """(n, f) numpy -> batch-minor torch tensor (f, ld) on the device."""
    a = np.asarray(a, dtype=np.float64)
    t = torch.full((a.shape[1], ld), fill, dtype=torch.float64)
    t[:, :a.shape[0]] = torch.from_numpy(a.reshape(a.shape[0], -1)).T
    return t.to(DEV)


def _walks(rng, B, N, c):
    """Rest-to-rest random walks of about 1.5 m steps, reflected into a common 6 m box so that vehicles do meet."""
    pts = np.empty((B, N + 1, 3))
    pts[:, 0] = rng.uniform(0.0, 6.0, (B, 3))
    for i in range(N):
        p = pts[:, i] + rng.normal(size=(B, 3)) * 0.9
        p = np.abs(p)
        pts[:, i + 1] = 6.0 - np.abs(6.0 - p)
    head, tail = np.zeros((B, 3, c)), np.zeros((B, 3, c))
    head[:, :, 0], tail[:, :, 0] = pts[:, 0], pts[:, -1]
    T = np.linalg.norm(np.diff(pts, axis=1), axis=2) / 1.5 + 0.4
    return head, tail, pts[:, 1:-1].copy(), T


def _fleet(anet_ctx, rng, s, N, B):
    import allocnet_amd as aa
    head, tail, wps, T = _walks(rng, B, N, min(s, 3))
    co, _ = aa.minco_solve(head, tail, wps, T, s, ctx=anet_ctx)
    return head, tail, wps, T, co


class Case:
    """One problem on the host and on the device.  alias: the others ARE the ego buffers."""

    def __init__(self, anet_ctx, s, N, No, B, Bo, res, lists, seed, z_scale=1.0, ego_t0=True, other_t0=True, alias=False):
        rng = np.random.default_rng(seed)
        self.s, self.N, self.No, self.B, self.Bo, self.res, self.z_scale = s, N, No, B, Bo, res, z_scale
        self.head, self.tail, self.wps, self.T, self.co = _fleet(anet_ctx, rng, s, N, B)
        span = self.T.sum(1).mean()
        self.t0 = rng.uniform(0.0, 0.4 * span, B) if ego_t0 else None
        if alias:
            assert (No, Bo) == (N, B) and ego_t0 == other_t0
            self.oT, self.oco, self.ot0 = self.T, self.co, self.t0
        else:
            _, _, _, self.oT, self.oco = _fleet(anet_ctx, rng, s, No, Bo)
            self.ot0 = rng.uniform(-0.2 * span, 0.5 * span, Bo) if other_t0 else None
        self.start = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
        self.nbr = np.concatenate([np.asarray(l, dtype=np.int32) for l in lists]) if self.start[-1] else np.zeros(0, dtype=np.int32)
        self.alias = alias

    def host(self):
        return self.co, self.T, self.t0, self.oco, self.oT, self.ot0, self.start, self.nbr

    def limits(self, w=40.0):
        """min_dist^2 at the 40th percentile of the restatement's q over the (sample, neighbour) terms at which the neighbour is
        there, mu a tenth of the spread to the 60th; on the restatement alone: with 50 terms or more, active on >= 10 % and
        inactive on >= 10 % of them."""
        q = av.all_q(*self.host(), self.res, self.z_scale)
        min_dist, mu, frac = av.limits_from(q) if len(q) else (1.0, 0.0, 0.0)
        if mu <= 0.0:                                                   # (fewer than two distinct terms)
            mu = 0.1 * min_dist ** 2
        print(f"{len(q)} terms, active on {100 * frac:.1f} %; min_dist {min_dist:.3f} m, mu {mu:.3g} m^2")
        if len(q) >= 50:
            assert 0.1 <= frac <= 0.9
        self.kw = dict(res=self.res, w=w, mu=mu, min_dist=min_dist, z_scale=self.z_scale)
        return len(q)

    def penalty(self):
        import allocnet_amd as aa
        k = self.kw
        return aa.make_avoid_penalty(w=k["w"], smooth_mu=k["mu"], min_dist=k["min_dist"], z_scale=k["z_scale"], res=k["res"])

    def device(self, ld=None, ldo=None):
        import allocnet_amd as aa
        ld = ld or (aa.recommended_ld(self.B) if self.B > 1 else 1)
        ldo = ldo or (aa.recommended_ld(self.Bo) if self.Bo > 1 else 1)
        d = dict(ld=ld, co=_bm(self.co.reshape(self.B, -1), ld), T=_bm(self.T, ld, fill=1.0),
                 t0=torch.from_numpy(self.t0).to(DEV) if self.t0 is not None else None)
        if self.alias:
            d["others"] = aa.AvoidOthers(d["co"], d["T"], d["t0"], self.N, self.B)
        else:
            d["others"] = aa.AvoidOthers(_bm(self.oco.reshape(self.Bo, -1), ldo), _bm(self.oT, ldo, fill=1.0),
                                         torch.from_numpy(self.ot0).to(DEV) if self.ot0 is not None else None, self.No, self.Bo)
        d["nbr"] = (torch.from_numpy(self.start).to(DEV), torch.from_numpy(self.nbr).to(DEV))
        return d

    def launch(self, anet_ctx, d=None, pen=None, accumulate=False, into=None, fill=float("nan")):
        """-> the device tensors gdC, gdT, piece_cost, gd_t0 (whole rows, padding lanes included)."""
        import allocnet_amd as aa
        d = d or self.device()
        ld = d["ld"]
        if into is None:
            into = tuple(torch.full(shape, fill, dtype=torch.float64, device=DEV)
                         for shape in ((self.N * 3 * 2 * self.s, ld), (self.N, ld), (self.N, ld), (ld,)))
        aa.minco_avoid_partial_grads_dev(pen or self.penalty(), self.s, self.N, self.B, d["co"], d["T"], d["others"], d["nbr"],
                                         into[0], into[1], into[2], into[3], t0=d["t0"], accumulate=accumulate, ctx=anet_ctx)
        torch.cuda.synchronize()
        return into

    def numpy(self, out):
        B, N, D = self.B, self.N, 2 * self.s
        gC, gT, pc, g0 = out
        return (pc[:, :B].T.cpu().numpy(), gC[:, :B].T.cpu().numpy().reshape(B, N, 3, D), gT[:, :B].T.cpu().numpy(), g0[:B].cpu().numpy())


def _compare(what, got, ref, n_terms):
    """cost 1e-9 relative; gdC, gdT, gd_t0 1e-7 scaled by max(1, max|ref|): the bars of test_flat_partial_grads_match_autograd."""
    (pc, gC, gT, g0), (rpc, rgC, rgT, rg0) = got, ref
    cost, rcost = pc.sum(1), rpc.sum(1)
    rel = np.abs(cost - rcost) / np.maximum(np.abs(rcost), 1e-300)
    rel[rcost == 0.0] = np.abs(cost[rcost == 0.0])
    print(f"{what} cost: worst relative {rel.max():.3e} (bar 1e-9)")
    errs = {n: np.abs(g - r).max() / max(1.0, np.abs(r).max()) for n, g, r in (("gdC", gC, rgC), ("gdT", gT, rgT), ("gd_t0", g0, rg0))}
    print(f"{what} " + ", ".join(f"{n}: {e:.3e}" for n, e in errs.items()) + " (bar 1e-7); max |ref| " +
          ", ".join(f"{np.abs(r).max():.3e}" for r in (rgC, rgT, rg0)))
    if n_terms >= 50:
        assert max(np.abs(r).max() for r in (rgC, rgT, rg0)) > 0.0
    assert rel.max() <= 1e-9
    assert all(e <= 1e-7 for e in errs.values()), errs


def _lists(rng, B, Bo, k, exclude_self=False):
    out = []
    for b in range(B):
        pool = np.array([o for o in range(Bo) if not (exclude_self and o == b)])
        out.append(rng.permutation(pool)[:k])
    return out


SHAPES = {
    "one": dict(s=2, N=1, No=1, B=1, Bo=1, res=1, other_t0=False),
    "ragged": dict(s=3, N=5, No=4, B=3, Bo=7, res=5, z_scale=1.5),
    "alias": dict(s=4, N=8, No=8, B=130, Bo=130, res=20, alias=True),
    "rounds": dict(s=3, N=16, No=3, B=2, Bo=70, res=64, z_scale=1.5, other_t0=False),
    "long": dict(s=4, N=16, No=16, B=65, Bo=5, res=20, ego_t0=False),
}


def _case(anet_ctx, name):
    kw = SHAPES[name]
    rng = np.random.default_rng(17)
    if name == "one":
        lists = [[0]]
    elif name == "ragged":
        lists = [[3, 0, 6, 1, 5, 2], [], [4, 4, 1]]                    # 0..6 neighbours, one list empty, a repeat, no order
    elif name == "alias":
        lists = _lists(rng, 130, 130, 3, exclude_self=True)
    elif name == "rounds":
        lists = [rng.permutation(70), np.arange(70)]                   # more than a wave of neighbours, 1024 samples per ego
    else:
        lists = [np.arange(5) for _ in range(65)]
    return Case(anet_ctx, lists=lists, seed=1000 + len(name), **kw)


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_matches_the_restatement(anet_ctx, name):
    case = _case(anet_ctx, name)
    n_terms = case.limits()
    got = case.numpy(case.launch(anet_ctx))
    ref = av.j_avoid_grads(*case.host(), **case.kw)
    _compare(name, got, ref, n_terms)


# 2 ---------------------------------------------------------------------------------------------
def test_zero_duration_padding_is_never_located(anet_ctx):
    """Others with zero-duration pieces in the middle and at the end, their coefficients NaN: the same bits as without them."""
    import allocnet_amd as aa
    case = _case(anet_ctx, "ragged")
    case.limits()
    plain = case.launch(anet_ctx)
    keep = [0, 2, 3, 5]                                                 # pieces 1, 4, 6 of 7 are padding
    oco = np.full((case.Bo, 7, 3, 2 * case.s), np.nan)
    oT = np.zeros((case.Bo, 7))
    oco[:, keep], oT[:, keep] = case.oco, case.oT
    ref = av.j_avoid_grads(case.co, case.T, case.t0, oco, oT, case.ot0, case.start, case.nbr, **case.kw)
    assert all(np.array_equal(a, b) for a, b in zip(ref, av.j_avoid_grads(*case.host(), **case.kw)))
    d = case.device()
    ldo = d["others"].T.stride(0)
    d["others"] = aa.AvoidOthers(_bm(oco.reshape(case.Bo, -1), ldo), _bm(oT, ldo, fill=1.0), d["others"].t0, 7, case.Bo)
    padded = case.launch(anet_ctx, d=d)
    for a, b in zip(plain, padded):
        assert torch.equal(a[..., :case.B], b[..., :case.B])
    assert torch.isfinite(padded[0][:, :case.B]).all()


def test_location_rule_at_a_shared_knot(anet_ctx):
    """The discontinuous equal-knot case of the CPU test: the sample on a knot sees the piece that starts there."""
    import allocnet_amd as aa
    co, T, t0, oco, oT, ot0, start, nbr, kw = av.discontinuous_case()
    s, N = 3, 3
    pen = aa.make_avoid_penalty(w=kw["w"], smooth_mu=kw["mu"], min_dist=kw["min_dist"], z_scale=kw["z_scale"], res=kw["res"])
    out = tuple(torch.full(shape, float("nan"), dtype=torch.float64, device=DEV) for shape in ((N * 3 * 2 * s, 1), (N, 1), (N, 1), (1,)))
    others = aa.AvoidOthers(_bm(oco.reshape(1, -1), 1), _bm(oT, 1), torch.from_numpy(ot0).to(DEV), N, 1)
    aa.minco_avoid_partial_grads_dev(pen, s, N, 1, _bm(co.reshape(1, -1), 1), _bm(T, 1), others, (start, nbr), *out,
                                     t0=torch.from_numpy(t0).to(DEV), ctx=anet_ctx)
    torch.cuda.synchronize()
    rpc, rgC, rgT, rg0 = av.j_avoid_grads(co, T, t0, oco, oT, ot0, start, nbr, **kw)
    pc = out[2][:, 0].cpu().numpy()
    assert pc[1] == 0.0 and rpc[0, 1] == 0.0
    assert np.allclose(pc, rpc[0], rtol=1e-12) and pc[0] > 0.0 and pc[2] > 0.0
    assert np.allclose(out[0][:, 0].cpu().numpy().reshape(N, 3, 2 * s), rgC[0], rtol=1e-9, atol=1e-12)
    assert np.allclose(out[1][:, 0].cpu().numpy(), rgT[0], rtol=1e-9, atol=1e-12)


# 3 ---------------------------------------------------------------------------------------------
def test_accumulate_contract(anet_ctx):
    """accumulate = 1 after anet_minco_partial_grads_dev equals the sum of the separate results to the last bit, gd_t0 included;
    accumulate = 0 overwrites a NaN-poisoned buffer; lanes in [B, ld) keep a sentinel."""
    import allocnet_amd as aa
    case = _case(anet_ctx, "alias")
    case.limits()
    s, N, B = case.s, case.N, case.B
    d = case.device()
    ld = d["ld"]
    assert ld > B
    own = case.launch(anet_ctx, d=d)                                     # onto NaN
    for t in own:
        assert torch.isfinite(t[..., :B]).all() and torch.isnan(t[..., B:]).all()
    pen = aa.make_penalty(rho=0.0, w_vel=25.0, w_acc=9.0, smooth_mu=0.05, max_vel=1.5, max_acc=2.5, res=case.res)
    acc = tuple(torch.full_like(t, 123.0) for t in own)
    q = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    anet_ctx.check(anet_ctx.lib.anet_minco_partial_grads_dev(anet_ctx.handle, s, N, B, ld, q(d["co"]), q(d["T"]), None,
                                                             ctypes.cast(ctypes.pointer(pen), ctypes.c_void_p), 1, q(acc[0]),
                                                             q(acc[1]), q(acc[2]), st))
    torch.cuda.synchronize()
    sums = [e[..., :B] + f[..., :B] for e, f in zip(acc, own)]
    assert float(acc[2][:, :B].sum()) > 0.0 and float(own[2][:, :B].sum()) > 0.0 and float(own[3][:B].abs().sum()) > 0.0
    case.launch(anet_ctx, d=d, accumulate=True, into=acc)
    for got, ref in zip(acc, sums):
        assert torch.equal(got[..., :B], ref)
        assert (got[..., B:] == 123.0).all()


def test_same_bits_alone_and_at_another_stride(anet_ctx):
    """The outputs of three egos: the whole batch in one launch, each alone in a launch of its own, and two values of ld and o_ld."""
    import allocnet_amd as aa
    case = _case(anet_ctx, "alias")
    case.limits()
    B = case.B
    whole = case.launch(anet_ctx)
    wide = Case.launch(case, anet_ctx, d=_unaliased(case, ld=B + 3, ldo=B + 70))
    for a, b in zip(whole, wide):
        assert torch.equal(a[..., :B], b[..., :B])
    pen = case.penalty()
    for b in (0, 64, 129):
        d = _unaliased(case, ld=aa.recommended_ld(B), ldo=B)
        lo, hi = case.start[b], case.start[b + 1]
        one = tuple(torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
                    for shape in ((case.N * 3 * 2 * case.s, 1), (case.N, 1), (case.N, 1), (1,)))
        nbr = (np.array([0, hi - lo], dtype=np.int32), case.nbr[lo:hi])
        aa.minco_avoid_partial_grads_dev(pen, case.s, case.N, 1, d["co"][:, b:b + 1].contiguous(), d["T"][:, b:b + 1].contiguous(),
                                         d["others"], nbr, *one, t0=d["t0"][b:b + 1].contiguous(), ctx=anet_ctx)
        torch.cuda.synchronize()
        for a, w in zip(one, whole):
            assert torch.equal(a[..., 0], w[..., b]), b


def _unaliased(case, ld, ldo):
    """The aliased fleet with the others in a buffer of their own (another row stride)."""
    import allocnet_amd as aa
    d = case.device(ld=ld)
    d["others"] = aa.AvoidOthers(_bm(case.co.reshape(case.B, -1), ldo), _bm(case.T, ldo, fill=1.0), d["t0"].clone(), case.N, case.B)
    return d


# 4 ---------------------------------------------------------------------------------------------
def test_exact_zeros_and_nan_isolation(anet_ctx):
    import allocnet_amd as aa
    case = _case(anet_ctx, "long")
    case.limits()
    B = case.B
    # well separated: the others moved 100 m away, min_dist = 1e-3
    far = Case.device(case)
    shifted = case.oco.copy()
    shifted[..., -1] += 100.0
    ldo = far["others"].T.stride(0)
    far["others"] = far["others"]._replace(coeffs=_bm(shifted.reshape(case.Bo, -1), ldo))
    out = case.launch(anet_ctx, d=far, pen=aa.make_avoid_penalty(w=40.0, smooth_mu=1e-8, min_dist=1e-3, res=case.res))
    for t in out:
        assert (t[..., :B] == 0.0).all()
    # a neighbour index of Bo in the list of ego 7: NaN there, the same bits elsewhere
    good = case.launch(anet_ctx)
    d = case.device()
    nbr = case.nbr.copy()
    nbr[case.start[7] + 2] = case.Bo
    d["nbr"] = (d["nbr"][0], torch.from_numpy(nbr).to(DEV))
    bad = case.launch(anet_ctx, d=d, fill=5.0)
    rest = [b for b in range(B) if b != 7]
    for g, t in zip(good, bad):
        assert torch.isnan(t[..., 7]).all()
        assert torch.equal(g[..., rest], t[..., rest]) and torch.isfinite(t[..., rest]).all()
        assert (t[..., B:] == 5.0).all()
    # a duration of ego 3 that is not positive, a neighbour's duration that is not finite
    d = case.device()
    d["T"][2, 3] = 0.0
    out = case.launch(anet_ctx, d=d)
    assert all(torch.isnan(t[..., 3]).all() and torch.isfinite(t[..., [0, 4, B - 1]]).all() for t in out)
    d = case.device()
    d["others"].T[1, 4] = float("inf")
    out = case.launch(anet_ctx, d=d)
    assert all(torch.isnan(t[..., :B]).all() for t in out)               # every ego lists other 4


# 5 ---------------------------------------------------------------------------------------------
def test_minco_avoid_cost_grad_finite_differences(anet_ctx):
    """s = 4, N = 6, B = 8, three others: the cost is minco_cost_grad + the restatement within 1e-9 relative; gradP, gradT and
    grad_t0 against central differences of the returned cost, h = 1e-6, bar 2e-5 (test_minco_flat_cost_grad_finite_differences)."""
    import allocnet_amd as aa
    s, N, B, res = 4, 6, 8, 7
    case = Case(anet_ctx, s, N, 5, B, 3, res, lists=[np.arange(3)] * B, seed=77, z_scale=1.5)
    case.limits(w=25.0)
    apen = case.penalty()
    pen = aa.make_penalty(rho=2.0, w_vel=25.0, w_acc=9.0, smooth_mu=0.05, max_vel=1.5, max_acc=2.5, res=9)
    others = aa.upload_others(case.oco, case.oT, case.ot0, ctx=anet_ctx)
    nbr = (case.start, case.nbr)
    f = lambda w, t, z: aa.minco_avoid_cost_grad(case.head, case.tail, w, t, s, others, apen, nbr, t0=z, penalty=pen, ctx=anet_ctx)
    wps, T, t0 = case.wps, case.T, case.t0
    cost, gP, gT, g0 = f(wps, T, t0)
    base = aa.minco_cost_grad(case.head, case.tail, wps, T, s, penalty=pen, ctx=anet_ctx)[0]
    ja = av.j_avoid(*case.host(), **case.kw)
    assert (ja > 0.0).any()
    rel = np.abs(cost - (base + ja)) / np.abs(base + ja)
    print(f"cost against minco_cost_grad + J_avoid: worst relative {rel.max():.3e} (bar 1e-9)")
    assert rel.max() <= 1e-9
    h = 1e-6

    def check(what, fd, g):
        err = np.abs(fd - g).max() / max(1.0, np.abs(g).max())
        print(f"{what}: {err:.3e} (bar 2e-5)")
        assert err <= 2e-5
    for (k, ax) in [(0, 0), (2, 1), (4, 2)]:
        wp, wm = wps.copy(), wps.copy()
        wp[:, k, ax] += h
        wm[:, k, ax] -= h
        check(f"gradP[{k},{ax}]", (f(wp, T, t0)[0] - f(wm, T, t0)[0]) / (2 * h), gP[:, k, ax])
    for i in (0, 3, 5):
        tp, tm = T.copy(), T.copy()
        tp[:, i] += h
        tm[:, i] -= h
        check(f"gradT[{i}]", (f(wps, tp, t0)[0] - f(wps, tm, t0)[0]) / (2 * h), gT[:, i])
    check("grad_t0", (f(wps, T, t0 + h)[0] - f(wps, T, t0 - h)[0]) / (2 * h), g0)


# 6 ---------------------------------------------------------------------------------------------
def test_lockstep_lbfgs_separates_a_head_on_pair(anet_ctx):
    """Two vehicles fly head-on through the same point at the same time, each the other's only neighbour: a few rounds of
    lbfgs_optimize_dev on the composed objective, the other frozen per round.  Every status is >= 0, the composed cost and its
    J_avoid share end below the start.  The separation is printed, not asserted (the energy may trade against the penalty)."""
    import allocnet_amd as aa
    s, c, N, B, res = 3, 3, 4, 2, 20
    frac = np.linspace(0.0, 1.0, N + 1)[None, :, None]
    ends = np.array([[[-4.0, 0.03, 1.0], [4.0, 0.03, 1.0]], [[4.0, -0.03, 1.0], [-4.0, -0.03, 1.0]]])
    pts = ends[:, :1] * (1.0 - frac) + ends[:, 1:] * frac
    head, tail = np.zeros((B, 3, c)), np.zeros((B, 3, c))
    head[:, :, 0], tail[:, :, 0] = pts[:, 0], pts[:, -1]
    wps, T = pts[:, 1:-1], np.full((B, N), 1.0)
    apen = aa.make_avoid_penalty(w=200.0, smooth_mu=0.05, min_dist=0.8, z_scale=1.0, res=res)
    pen = aa.make_penalty(rho=5.0, res=res)
    nbr = aa.neighbours_all(B, B, exclude_self=True)
    kw = dict(res=res, w=200.0, mu=0.05, min_dist=0.8, z_scale=1.0)

    def state(w, t):
        """composed cost and J_avoid of the fleet against itself, its coefficients and exact separation"""
        co, _ = aa.minco_solve(head, tail, w, t, s, ctx=anet_ctx)
        ja = av.j_avoid(co, t, None, co, t, None, nbr[0], nbr[1], **kw)
        base = aa.minco_cost_grad(head, tail, w, t, s, penalty=pen, ctx=anet_ctx)[0]
        sep = aa.traj_separation(co, t, ctx=anet_ctx)[0]
        return (base + ja).sum(), ja.sum(), co, float(sep.min())
    j0, a0, co, sep0 = state(wps, T)
    assert a0 > 0.0
    ld = aa.recommended_ld(B)
    nw = 3 * (N - 1)
    x = torch.zeros(nw + N, ld, dtype=torch.float64, device=DEV)
    x[:nw, :B] = torch.from_numpy(wps.reshape(B, -1)).T.to(DEV)
    x[nw:, :B] = torch.from_numpy(np.log(T)).T.to(DEV)
    d_head, d_tail = _bm(head.reshape(B, -1), ld), _bm(tail.reshape(B, -1), ld)
    w, t = wps, T
    for rnd in range(3):
        others = aa.upload_others(co, t, ctx=anet_ctx)                    # the fleet at the previous iterate, frozen
        ev = aa.avoid_objective_dev(d_head, d_tail, s, c, N, B, others, apen, nbr, penalty=pen, ctx=anet_ctx)
        res_ = aa.lbfgs_optimize_dev(x, ev, batch=B, param=aa.lbfgs_parameter_t(past=3, delta=1e-4), max_evals=600, ctx=anet_ctx)
        torch.cuda.synchronize()
        status = res_["status"].cpu().numpy()
        print(f"round {rnd}: status {status.tolist()}, evals {res_['evals'].cpu().numpy().tolist()}")
        assert (status >= 0).all()
        w = x[:nw, :B].T.cpu().numpy().reshape(B, N - 1, 3)
        t = np.exp(x[nw:, :B].T.cpu().numpy())
        j1, a1, co, sep1 = state(w, t)
    print(f"J {j0:.6g} -> {j1:.6g}, J_avoid {a0:.6g} -> {a1:.6g}, exact separation {sep0:.4f} m -> {sep1:.4f} m")
    assert j1 < j0 and a1 < a0
