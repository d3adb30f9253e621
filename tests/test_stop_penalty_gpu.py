"""Stop within known space on the device (anet_minco_stop_partial_grads_dev, anet_traj_stop_margin[_dev], traj_stop_check and the
facades) against the restatement of tests/stop_np.py: the penalty's values and contracts, its degenerate form against the obstacle
term, the sampled margin, the composed objective end to end and under the lockstep L-BFGS, the directional check against a closed
form, and the C++ members.  The maps, pieces and shapes are those of tests/test_voxel_distance_gpu.py."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import dist_np as dn
from tests import stop_np as sn
from tests.avoid_np import horner
from tests.test_voxel_distance_gpu import DEV, SHAPES, Field, _bm, _pieces, _transform, _walks

pytestmark = pytest.mark.gpu
A_BRAKE = 2.0                                                            # m/s^2: the pieces move at about 0.3 m/s
REACT = {"brake": dict(t_react=0.0, speed_eps=0.0), "react": dict(t_react=0.15, speed_eps=1e-2)}


def _effective(co, T, res, f, a_brake, t_react, speed_eps):
    """d - t_react s_eps - v.v / (2 a_brake) of every sample j < res of the batch, by the restatement alone: what the percentile rule
    of dist_np.limits_from is applied to."""
    d, _ = dn.all_d(co, T, res, **f.kw)
    vv = np.concatenate([(dn.sample_points(co[b], T[b], res)[3] ** 2).sum(-1).reshape(-1) for b in range(len(T))])
    return d - sn.stop_distance(vv, a_brake, t_react, np.sqrt(vv + speed_eps ** 2))


class Case:
    _cache = {}

    def __init__(self, anet_ctx, s, N, B, res, seed, react="brake", w=40.0, a_brake=A_BRAKE):
        self.f = Field.get(anet_ctx)
        self.s, self.N, self.B, self.res = s, N, B, res
        self.co, self.T = _pieces(np.random.default_rng(seed), self.f, B, N, s, res)
        off = dn.all_d(self.co, self.T, res, **self.f.kw)[1]
        eff = _effective(self.co, self.T, res, self.f, a_brake, **REACT[react])
        clearance, mu, frac = dn.limits_from(eff)
        if len(eff) < 2:
            # one sample has no percentiles: a fixed mu and the sample in the middle of the blend, g = mu / 2, as the distance test has it
            mu = 0.05
            clearance, frac = float(eff[0]) + 0.5 * mu, 1.0
        print(f"{len(eff)} samples, active on {100 * frac:.1f} %, nearest lattice plane {off:.3e} voxel; clearance {clearance:.4f} m, "
              f"mu {mu:.4f} m")
        assert off >= 1e-4
        if len(eff) >= 2:
            assert 0.1 <= frac <= 0.9
        self.kw = dict(res=res, w=w, mu=mu, clearance=clearance, a_brake=a_brake, **REACT[react], **self.f.kw)

    @classmethod
    def get(cls, anet_ctx, name, react="brake"):
        """the case of a shape, and its reference, computed once and shared (never written to)"""
        key = (name, react)
        if key not in cls._cache:
            case = cls(anet_ctx, seed=1000 + len(name), react=react, **SHAPES[name])
            case.ref = sn.j_stop_grads(case.co, case.T, parts=True, **case.kw)
            cls._cache[key] = case
        return cls._cache[key]

    def penalty(self, **over):
        import allocnet_amd as aa
        k = dict(self.kw, **over)
        return aa.make_stop_penalty(w=k["w"], smooth_mu=k["mu"], clearance=k["clearance"], a_brake=k["a_brake"], t_react=k["t_react"],
                                    speed_eps=k["speed_eps"], res=self.res)

    def device(self, ld=None):
        import allocnet_amd as aa
        ld = ld or (aa.recommended_ld(self.B) if self.B > 1 else 1)
        return dict(ld=ld, co=_bm(self.co.reshape(self.B, -1), ld), T=_bm(self.T, ld, fill=1.0))

    def launch(self, anet_ctx, d=None, pen=None, accumulate=False, into=None, fill=float("nan"), field=None):
        """-> the device tensors gdC, gdT, piece_cost (whole rows, padding lanes included)."""
        import allocnet_amd as aa
        d = d or self.device()
        ld = d["ld"]
        if into is None:
            into = tuple(torch.full(shape, fill, dtype=torch.float64, device=DEV)
                         for shape in ((self.N * 3 * 2 * self.s, ld), (self.N, ld), (self.N, ld)))
        aa.minco_stop_partial_grads_dev(pen or self.penalty(), self.s, self.N, self.B, d["co"], d["T"],
                                        field or (self.f.grid, self.f.d_sd2), into[0], into[1], into[2], accumulate=accumulate,
                                        ctx=anet_ctx)
        torch.cuda.synchronize()
        return into

    def numpy(self, out):
        B, N, D = self.B, self.N, 2 * self.s
        gC, gT, pc = out
        return pc[:, :B].T.cpu().numpy(), gC[:, :B].T.cpu().numpy().reshape(B, N, 3, D), gT[:, :B].T.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# the penalty against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("react", list(REACT))
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_matches_the_restatement(anet_ctx, name, react):
    """cost 1e-9 relative; gdC and gdT 1e-7 scaled by max(1, max|ref|): the obstacle term's bars.  On the restatement alone: the
    reference cost is > 0, the gradients and the G share of gdC (the velocity row of the chain rule) are not zero.  `one` has a single
    sample and so no percentiles: its clearance puts g at mu / 2 with mu = 0.05."""
    case = Case.get(anet_ctx, name, react)
    d = case.device()
    assert d["ld"] > case.B or name != "wide"
    pc, gC, gT = case.numpy(case.launch(anet_ctx, d=d))
    rpc, rgC, rgT, rgC_G, _ = case.ref
    cost, rcost = pc.sum(1), rpc.sum(1)
    rel = np.abs(cost - rcost) / np.maximum(np.abs(rcost), 1e-300)
    rel[rcost == 0.0] = np.abs(cost[rcost == 0.0])
    errs = {n: np.abs(g - r).max() / max(1.0, np.abs(r).max()) for n, g, r in (("gdC", gC, rgC), ("gdT", gT, rgT))}
    print(f"{name}/{react} cost: worst relative {rel.max():.3e} (bar 1e-9); " + ", ".join(f"{n}: {e:.3e}" for n, e in errs.items()) +
          f" (bar 1e-7); max |ref| {np.abs(rgC).max():.3e}, {np.abs(rgT).max():.3e}, G share {np.abs(rgC_G).max():.3e}")
    assert np.abs(rgC).max() > 0.0 and np.abs(rgT).max() > 0.0 and (rcost > 0.0).any() and rcost.sum() > 0.0
    assert np.abs(rgC_G).max() > 0.0
    assert np.abs(gC).max() > 0.0 and np.abs(gT).max() > 0.0
    assert rel.max() <= 1e-9
    assert all(e <= 1e-7 for e in errs.values()), errs


@pytest.mark.parametrize("name", ["quad", "ragged", "wide"])
def test_degenerate_form_is_the_obstacle_term(anet_ctx, name):
    """a_brake = inf, t_react = 0: the outputs agree with minco_obstacle_partial_grads_dev on the same inputs within 1e-12 scaled by
    max(1, max|value|), and are not zero."""
    import allocnet_amd as aa
    case = Case.get(anet_ctx, name)
    d = case.device()
    own = case.launch(anet_ctx, d=d, pen=case.penalty(a_brake=float("inf"), t_react=0.0, speed_eps=0.0))
    obs = tuple(torch.full_like(t, float("nan")) for t in own)
    open_ = aa.make_obstacle_penalty(w=case.kw["w"], smooth_mu=case.kw["mu"], clearance=case.kw["clearance"], res=case.res)
    aa.minco_obstacle_partial_grads_dev(open_, case.s, case.N, case.B, d["co"], d["T"], (case.f.grid, case.f.d_sd2), *obs, ctx=anet_ctx)
    torch.cuda.synchronize()
    for what, a, b in zip(("gdC", "gdT", "piece_cost"), own, obs):
        a, b = a[:, :case.B].cpu().numpy(), b[:, :case.B].cpu().numpy()
        err = np.abs(a - b).max() / max(1.0, np.abs(b).max())
        print(f"{name} {what}: {err:.3e} (bar 1e-12), max |value| {np.abs(b).max():.3e}")
        assert np.abs(b).max() > 0.0 and err <= 1e-12


# ---------------------------------------------------------------------------------------------
# the penalty's contracts
# ---------------------------------------------------------------------------------------------
def test_accumulate_contract(anet_ctx):
    """accumulate = 1 after anet_minco_partial_grads_dev equals the sum of the separate results to the last bit; accumulate = 0
    overwrites a NaN-poisoned buffer; lanes in [B, ld) keep a sentinel; piece_cost may be NULL."""
    import allocnet_amd as aa
    case = Case.get(anet_ctx, "wide", "react")
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
    assert float(acc[2][:, :B].sum()) > 0.0 and float(own[2][:, :B].sum()) > 0.0
    case.launch(anet_ctx, d=d, accumulate=True, into=acc)
    for got, ref in zip(acc, sums):
        assert torch.equal(got[..., :B], ref)
        assert (got[..., B:] == 123.0).all()
    two = tuple(torch.full_like(t, float("nan")) for t in own[:2])
    aa.minco_stop_partial_grads_dev(case.penalty(), s, N, B, d["co"], d["T"], (case.f.grid, case.f.d_sd2), two[0], two[1], None,
                                    ctx=anet_ctx)
    torch.cuda.synchronize()
    assert torch.equal(two[0][:, :B], own[0][:, :B]) and torch.equal(two[1][:, :B], own[1][:, :B])


def test_same_bits_alone_and_at_another_stride(anet_ctx):
    """The outputs of three trajectories: the whole batch in one launch, at another ld, and each alone in a launch of its own."""
    import allocnet_amd as aa
    case = Case.get(anet_ctx, "wide", "react")
    B = case.B
    whole = case.launch(anet_ctx)
    wide = case.launch(anet_ctx, d=case.device(ld=B + 3))
    for a, b in zip(whole, wide):
        assert torch.equal(a[..., :B], b[..., :B])
    d = case.device()
    for b in (0, 64, 129):
        one = tuple(torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
                    for shape in ((case.N * 3 * 2 * case.s, 1), (case.N, 1), (case.N, 1)))
        aa.minco_stop_partial_grads_dev(case.penalty(), case.s, case.N, 1, d["co"][:, b:b + 1].contiguous(),
                                        d["T"][:, b:b + 1].contiguous(), (case.f.grid, case.f.d_sd2), *one, ctx=anet_ctx)
        torch.cuda.synchronize()
        for a, w in zip(one, whole):
            assert torch.equal(a[..., 0], w[..., b]), b


def test_exact_zeros_and_nan_isolation(anet_ctx):
    case = Case.get(anet_ctx, "ragged", "react")
    B = case.B
    # inactive everywhere: a clearance far below -(the map's diameter), and the +NONE map: d = +inf
    out = case.launch(anet_ctx, pen=case.penalty(clearance=-1e3))
    for t in out:
        assert (t[..., :B] == 0.0).all() and torch.isnan(t[..., B:]).all()
    far = Field.get(anet_ctx, size=(40, 4, 4), origin=(-300.0, -20.0, -20.0), scale=10.0, density=0.0, walls=0)
    assert (far.d_sd2 == dn.NONE).all()
    out = case.launch(anet_ctx, field=(far.grid, far.d_sd2))
    for t in out:
        assert (t[..., :B] == 0.0).all() and torch.isnan(t[..., B:]).all()
    # a duration of trajectory 1 that is not positive: NaN there, the same bits elsewhere; lanes in [B, ld) keep their sentinel
    good = case.launch(anet_ctx)
    assert all(float(t[..., :B].abs().sum()) > 0.0 for t in good)
    d = case.device()
    d["T"][2, 1] = 0.0
    bad = case.launch(anet_ctx, d=d, fill=5.0)
    for g, t in zip(good, bad):
        assert torch.isnan(t[..., 1]).all() and torch.isfinite(t[..., [0, 2]]).all()
        assert torch.equal(g[..., [0, 2]], t[..., [0, 2]]) and (t[..., B:] == 5.0).all()
    # a non-finite constant coefficient of trajectory 2, then a non-finite linear one (the velocity) of trajectory 0
    for row, b in ((5, 2), (4, 0)):
        d = case.device()
        d["co"][row, b] = float("inf")
        out = case.launch(anet_ctx, d=d)
        others = [x for x in range(B) if x != b]
        for g, t in zip(good, out):
            assert torch.isnan(t[..., b]).all() and torch.equal(g[..., others], t[..., others])
    # the all-blocked map: d = -inf, NaN everywhere
    full = _transform(anet_ctx, np.ones(case.f.size, np.uint8), 1, origin=case.f.origin, scale=case.f.scale)
    out = case.launch(anet_ctx, field=(case.f.grid, full))
    assert all(torch.isnan(t[..., :B]).all() for t in out)


def test_error_codes(anet_ctx):
    """ANET_ERR_UNSUPPORTED for an order other than 2, 3, 4; ANET_ERR_INVALID for a NULL pointer other than the optional outputs,
    ld < batch, a piece count outside [1, ANET_MAX_PIECES], a bad grid, a penalty outside its ranges; batch == 0 touches nothing."""
    import allocnet_amd as aa
    from allocnet_amd._lib import ANET_ERR_INVALID, ANET_ERR_UNSUPPORTED, ANET_OK
    case = Case.get(anet_ctx, "ragged", "react")
    s, N, B = case.s, case.N, case.B
    d = case.device()
    ld = d["ld"]
    lib, h = anet_ctx.lib, anet_ctx.handle
    q = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    ref = lambda p: ctypes.cast(ctypes.pointer(p), ctypes.c_void_p)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    grid, sd2 = case.f.grid, case.f.d_sd2
    gC = torch.full((N * 3 * 2 * s, ld), 7.0, dtype=torch.float64, device=DEV)
    gT, pc, m = (torch.full((N, ld), 7.0, dtype=torch.float64, device=DEV) for _ in range(3))
    host_co, host_T, host_m = np.ascontiguousarray(case.co), np.ascontiguousarray(case.T), np.empty((B, N))
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def grads(pen=None, s_=s, N_=N, B_=B, ld_=ld, co=d["co"], T=d["T"], g=grid, f=sd2, out=gC, outT=gT):
        return lib.anet_minco_stop_partial_grads_dev(h, ref(pen or case.penalty()), s_, N_, B_, ld_, q(co), q(T), ctypes.byref(g), q(f),
                                                     0, q(out), q(outT), q(pc), st)

    def margin_dev(pen=None, s_=s, N_=N, B_=B, ld_=ld, co=d["co"], T=d["T"], g=grid, f=sd2, out=m):
        return lib.anet_traj_stop_margin_dev(h, ref(pen or case.penalty()), s_, N_, B_, ld_, q(co), q(T), ctypes.byref(g), q(f), q(out),
                                             None, None, None, st)

    def margin_host(pen=None, s_=s, N_=N, B_=B, co=host_co, T=host_T, g=grid, f=sd2, out=host_m):
        return lib.anet_traj_stop_margin(h, ref(pen or case.penalty()), s_, N_, B_, hp(co) if co is not None else None,
                                         hp(T) if T is not None else None, ctypes.byref(g), q(f),
                                         hp(out) if out is not None else None, None, None, None)
    bad_grid = type(grid)()
    ctypes.memmove(ctypes.byref(bad_grid), ctypes.byref(grid), ctypes.sizeof(grid))
    bad_grid.scale = 0.0
    for fn in (grads, margin_dev, margin_host):
        assert fn() == ANET_OK
        for order in (1, 5):
            assert fn(s_=order) == ANET_ERR_UNSUPPORTED
        for pieces in (0, 17):
            assert fn(N_=pieces) == ANET_ERR_INVALID
        assert fn(g=bad_grid) == ANET_ERR_INVALID
        assert fn(co=None) == ANET_ERR_INVALID and fn(T=None) == ANET_ERR_INVALID and fn(f=None) == ANET_ERR_INVALID
        assert fn(out=None) == ANET_ERR_INVALID
        for over in (dict(clearance=float("inf")), dict(a_brake=0.0), dict(a_brake=float("nan")), dict(t_react=-0.1),
                     dict(t_react=float("inf")), dict(speed_eps=-1.0), dict(res=0)):
            pen = case.penalty()
            for k, v in over.items():
                setattr(pen, k, v)
            assert fn(pen=pen) == ANET_ERR_INVALID, over
        assert fn(pen=case.penalty(a_brake=float("inf"))) == ANET_OK
    assert grads(outT=None) == ANET_ERR_INVALID
    for fn in (grads, margin_dev):
        assert fn(ld_=B - 1) == ANET_ERR_INVALID
    # what only the penalty reads: w, smooth_mu, speed_eps > 0 with t_react > 0
    for over in (dict(w=-1.0), dict(w=float("inf")), dict(smooth_mu=0.0), dict(speed_eps=0.0)):
        pen = case.penalty()
        for k, v in over.items():
            setattr(pen, k, v)
        assert grads(pen=pen) == ANET_ERR_INVALID, over
        assert margin_dev(pen=pen) == ANET_OK and margin_host(pen=pen) == ANET_OK, over
    assert lib.anet_minco_stop_partial_grads_dev(h, None, s, N, B, ld, q(d["co"]), q(d["T"]), ctypes.byref(grid), q(sd2), 0, q(gC), q(gT),
                                                 q(pc), st) == ANET_ERR_INVALID
    torch.cuda.synchronize()
    # batch == 0: ANET_OK, nothing touched, NULL pointers allowed
    gC.fill_(7.0); gT.fill_(7.0); pc.fill_(7.0); m.fill_(7.0)
    assert grads(B_=0) == ANET_OK and margin_dev(B_=0) == ANET_OK and margin_host(B_=0) == ANET_OK
    assert grads(B_=0, co=None, out=None) == ANET_OK
    torch.cuda.synchronize()
    assert all((t == 7.0).all() for t in (gC, gT, pc, m))
    with pytest.raises(aa.AnetError):
        aa.minco_stop_partial_grads_dev(case.penalty(), 5, N, B, d["co"], d["T"], (grid, sd2), gC, gT, pc, ctx=anet_ctx)


# ---------------------------------------------------------------------------------------------
# the sampled margin
# ---------------------------------------------------------------------------------------------
def _margin_args(case):
    k = case.kw
    return dict(res=case.res, clearance=k["clearance"], a_brake=k["a_brake"], t_react=k["t_react"], **case.f.kw)


def _margin_bar(case):
    """1e-12 max(1, max|D|, the largest stop distance of a sample)"""
    k = case.kw
    _, speed, vv, _ = sn.sample_states(case.co, case.T, case.res, **case.f.kw)
    D = dn.centre_values(case.f.sd2, case.f.scale)
    return 1e-12 * max(1.0, np.abs(D[np.isfinite(D)]).max(), (k["t_react"] * speed + vv / (2.0 * k["a_brake"])).max())


@pytest.mark.parametrize("name", ["ragged", "wide"])
def test_margin_matches_the_restatement(anet_ctx, name):
    """margin against stop_np.stop_margin within 1e-12 max(1, max|D|, max stop distance); the diagnostics by consistency: the value
    recomputed at the returned t reproduces margin, and so do the returned speed and dist; the host form equals the device form
    to the bit."""
    import allocnet_amd as aa
    case = Case.get(anet_ctx, name, "react")
    B, N, k = case.B, case.N, case.kw
    d = case.device()
    out = aa.traj_stop_margin_dev(case.penalty(), case.s, N, B, d["co"], d["T"], (case.f.grid, case.f.d_sd2), ctx=anet_ctx)
    torch.cuda.synchronize()
    m, t, speed, dist = [o[:, :B].T.cpu().numpy() for o in out]
    ref = sn.stop_margin(case.co, case.T, **_margin_args(case))
    bar = _margin_bar(case)
    err = np.abs(m - ref[0]).max()
    print(f"{name}: margin error {err:.3e} (bar {bar:.3e}); margins in [{ref[0].min():.4f}, {ref[0].max():.4f}]")
    assert err <= bar and (ref[0] < 0.0).any() and (ref[0] > 0.0).any()
    assert ((t >= 0.0) & (t <= case.T)).all()
    p, v = horner(case.co, t[:, :, None])
    vv = (v ** 2).sum(-1)
    dq = dn.query(case.f.sd2, case.f.size, case.f.origin, case.f.scale, p.reshape(-1, 3))[0].reshape(B, N)
    again = ((dq - k["clearance"]) - k["t_react"] * np.sqrt(vv)) - vv / (2.0 * k["a_brake"])
    assert np.abs(again - m).max() <= bar and np.abs(dq - dist).max() <= bar and np.abs(np.sqrt(vv) - speed).max() <= bar
    assert np.abs(((dist - k["clearance"]) - k["t_react"] * speed) - speed ** 2 / (2.0 * k["a_brake"]) - m).max() <= bar
    host = aa.traj_stop_margin(case.co, case.T, (case.f.grid, case.f.d_sd2), k["a_brake"], k["t_react"], k["clearance"], case.res,
                               ctx=anet_ctx)
    for a, b in zip(host, (m, t, speed, dist)):
        assert np.array_equal(a, b)
    # only margin asked for; a bad piece poisons itself alone
    d["T"][1, 0] = float("nan")
    only = torch.full((N, d["ld"]), 3.0, dtype=torch.float64, device=DEV)
    anet_ctx.check(anet_ctx.lib.anet_traj_stop_margin_dev(
        anet_ctx.handle, ctypes.cast(ctypes.pointer(case.penalty()), ctypes.c_void_p), case.s, N, B, d["ld"],
        ctypes.c_void_p(d["co"].data_ptr()), ctypes.c_void_p(d["T"].data_ptr()), ctypes.byref(case.f.grid),
        ctypes.c_void_p(case.f.d_sd2.data_ptr()), ctypes.c_void_p(only.data_ptr()), None, None, None,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    got = only[:, :B].T.cpu().numpy()
    keep = np.ones((B, N), bool)
    keep[0, 1] = False
    assert np.isnan(got[0, 1]) and np.array_equal(got[keep], m[keep]) and (only[:, B:] == 3.0).all()


def test_inactive_pieces_have_a_margin(anet_ctx):
    """s_eps >= |v|: on a piece whose samples j < res are all inactive in the penalty, the margin over those samples is >= 0.  The
    pieces are chosen on the restatement alone (every g <= 0), which also has active pieces; the device agrees about them (a
    piece_cost of exactly 0).  The margin kernel also looks at the piece's end, j = res, which is no sample of the penalty: the
    device's margin is asserted >= 0 where its minimiser lies before the end, and the restatement's over j < res everywhere.  At
    this case 215 of the 1040 pieces are inactive: 105 with the minimiser before the end (the device assertion) and 110 with it at
    the end; both counts are printed, and each group must hold at least a quarter of the inactive pieces."""
    import allocnet_amd as aa
    case = Case.get(anet_ctx, "wide", "react")
    B, N = case.B, case.N
    g = case.ref[4]
    inactive = (g <= 0.0).all(2)
    print(f"{inactive.sum()} of {inactive.size} pieces inactive")
    assert inactive.sum() >= 5 and (~inactive).sum() >= 5
    d = case.device()
    pc = case.launch(anet_ctx, d=d)[2][:, :B].T.cpu().numpy()
    assert np.array_equal(pc == 0.0, inactive)
    out = aa.traj_stop_margin_dev(case.penalty(), case.s, N, B, d["co"], d["T"], (case.f.grid, case.f.d_sd2), ctx=anet_ctx)
    torch.cuda.synchronize()
    m, t = out[0][:, :B].T.cpu().numpy(), out[1][:, :B].T.cpu().numpy()
    inner = inactive & (t < case.T)
    print(f"minimiser before the end on {inner.sum()} inactive pieces, at the end on {(inactive & ~inner).sum()}")
    assert 4 * inner.sum() >= inactive.sum() and 4 * (inactive & ~inner).sum() >= inactive.sum()
    assert (m[inner] >= 0.0).all()
    per = sn.stop_margin(case.co, case.T, per_sample=True, **_margin_args(case))
    assert (per[..., :-1][inactive] >= 0.0).all()
    assert (m[~inactive] < m[inactive].max()).any()


# ---------------------------------------------------------------------------------------------
# composed
# ---------------------------------------------------------------------------------------------
def test_minco_stop_cost_grad_finite_differences(anet_ctx):
    """s = 4, N = 6, B = 8: the cost is minco_cost_grad + the restatement within 1e-9 relative; gradP and gradT against central
    differences of the returned cost, h = 1e-6, bar 2e-5.  The seed is the first from 77 for which, on the restatement alone, the term
    is active on 10-90 % of the samples and no sample lies within 1e-4 voxel of a lattice plane."""
    import allocnet_amd as aa
    s, N, B, res = 4, 6, 8, 7
    a_brake, t_react, speed_eps = 2.0, 0.15, 1e-2
    f = Field.get(anet_ctx)
    for seed in range(77, 177):
        head, tail, wps, T = _walks(np.random.default_rng(seed), f, B, N, 3)
        co, _ = aa.minco_solve(head, tail, wps, T, s, ctx=anet_ctx)
        off = dn.all_d(co, T, res, **f.kw)[1]
        clearance, mu, frac = dn.limits_from(_effective(co, T, res, f, a_brake, t_react, speed_eps))
        if off >= 1e-4 and 0.1 <= frac <= 0.9 and mu > 0.0:
            break
    else:
        raise AssertionError("no seed meets the two conditions")
    print(f"seed {seed}: active on {100 * frac:.1f} %, nearest lattice plane {off:.3e} voxel; clearance {clearance:.4f} m, mu {mu:.4f} m")
    kw = dict(res=res, w=25.0, mu=mu, clearance=clearance, a_brake=a_brake, t_react=t_react, speed_eps=speed_eps, **f.kw)
    stop = aa.make_stop_penalty(w=25.0, smooth_mu=mu, clearance=clearance, a_brake=a_brake, t_react=t_react, speed_eps=speed_eps, res=res)
    pen = aa.make_penalty(rho=2.0, w_vel=25.0, w_acc=9.0, smooth_mu=0.05, max_vel=1.5, max_acc=2.5, res=9)
    field = (f.grid, f.d_sd2)
    fn = lambda w, t: aa.minco_stop_cost_grad(head, tail, w, t, s, field, stop, penalty=pen, ctx=anet_ctx)
    cost, gP, gT = fn(wps, T)
    base = aa.minco_cost_grad(head, tail, wps, T, s, penalty=pen, ctx=anet_ctx)[0]
    js = sn.j_stop(co, T, **kw)
    assert (js > 0.0).any()
    rel = np.abs(cost - (base + js)) / np.abs(base + js)
    print(f"cost against minco_cost_grad + J_stop: worst relative {rel.max():.3e} (bar 1e-9)")
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
        check(f"gradP[{k},{ax}]", (fn(wp, T)[0] - fn(wm, T)[0]) / (2 * h), gP[:, k, ax])
    for i in (0, 3, 5):
        tp, tm = T.copy(), T.copy()
        tp[:, i] += h
        tm[:, i] -= h
        check(f"gradT[{i}]", (fn(wps, tp)[0] - fn(wps, tm)[0]) / (2 * h), gT[:, i])


def test_lockstep_lbfgs_slows_down_in_a_thin_known_region(anet_ctx):
    """An empty 48 x 24 x 12 map at scale 0.25 with walls; a rest-to-rest 4-piece jerk trajectory from (1.5, 3.0, 1.5) to
    (10.5, 3.0, 1.5) with T = 0.6 each (about 7 m/s at its peak, 1.6 m from floor and ceiling); a_brake = 5, t_react = 0.1,
    clearance = 0.3, w = 200, mu = 0.05, rho = 5.  lbfgs_optimize_dev on stop_objective_dev: every status >= 0; J_stop > 0 and the
    worst margin < 0 before; the composed cost and J_stop end below their start, the worst sampled margin rises, the peak sampled
    speed falls and the total duration grows.  The final margin is printed, not asserted: a penalty method leaves a residual that
    depends on w."""
    import allocnet_amd as aa
    s, c, N, B, res = 3, 3, 4, 1, 20
    size, origin, scale = (48, 24, 12), (0.0, 0.0, 0.0), 0.25
    a_brake, t_react, clearance, w, mu = 5.0, 0.1, 0.3, 200.0, 0.05
    vm = aa.VoxelMap(size, origin, scale, ctx=anet_ctx)
    frac = np.linspace(0.0, 1.0, N + 1)[None, :, None]
    ends = np.array([[[1.5, 3.0, 1.5], [10.5, 3.0, 1.5]]])
    pts = ends[:, :1] * (1.0 - frac) + ends[:, 1:] * frac
    head, tail = np.zeros((B, 3, c)), np.zeros((B, 3, c))
    head[:, :, 0], tail[:, :, 0] = pts[:, 0], pts[:, -1]
    wps, T = pts[:, 1:-1], np.full((B, N), 0.6)
    stop = aa.make_stop_penalty(w=w, smooth_mu=mu, clearance=clearance, a_brake=a_brake, t_react=t_react, speed_eps=1e-2, res=res)
    pen = aa.make_penalty(rho=5.0, res=res)
    f = dict(sd2=dn.unflat(vm.distance_field().cpu().numpy(), size), size=size, origin=origin, scale=scale)
    kw = dict(res=res, w=w, mu=mu, clearance=clearance, a_brake=a_brake, t_react=t_react, speed_eps=1e-2, **f)

    def state(wp, t):
        co, _ = aa.minco_solve(head, tail, wp, t, s, ctx=anet_ctx)
        js = sn.j_stop(co, t, **kw)
        base = aa.minco_cost_grad(head, tail, wp, t, s, penalty=pen, ctx=anet_ctx)[0]
        margin = aa.traj_stop_margin(co, t, vm, a_brake, t_react, clearance, res, ctx=anet_ctx)[0].min()
        speed = sn.sample_states(co, t, res, **f)[1].max()
        return dict(J=float((base + js).sum()), J_stop=float(js.sum()), margin=float(margin), speed=float(speed), total=float(t.sum()))
    before = state(wps, T)
    assert before["J_stop"] > 0.0 and before["margin"] < 0.0
    ld, nw = 1, 3 * (N - 1)
    x = torch.zeros(nw + N, ld, dtype=torch.float64, device=DEV)
    x[:nw, :B] = torch.from_numpy(wps.reshape(B, -1)).T.to(DEV)
    x[nw:, :B] = torch.from_numpy(np.log(T)).T.to(DEV)
    ev = aa.stop_objective_dev(_bm(head.reshape(B, -1), ld), _bm(tail.reshape(B, -1), ld), s, c, N, B, vm, stop, penalty=pen, ctx=anet_ctx)
    res_ = aa.lbfgs_optimize_dev(x, ev, batch=B, param=aa.lbfgs_parameter_t(past=3, delta=1e-4), max_evals=600, ctx=anet_ctx)
    torch.cuda.synchronize()
    status = res_["status"].cpu().numpy()
    print(f"status {status.tolist()}, evals {res_['evals'].cpu().numpy().tolist()}")
    assert (status >= 0).all()
    after = state(x[:nw, :B].T.cpu().numpy().reshape(B, N - 1, 3), np.exp(x[nw:, :B].T.cpu().numpy()))
    print("before", before)
    print("after ", after)
    assert after["J"] < before["J"] and after["J_stop"] < before["J_stop"]
    assert after["margin"] > before["margin"] and after["speed"] < before["speed"] and after["total"] > before["total"]
    # the facade of one trajectory reports the same margin
    co, _ = aa.minco_solve(head, tail, wps, T, s, ctx=anet_ctx)
    traj = aa.Trajectory(T[0], co[0], ctx=anet_ctx)
    m, t, piece = traj.getStopMargin(vm, a_brake, t_react, clearance, res)
    assert m == before["margin"] and 0 <= piece < N and 0.0 <= t <= T.sum() and not traj.checkStoppable(vm, a_brake, t_react, clearance, res)
    assert traj.checkStoppable(vm, a_brake, t_react, clearance + m - 1e-9, res)


# ---------------------------------------------------------------------------------------------
# the directional check
# ---------------------------------------------------------------------------------------------
def _line_piece(x0, v0, acc, y, z):
    """x = x0 + v0 t + acc t^2 / 2 at constant y, z as a degree-5 piece, highest power first"""
    cm = np.zeros((3, 6))
    cm[0, 3:], cm[1, 5], cm[2, 5] = (0.5 * acc, v0, x0), y, z
    return cm


def test_stop_check_against_a_wall_in_closed_form(anet_ctx):
    """A 40 x 8 x 8 map at scale 0.25 with a one-voxel-thick wall of occupied voxels at x index 30 (near face x = 7.5).  Trajectories
    along +x with the speed v0 + acc t: the unsafe samples are exactly those with p_x + t_react v + v^2 / (2 a_brake) >= 7.5 (every
    sample keeps 1e-6 from that boundary); a constant piece in free space is safe, one inside the wall is not."""
    import allocnet_amd as aa
    size, scale, res, a_brake, t_react = (40, 8, 8), 0.25, 10, 4.0, 0.2
    vm = aa.VoxelMap(size, (0.0, 0.0, 0.0), scale, ctx=anet_ctx)
    wall = np.stack(np.meshgrid([30], np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    vm.setOccupied(wall.astype(np.int32))
    T = np.array([[1.5, 1.0], [1.0, 0.9], [0.5, 0.5], [0.5, 0.5]])
    starts = [(1.0, 1.0, 1.0), (0.6, 2.5, 0.8)]
    co = np.zeros((4, 2, 3, 6))
    for b, (x0, v0, acc) in enumerate(starts):
        co[b, 0] = _line_piece(x0, v0, acc, 1.03, 0.91)
        x1, v1 = x0 + v0 * T[b, 0] + 0.5 * acc * T[b, 0] ** 2, v0 + acc * T[b, 0]
        co[b, 1] = _line_piece(x1, v1, 0.5 * acc, 1.03, 0.91)
    co[2, :] = _line_piece(3.1, 0.0, 0.0, 1.03, 0.91)                    # at rest in free space
    co[3, :] = _line_piece(7.6, 0.0, 0.0, 1.03, 0.91)                    # at rest inside the wall
    count, first = aa.traj_stop_check(co, T, vm, a_brake, t_react, res, ctx=anet_ctx)
    sigma = np.arange(res + 1) / res
    for b in range(2):
        reach = []
        for i in range(2):
            t = sigma * T[b, i]
            c = co[b, i, 0]
            x, v = c[5] + c[4] * t + c[3] * t * t, c[4] + 2.0 * c[3] * t
            reach.append(x + t_react * v + v * v / (2.0 * a_brake))
            assert (x < 7.4).all()
        reach = np.concatenate(reach)
        assert np.abs(reach - 7.5).min() >= 1e-6
        unsafe = reach >= 7.5
        print(f"trajectory {b}: {unsafe.sum()} of {len(unsafe)} samples unsafe, first {unsafe.argmax()}")
        assert 0 < unsafe.sum() < len(unsafe)
        assert count[b] == unsafe.sum() and first[b] == unsafe.argmax()
    assert (count[2], first[2]) == (0, -1) and (count[3], first[3]) == (2 * (res + 1), 0)


def test_stop_check_flags_segments_that_end_outside_the_map(anet_ctx):
    """An empty map: the walk passes through the outside of the map and meets nothing, so a stop segment that ends beyond x = 10 is
    flagged through `query` alone."""
    import allocnet_amd as aa
    size, scale, res, a_brake, t_react = (40, 8, 8), 0.25, 10, 4.0, 0.2
    vm = aa.VoxelMap(size, (0.0, 0.0, 0.0), scale, ctx=anet_ctx)
    T = np.array([[1.0]])
    co = _line_piece(5.0, 2.0, 2.0, 1.03, 0.91)[None, None]
    t = np.arange(res + 1) / res * T[0, 0]
    x, v = 5.0 + 2.0 * t + t * t, 2.0 + 2.0 * t
    reach = x + t_react * v + v * v / (2.0 * a_brake)
    assert (x < 9.9).all() and np.abs(reach - 10.0).min() >= 1e-6
    unsafe = reach >= 10.0
    assert 0 < unsafe.sum() < len(unsafe)
    voxel, _ = vm.raycast(np.stack([x, np.full_like(x, 1.03), np.full_like(x, 0.91)], 1),
                          np.stack([reach, np.full_like(x, 1.03), np.full_like(x, 0.91)], 1))
    assert (voxel == aa.HIT_FREE).all()
    count, first = aa.traj_stop_check(co, T, vm, a_brake, t_react, res, ctx=anet_ctx)
    assert count[0] == unsafe.sum() and first[0] == unsafe.argmax()


# ---------------------------------------------------------------------------------------------
# C++
# ---------------------------------------------------------------------------------------------
def test_cpp_members_program(anet_ctx):
    """tests/cpp/test_stop_margin.cpp: getStopMargin of a three-piece quintic trajectory on a 24 x 16 x 12 map with a few occupied
    voxels agrees with Trajectory.getStopMargin within 1e-12, names the same piece, and checkStoppable turns at the margin."""
    import allocnet_amd as aa
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, lib = os.path.join(root, "tests", "cpp", "test_stop_margin.cpp"), os.path.join(root, "allocnet_amd", "lib")
    size, origin, scale = (24, 16, 12), (-1.0, 0.0, 0.25), 0.25
    a_brake, t_react, clearance, res = 3.0, 0.1, 0.2, 12
    ids = np.array([[12, 8, 5], [12, 9, 5], [13, 8, 6], [5, 3, 2]], dtype=np.int32)
    vm = aa.VoxelMap(size, origin, scale, ctx=anet_ctx)
    vm.setOccupied(ids)
    head, tail = np.zeros((1, 3, 3)), np.zeros((1, 3, 3))
    head[0, :, 0], tail[0, :, 0] = (-0.2, 0.8, 1.0), (4.2, 3.1, 2.4)
    wps = np.array([[[1.0, 1.5, 1.2], [2.6, 2.4, 1.9]]])
    T = np.array([[1.1, 0.9, 1.3]])
    co, _ = aa.minco_solve(head, tail, wps, T, 3, ctx=anet_ctx)
    traj = aa.Trajectory(T[0], co[0], ctx=anet_ctx)
    m, t, piece = traj.getStopMargin(vm, a_brake, t_react, clearance, res)
    with tempfile.TemporaryDirectory() as td:
        exe, case = os.path.join(td, "test_stop_margin"), os.path.join(td, "case.txt")
        with open(case, "w") as fh:
            fh.write("%d %d %d %.17g %.17g %.17g %.17g %d\n" % (*size, *origin, scale, len(ids)))
            fh.write("\n".join("%d %d %d" % tuple(i) for i in ids) + "\n")
            fh.write("%.17g %.17g %.17g %d %d\n" % (a_brake, t_react, clearance, res, T.shape[1]))
            for i in range(T.shape[1]):
                fh.write("%.17g " % T[0, i] + " ".join("%.17g" % x for x in co[0, i].reshape(-1)) + "\n")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"), src, "-o", exe,
                        "-L", lib, "-lallocnet_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
        res_ = subprocess.run([exe, case], capture_output=True, text=True, timeout=120)
    assert res_.returncode == 0, res_.stdout + res_.stderr
    out = json.loads(res_.stdout)
    print(out, (m, t, piece))
    assert np.isfinite(m) and abs(out["margin"] - m) <= 1e-12 and abs(out["t"] - t) <= 1e-12 and out["piece"] == piece
    assert out["stoppable"] == int(m >= 0.0) and out["stoppable_loose"] == 1 and out["stoppable_tight"] == 0
