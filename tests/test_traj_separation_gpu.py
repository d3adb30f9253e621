"""k_traj_separation on the GPU: against the multiprecision references of tests/golden/traj_separation_cases.npz at the a-priori
bound of tests/traj_separation_mp.separation_bound (met by a float64 restatement of the procedure in
tests/test_traj_separation_cpu.py); the device form's shapes, strides and pair orders; the cutoff; edge inputs; what sampling
overestimates; the Python and C++ facades."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import traj_separation_mp as sp
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "traj_separation_cases.npz"))


@pytest.fixture(scope="module")
def bounds(fx):
    return np.array([sp.fixture_bound(fx, i) for i in range(len(fx["d"]))])


def run_cases(anet_ctx, fx, cutoff):
    """every fixture case alone through the host form -> [(sep, t, piece_a, piece_b)]"""
    import allocnet_amd as aa
    out = []
    for i in range(len(fx["d"])):
        co, T, t0, pair = sp.fixture_case(fx, i)
        sep, t, pieces, pairs = aa.traj_separation(co, T, np.array([pair]), t0, cutoff=cutoff, ctx=anet_ctx)
        assert pairs.tolist() == [list(pair)] and pairs.dtype == np.int32
        out.append((float(sep[0]), float(t[0]), int(pieces[0, 0]), int(pieces[0, 1])))
    return out


@pytest.fixture(scope="module")
def host_answers(anet_ctx, fx):
    return run_cases(anet_ctx, fx, np.inf)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_separation_matches_multiprecision_reference(fx, bounds, host_answers, s):
    """(a) every case of the fixture alone through the host form: |sep - ref| <= bound and sep >= ref - bound; +inf cases exact;
    dist_exact at (t, pieces) reproduces sep within the bound and t lies inside W and both pieces' spans; the reference's pieces
    where the runner-up interval is farther than twice the bound (traj_separation_mp.check_result)."""
    worst = {}
    for i in np.flatnonzero(fx["s"] == s):
        fam = str(fx["families"][fx["family"][i]])
        r = sp.check_result(fx, i, bounds[i], host_answers[i])
        print("case %d %s sep %.17g ref %.17g err/bound %.3g" % (i, fam, host_answers[i][0], fx["d"][i], r))
        worst[fam] = max(worst.get(fam, 0.0), r)
    print("s=%d worst |err| / bound per family:" % s, {k: "%.3g" % v for k, v in worst.items()})
    assert len(worst) == 14


def fleet(fx, N, B=12, s=3):
    """B trajectories of order s with N pieces from the fixture's (cases of at most N pieces, padded with zero durations), start
    times spread so that most pairs share some time"""
    ids = np.flatnonzero((fx["s"] == s) & (fx["n"] <= N) & (fx["pa"] >= 0))
    co = np.zeros((B, N, 3, 2 * s))
    T = np.zeros((B, N))
    for b in range(B):
        c, t, _, _ = sp.fixture_case(fx, ids[(b // 2 * 5) % len(ids)])
        co[b, :c.shape[1]] = c[b % 2]
        T[b, :c.shape[1]] = t[b % 2]
    t0 = 0.375 * (np.arange(B) % 5) - 0.5
    return co, T, t0


_alone = {}


def alone(anet_ctx, key, co, T, t0, a, b):
    """the answer of the pair (a, b) as the only pair of a host call, cached"""
    import allocnet_amd as aa
    if (key, a, b) not in _alone:
        sep, t, pieces, _ = aa.traj_separation(co, T, np.array([[a, b]]), t0, ctx=anet_ctx)
        _alone[(key, a, b)] = (sep[0], t[0], pieces[0, 0], pieces[0, 1])
    return _alone[(key, a, b)]


@pytest.mark.parametrize("P", [1, 65, 130])
@pytest.mark.parametrize("N", [1, 3])
def test_device_form_shapes_strides_and_pair_orders(anet_ctx, fx, N, P):
    """(b) B = 12, ld = B + 19 with junk behind the batch and behind P; diagnostics wanted and NULL; nothing is written outside the
    outputs; every pair gives the bits it gives alone, in any pair order."""
    import allocnet_amd as aa
    import torch
    dev = torch.device("cuda", anet_ctx.device)
    B, s = 12, 3
    ld = B + 19
    co, T, t0 = fleet(fx, N)
    k = np.arange(P)
    pairs = np.stack([(k * 5 + k // 12) % B, (k * 7 + 3) % B], axis=1).astype(np.int32)

    def bm(a):
        out = torch.full((a.reshape(B, -1).shape[1], ld), 7.0, device=dev, dtype=torch.float64)
        out[:, :B] = torch.as_tensor(np.ascontiguousarray(a.reshape(B, -1).T), device=dev)
        return out
    d_co, d_T = bm(co), bm(T)
    d_t0 = torch.full((ld,), 1e300, device=dev, dtype=torch.float64)
    d_t0[:B] = torch.as_tensor(t0, device=dev)

    def run(pr, diagnostics=True):
        pad = lambda x: torch.cat([torch.as_tensor(np.ascontiguousarray(x), device=dev), torch.full((19,), 1 << 30, device=dev, dtype=torch.int32)])
        pa, pb = pad(pr[:, 0])[:P], pad(pr[:, 1])[:P]          # views of longer buffers: junk behind P
        outs = [torch.full((P + 19,), -7.0, device=dev, dtype=torch.float64), torch.full((P + 19,), -7.0, device=dev, dtype=torch.float64),
                torch.full((P + 19,), -7, device=dev, dtype=torch.int32), torch.full((P + 19,), -7, device=dev, dtype=torch.int32)]
        aa.traj_separation_dev(d_co, d_T, pa.contiguous(), pb.contiguous(), s, N, B, t0=d_t0, sep=outs[0],
                               t=outs[1] if diagnostics else False, piece_a=outs[2] if diagnostics else False,
                               piece_b=outs[3] if diagnostics else False, ctx=anet_ctx)
        torch.cuda.synchronize(dev)
        for o in outs:
            assert (o[P:] == -7).all()
        if not diagnostics:
            assert all((o == -7).all() for o in outs[1:])
        return [o[:P].cpu().numpy() for o in outs]
    got = run(pairs)
    assert np.array_equal(run(pairs, diagnostics=False)[0], got[0], equal_nan=True)
    assert (d_co[:, B:] == 7.0).all() and (d_T[:, B:] == 7.0).all() and (d_t0[B:] == 1e300).all()
    finite = 0
    for p in range(P):
        want = alone(anet_ctx, N, co, T, t0, int(pairs[p, 0]), int(pairs[p, 1]))
        assert all(np.array_equal(np.asarray(w, dtype=np.float64), np.asarray(g[p], dtype=np.float64), equal_nan=True) for w, g in zip(want, got)), (p, pairs[p], want)
        finite += np.isfinite(want[0])
    assert finite >= 0.5 * P
    perm = np.random.default_rng(P).permutation(P)
    again = run(pairs[perm])
    for g, h in zip(got, again):
        assert np.array_equal(g[perm].astype(np.float64), h.astype(np.float64), equal_nan=True)
    # the host form on the whole list, and with t0 = NULL
    host = aa.traj_separation(co, T, pairs, t0, ctx=anet_ctx)
    assert np.array_equal(host[0], got[0]) and np.array_equal(host[1], got[1]) and np.array_equal(host[2], np.stack(got[2:], axis=1))
    z = aa.traj_separation(co, T, pairs[:3], None, ctx=anet_ctx)
    z0 = aa.traj_separation(co, T, pairs[:3], np.zeros(B), ctx=anet_ctx)
    assert all(np.array_equal(x, y) for x, y in zip(z, z0))


def test_cutoff(anet_ctx, fx, bounds):
    """(c) a cutoff above every fixture minimum: the results satisfy (a); a cutoff of 0: every result is still at least ref - bound
    and reproduces under dist_exact."""
    assert fx["d"][np.isfinite(fx["d"])].max() < 100.0
    for i, res in enumerate(run_cases(anet_ctx, fx, 100.0)):
        sp.check_result(fx, i, bounds[i], res)
    same = 0
    for i, (sep, t, pa, pb) in enumerate(run_cases(anet_ctx, fx, 0.0)):
        co, T, t0, (a, b) = sp.fixture_case(fx, i)
        if fx["pa"][i] < 0:
            assert (sep, t, pa, pb) == (np.inf, 0.0, -1, -1)
            continue
        Ka, Kb = sp.knots(T[a], t0[a]), sp.knots(T[b], t0[b])
        assert sep >= fx["d"][i] - bounds[i][1], (i, sep, fx["d"][i])
        assert max(Ka[0], Kb[0]) <= t <= min(Ka[-1], Kb[-1]) and Ka[pa] <= t <= Ka[pa + 1] and Kb[pb] <= t <= Kb[pb + 1]
        assert abs(sp.dist_exact(co[a, pa], Ka[pa], co[b, pb], Kb[pb], t) - sep) <= bounds[i][1], i
        same += abs(sep - fx["d"][i]) <= bounds[i][0]
    print("cutoff 0: %d of %d cases still at the exact minimum" % (same, len(fx["d"])))


def test_edge_inputs_poison_only_their_own_pairs(anet_ctx, fx):
    """(d) poisoned pieces, durations and start times; out-of-range indices on the device form; the argument errors."""
    import allocnet_amd as aa
    import torch
    from allocnet_amd import _lib
    dev = torch.device("cuda", anet_ctx.device)
    B, N, s = 12, 3, 3
    co, T, t0 = fleet(fx, N)
    pairs = aa.trajectory.all_pairs(B)
    clean = aa.traj_separation(co, T, pairs, t0, ctx=anet_ctx)
    assert np.isfinite(clean[0]).sum() >= 30 and not np.isnan(clean[0]).any()

    def expect_nan_for(bad_traj, co_, T_, t0_):
        got = aa.traj_separation(co_, T_, pairs, t0_, ctx=anet_ctx)
        hit = (pairs == bad_traj).any(axis=1)
        assert np.isnan(got[0][hit]).all() and (got[1][hit] == 0.0).all() and (got[2][hit] == -1).all()
        for c, g in zip(clean, got):
            assert np.array_equal(c[~hit], g[~hit])
    for bad in (np.nan, np.inf, -np.inf, -1.0):
        Tb = T.copy()
        Tb[4, 1] = bad
        expect_nan_for(4, co, Tb, t0)
    for bad in (np.nan, np.inf):
        tb = t0.copy()
        tb[7] = bad
        expect_nan_for(7, co, T, tb)
    # a poisoned coefficient: NaN for the pairs whose window meets the piece, untouched bits elsewhere
    piece = int(np.flatnonzero(T[2] > 0.0)[0])
    for bad in (np.nan, np.inf, 1e305):
        cb = co.copy()
        cb[2, piece, 1, 0 if bad == 1e305 else 3] = bad
        Tb = T.copy()
        if bad == 1e305:
            Tb[2, piece] = 20.0          # c_k T^k overflows
        got = aa.traj_separation(cb, Tb, pairs, t0, ctx=anet_ctx)
        base = clean if bad != 1e305 else aa.traj_separation(co, Tb, pairs, t0, ctx=anet_ctx)
        K2 = sp.knots(Tb[2], t0[2])
        for p, (a, b) in enumerate(pairs):
            if 2 not in (a, b):
                assert all(np.array_equal(c[p], g[p]) for c, g in zip(base, got))
                continue
            o = b if a == 2 else a
            Ko = sp.knots(Tb[o], t0[o])
            lo, hi = max(K2[0], Ko[0], K2[piece]), min(K2[-1], Ko[-1], K2[piece + 1])
            if lo < hi:
                assert np.isnan(got[0][p]) and got[1][p] == 0.0 and (got[2][p] == -1).all(), (p, a, b)
    # a poisoned piece of zero duration is never read
    cz, Tz = co.copy(), T.copy()
    Tz[5, N - 1] = 0.0
    cz[5, N - 1] = np.nan
    ref = aa.traj_separation(co, Tz, pairs, t0, ctx=anet_ctx)
    got = aa.traj_separation(cz, Tz, pairs, t0, ctx=anet_ctx)
    assert all(np.array_equal(c, g) for c, g in zip(ref, got)) and not np.isnan(got[0]).any()
    # indices outside [0, B) on the device form: NaN for that pair, nothing read
    idx = np.array([[0, 1], [-1, 2], [3, B], [2 ** 31 - 1, 0], [4, 5], [-2 ** 31, -1]], dtype=np.int32)
    d_co = torch.as_tensor(np.ascontiguousarray(co.reshape(B, -1).T), device=dev)
    d_T = torch.as_tensor(np.ascontiguousarray(T.T), device=dev)
    out = aa.traj_separation_dev(d_co, d_T, torch.as_tensor(idx[:, 0].copy(), device=dev), torch.as_tensor(idx[:, 1].copy(), device=dev), s, N, B,
                                 t0=torch.as_tensor(t0, device=dev), ctx=anet_ctx)
    torch.cuda.synchronize(dev)
    sep, t, qa, qb = (o.cpu().numpy() for o in out)
    for p in (1, 2, 3, 5):
        assert np.isnan(sep[p]) and t[p] == 0.0 and qa[p] == -1 and qb[p] == -1
    for p, q in ((0, 0), (4, int(np.flatnonzero((pairs == [4, 5]).all(axis=1))[0]))):
        assert sep[p] == clean[0][q] and t[p] == clean[1][q] and (qa[p], qb[p]) == tuple(clean[2][q])
    with pytest.raises(aa.AnetError):
        aa.traj_separation(co, T, idx[:2], t0, ctx=anet_ctx)
    # argument errors
    lib, h = anet_ctx.lib, anet_ctx.handle
    q = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pa, pb = np.ascontiguousarray(pairs[:4, 0]), np.ascontiguousarray(pairs[:4, 1])
    sep4 = np.full(4, -7.0)
    inf = float("inf")

    def host(s_=s, n_=N, b_=B, np_=4, cut=inf, co_=co, sep_=sep4, pa_=pa):
        return lib.anet_traj_separation(h, s_, n_, b_, q(co_) if co_ is not None else None, q(T), q(t0), np_,
                                        q(pa_) if pa_ is not None else None, q(pb), cut, q(sep_) if sep_ is not None else None, None, None, None)
    assert host() == _lib.ANET_OK and np.array_equal(sep4, clean[0][:4])
    for kw in (dict(s_=1), dict(s_=5), dict(n_=0), dict(n_=17), dict(b_=-1), dict(np_=-1), dict(cut=float("nan")), dict(cut=-1.0),
               dict(co_=None), dict(sep_=None), dict(pa_=None)):
        sep4[:] = -7.0
        assert host(**kw) == _lib.ANET_ERR_INVALID, kw
        assert (sep4 == -7.0).all()
    assert host(np_=0, sep_=None, co_=None) == _lib.ANET_OK and host(b_=0, sep_=None) == _lib.ANET_OK
    dp = lambda x: ctypes.c_void_p(x.data_ptr())
    d_pa, d_sep = torch.as_tensor(pa, device=dev), torch.full((4,), -7.0, device=dev, dtype=torch.float64)
    assert lib.anet_traj_separation_dev(h, s, N, B, B - 1, dp(d_co), dp(d_T), None, 4, dp(d_pa), dp(d_pa), inf, dp(d_sep), None, None, None,
                                        None) == _lib.ANET_ERR_INVALID
    assert lib.anet_traj_separation_dev(h, s, N, B, B, dp(d_co), dp(d_T), None, 4, dp(d_pa), None, inf, dp(d_sep), None, None, None,
                                        None) == _lib.ANET_ERR_INVALID
    assert lib.anet_traj_separation_dev(h, s, N, B, B, None, None, None, 0, None, None, inf, None, None, None, None, None) == _lib.ANET_OK
    torch.cuda.synchronize(dev)
    assert (d_sep == -7.0).all()


def test_sampling_overestimates(anet_ctx, fx, bounds, host_answers):
    """(e) the sampled route -- traj_eval at 21 samples per piece on the merged grid, then a distance -- is never below the exact
    separation minus the bound and exceeds it by more than 1e-4 m somewhere.  (The continuous families: at a jump traj_eval
    names one side, the separation takes both.)"""
    import allocnet_amd as aa
    skip = [list(fx["families"]).index("discont")]
    excess = []
    for i in range(len(fx["d"])):
        if fx["pa"][i] < 0 or fx["family"][i] in skip:
            continue
        co, T, t0, (a, b) = sp.fixture_case(fx, i)
        Ka, Kb = sp.knots(T[a], t0[a]), sp.knots(T[b], t0[b])
        tq = np.concatenate([np.linspace(lo, hi, 21) for lo, hi, _, _ in sp.intervals(Ka, Kb)])
        tq = np.clip(tq, max(Ka[0], Kb[0]), min(Ka[-1], Kb[-1]))
        ka, kb = T[a] > 0.0, T[b] > 0.0          # traj_eval would place the last sample in a padding piece
        pa_ = aa.traj_eval(co[a][ka][None], T[a][ka][None], np.clip(tq - t0[a], 0.0, None)[None], 0, ctx=anet_ctx)[0]
        pb_ = aa.traj_eval(co[b][kb][None], T[b][kb][None], np.clip(tq - t0[b], 0.0, None)[None], 0, ctx=anet_ctx)[0]
        sampled = float(np.linalg.norm(pa_ - pb_, axis=1).min())
        assert sampled >= fx["d"][i] - bounds[i][0], (i, sampled, fx["d"][i])
        assert sampled >= host_answers[i][0] - 2.0 * bounds[i][0], (i, sampled, host_answers[i][0])
        excess.append(sampled - fx["d"][i])
    print("sampled route, 21 samples per piece: median excess %.3g m, worst %.3g m over %d cases" % (np.median(excess), max(excess), len(excess)))
    assert max(excess) > 1e-4


def test_python_facade(anet_ctx, fx):
    """(f) Trajectory.getSeparation / checkSeparation against traj_separation, pieces of different counts padded"""
    import allocnet_amd as aa
    co, T, t0 = fleet(fx, 3)
    trajs = [aa.Trajectory(list(T[b][T[b] > 0.0]), list(co[b][T[b] > 0.0]), ctx=anet_ctx) for b in (0, 5, 8)]
    assert len({tr.getPieceNum() for tr in trajs}) >= 2
    for x, y, bx, by in ((0, 1, 0, 5), (1, 2, 5, 8), (2, 0, 8, 0), (1, 1, 5, 5)):
        d, t, px, py = trajs[x].getSeparation(trajs[y], t0=t0[bx], other_t0=t0[by])
        nx, ny = trajs[x].getPieceNum(), trajs[y].getPieceNum()
        N = max(nx, ny)
        cc, TT = np.zeros((2, N, 3, 6)), np.zeros((2, N))
        cc[0, :nx], TT[0, :nx], cc[1, :ny], TT[1, :ny] = co[bx][T[bx] > 0], T[bx][T[bx] > 0], co[by][T[by] > 0], T[by][T[by] > 0]
        sep, tt, pieces, _ = aa.traj_separation(cc, TT, [[0, 1]], [t0[bx], t0[by]], ctx=anet_ctx)
        assert (d, t, px, py) == (sep[0], tt[0], pieces[0, 0], pieces[0, 1]) and np.isfinite(d)
        if d > 0.0:
            assert trajs[x].checkSeparation(trajs[y], 0.5 * d, t0[bx], t0[by])
            assert trajs[x].checkSeparation(trajs[y], d, t0[bx], t0[by]) and not trajs[x].checkSeparation(trajs[y], d * (1 + 1e-9) + 1e-9, t0[bx], t0[by])
    assert trajs[0].getSeparation(trajs[1], 0.0, 1000.0) == (np.inf, 0.0, -1, -1) and trajs[0].checkSeparation(trajs[1], 1e9, 0.0, 1000.0)
    assert np.isnan(trajs[0].getSeparation(trajs[1], np.nan, 0.0)[0]) and not trajs[0].checkSeparation(trajs[1], 0.0, np.nan, 0.0)
    sep_all = aa.traj_separation(co, T, None, t0, ctx=anet_ctx)
    assert sep_all[3].tolist() == aa.trajectory.all_pairs(12).tolist() and sep_all[0].shape == (66,)


def test_cpp_facade_program(anet_ctx, fx):
    """(f) tests/cpp/test_traj_separation.cpp: getSeparations on a fleet, getSeparation and checkSeparation pair by pair, print
    (%.17g) what the Python facade returns."""
    import allocnet_amd as aa
    co, T, t0 = fleet(fx, 3)
    keep = [T[b] > 0.0 for b in range(6)]
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (2, 2)]
    src = os.path.join(ROOT, "tests", "cpp", "test_traj_separation.cpp")
    lib = os.path.join(ROOT, "allocnet_amd", "lib")
    want = aa.traj_separation(co[:6], T[:6], pairs, t0[:6], ctx=anet_ctx)
    finite = want[0][np.isfinite(want[0]) & (want[0] > 0.0)]
    min_dist = float(np.median(finite))
    with tempfile.TemporaryDirectory() as td:
        txt, exe = os.path.join(td, "case.txt"), os.path.join(td, "test_traj_separation")
        with open(txt, "w") as f:
            f.write("%.17g %d\n" % (min_dist, 6))
            for b in range(6):
                f.write("%.17g %d\n" % (t0[b], keep[b].sum()))
                for d, m in zip(T[b][keep[b]], co[b][keep[b]]):
                    f.write("%.17g\n" % d + " ".join("%.17g" % x for x in m.ravel()) + "\n")
            f.write("%d\n" % len(pairs) + "\n".join("%d %d" % p for p in pairs) + "\n")
        subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                        "-L", lib, "-lallocnet_amd", "-Wl,-rpath," + lib], check=True, capture_output=True)
        res = subprocess.run([exe, txt], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    out = json.loads(res.stdout)
    trajs = [aa.Trajectory(list(T[b][keep[b]]), list(co[b][keep[b]]), ctx=anet_ctx) for b in range(6)]
    for p, (a, b) in enumerate(pairs):
        py = trajs[a].getSeparation(trajs[b], t0[a], t0[b])
        assert tuple(out["single"][p]) == py, (p, out["single"][p], py)
        assert tuple(out["batch"][p]) == (want[0][p], want[1][p], want[2][p, 0], want[2][p, 1])
        assert out["batch"][p][0] == py[0]
        assert bool(out["ok"][p]) == trajs[a].checkSeparation(trajs[b], min_dist, t0[a], t0[b])
    assert 0 < sum(out["ok"]) < len(pairs)
