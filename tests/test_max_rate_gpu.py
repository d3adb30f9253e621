"""GPU getMaxVelRate / getMaxAccRate / checkMax*Rate (trajectory.hpp:177-314, 576-630) vs the numpy
restatement (companion-matrix roots) and vs dense sampling of the GPU's own evaluation; and vs the multiprecision
references of tests/golden/max_rate_cases.npz at the a-priori float64 bound of tests/trajectory_mp.rate_bound."""
import math
import os

import numpy as np
import pytest

from oracle import minco_np as onp
from tests import trajectory_mp as tmp
from tests.util import GOLDEN, random_problem

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("s,N", [(4, 8), (3, 5), (3, 16), (2, 3)])
def test_max_rate_matches_oracle(anet_ctx, s, N):
    import allocnet_amd as aa
    rng = np.random.default_rng(3 * s + N)
    B = 70
    head, tail, wps, T = random_problem(rng, B, N, min(3, s))
    coeffs, _ = aa.minco_solve(head, tail, wps, T, s, ctx=anet_ctx)
    # make it harder: add random high-order wiggles to some trajectories (more interior extrema)
    coeffs[::3] += rng.normal(size=coeffs[::3].shape) * 0.05
    for which in (1, 2):
        got = aa.traj_max_rate(coeffs, T, which, ctx=anet_ctx)
        for b in range(0, B, 5):
            for i in range(N):
                ref = onp.piece_max_rate(coeffs[b, i], T[b, i], which)
                assert abs(got[b, i] - ref) <= 1e-8 * max(1.0, ref), (b, i, which, got[b, i], ref)
        # never below a dense sampling of the same polynomial
        for b in range(0, B, 9):
            tq = np.linspace(0, T[b].sum(), 400)[None]
            v = aa.traj_eval(coeffs[b:b + 1], T[b:b + 1], tq, which, ctx=anet_ctx)[0]
            assert np.linalg.norm(v, axis=1).max() <= got[b].max() * (1 + 1e-9) + 1e-12


def test_max_rate_edge_cases_and_class_methods(anet_ctx):
    import allocnet_amd as aa
    D = 6
    cm = np.zeros((3, D))
    cm[:, D - 2] = [1.0, -2.0, 0.5]          # constant velocity, zero acceleration
    cm[:, D - 1] = [0.3, 0.1, 0.0]
    piece = aa.Piece(1.7, cm, ctx=anet_ctx)
    assert abs(piece.getMaxVelRate() - np.linalg.norm([1.0, -2.0, 0.5])) < 1e-12
    assert piece.getMaxAccRate() == 0.0
    assert piece.checkMaxVelRate(2.5) and not piece.checkMaxVelRate(2.0)
    # accelerate-then-brake: the speed maximum is strictly inside the piece
    rng = np.random.default_rng(1)
    head, tail, wps, T = random_problem(rng, 1, 4, 3, rest=True)
    coeffs, _ = aa.minco_solve(head, tail, wps, T, 3, ctx=anet_ctx)
    traj = aa.Trajectory(list(T[0]), list(coeffs[0]), ctx=anet_ctx)
    vmax = traj.getMaxVelRate(); amax = traj.getMaxAccRate()
    ref_v = max(onp.piece_max_rate(coeffs[0, i], T[0, i], 1) for i in range(4))
    ref_a = max(onp.piece_max_rate(coeffs[0, i], T[0, i], 2) for i in range(4))
    assert abs(vmax - ref_v) <= 1e-9 * ref_v and abs(amax - ref_a) <= 1e-9 * ref_a
    assert traj.checkMaxVelRate(vmax * 1.001) and not traj.checkMaxVelRate(vmax * 0.999)
    assert traj.checkMaxAccRate(amax * 1.001) and not traj.checkMaxAccRate(amax * 0.999)


@pytest.fixture(scope="module")
def rate_fx():
    return np.load(os.path.join(GOLDEN, "max_rate_cases.npz"))


def _fill(rate_fx, s, which, B, N):
    """B x N slots filled by cycling through the fixture cases of (s, which) with a stride coprime to their number:
    every lane of every block and every piece row holds a case with a known answer."""
    idx = np.flatnonzero((rate_fx["s"] == s) & (rate_fx["which"] == which))
    stride = next(k for k in range(7, 7 + len(idx)) if math.gcd(k, len(idx)) == 1)
    slot = idx[(np.arange(B * N) * stride) % len(idx)].reshape(B, N)
    assert set(slot.ravel()) == set(idx)
    return slot, rate_fx["cm"][slot][..., :2 * s].copy(), rate_fx["T"][slot].copy()


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("which", [1, 2])
def test_max_rate_matches_multiprecision_reference(anet_ctx, rate_fx, s, which):
    """Every lane of two full 64-lane blocks and a 7-lane tail, all three piece rows, against the 60-digit reference:
    |got - ref| <= 32 eps A / T^which (derived in trajectory_mp.rate_bound, met by a float64 restatement of the
    modelled procedure in tests/test_trajectory_mp_cpu.py).  Below the DBL_EPSILON threshold of trajectory.hpp:190
    (half of the const family) the reference is the modelled rate at t = 0, not the true maximum."""
    import allocnet_amd as aa
    B, N = 135, 3
    slot, coeffs, T = _fill(rate_fx, s, which, B, N)
    got = aa.traj_max_rate(coeffs, T, which, ctx=anet_ctx)
    ratio = np.abs(got - rate_fx["ref"][slot]) / tmp.rate_bound(rate_fx["A"][slot], T, which)
    fam = rate_fx["family"][slot]
    worst = {str(f): float(ratio[fam == f].max()) for f in np.unique(fam)}
    print("s=%d which=%d worst |err| / bound per family: %s" % (s, which, {k: round(v, 4) for k, v in worst.items()}))
    bad = np.argwhere(~(ratio <= 1.0))
    assert len(bad) == 0, [(int(b), int(i), str(fam[b, i]), got[b, i], rate_fx["ref"][slot[b, i]], ratio[b, i])
                           for b, i in bad[:8]]


def test_rest_and_cheb_pieces_through_the_trajectory_class(anet_ctx, rate_fx):
    """Trajectory.getMax*Rate / checkMax*Rate on three fixture pieces (rest, cheb, rest): the maximum over the pieces is
    the maximum of their references, and the check flips within 1e-9 of it."""
    import allocnet_amd as aa
    for which in (1, 2):
        sel = (rate_fx["s"] == 4) & (rate_fx["which"] == which)
        rest = np.flatnonzero(sel & (rate_fx["family"] == "rest"))
        cheb = np.flatnonzero(sel & (rate_fx["family"] == "cheb"))
        for pieces in ([rest[0], cheb[1], rest[1]], [cheb[0], rest[2], cheb[1]]):
            traj = aa.Trajectory([rate_fx["T"][i] for i in pieces], [rate_fx["cm"][i] for i in pieces], ctx=anet_ctx)
            ref = max(rate_fx["ref"][i] for i in pieces)
            bound = max(float(tmp.rate_bound(rate_fx["A"][i], rate_fx["T"][i], which)) for i in pieces)
            get, check = ((traj.getMaxVelRate, traj.checkMaxVelRate) if which == 1 else
                          (traj.getMaxAccRate, traj.checkMaxAccRate))
            assert abs(get() - ref) <= bound, (which, pieces, get(), ref, bound)
            assert check(ref * (1 + 1e-9)) and not check(ref * (1 - 1e-9))
