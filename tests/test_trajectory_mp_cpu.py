"""The multiprecision reference tests/trajectory_mp.py and its fixture tests/golden/max_rate_cases.npz, pinned on the
CPU before any kernel is judged by them: the fixture is what the reference computes, every case keeps its margin
from the constant-rate threshold, the error bound of the GPU tests is met by a plain double-precision restatement of
the modelled procedure, the numpy oracle meets it too, and the new reference agrees with the existing oracle and the
reference-generated golden files where they overlap."""
import itertools
import os
from fractions import Fraction as Fr

import numpy as np
import pytest

from oracle import minco_np as onp
from tests import trajectory_mp as tmp
from tests.util import GOLDEN, golden_files

FIXTURE = os.path.join(GOLDEN, "max_rate_cases.npz")
EPS = tmp.EPS


@pytest.fixture(scope="module")
def fx():
    return np.load(FIXTURE)


def _case(fx, i):
    s = int(fx["s"][i])
    return fx["cm"][i][:, :2 * s].copy(), float(fx["T"][i]), int(fx["which"][i])


def test_fixture_covers_the_families(fx):
    fam, s, which = fx["family"], fx["s"], fx["which"]
    assert 180 <= len(fam) <= 260
    for f in ("plain", "wide_T", "scale", "rest", "one_axis", "multi_root", "cheb", "const"):
        for ss, w in itertools.product((2, 3, 4), (1, 2)):
            assert ((fam == f) & (s == ss) & (which == w)).sum() >= 2, (f, ss, w)
    const = fam == "const"
    assert (fx["dqn"][const] < EPS / 4).sum() >= 10 and (fx["dqn"][const] > 4 * EPS).sum() >= 10
    assert set(fx["T"][fam == "wide_T"]) == {0.05, 0.2, 5.0, 20.0, 50.0}
    biggest = max(os.path.getsize(p) for p in golden_files())
    assert os.path.getsize(FIXTURE) <= biggest


def test_threshold_margin_of_every_case(fx):
    """dq_norm_mp is either below DBL_EPSILON / 4 or above 4 DBL_EPSILON: the branch a float64 implementation takes
    does not depend on its rounding."""
    for i in range(len(fx["T"])):
        n = tmp.dq_norm_mp(*_case(fx, i))
        assert n < Fr(EPS) / 4 or n > 4 * Fr(EPS), (i, str(fx["family"][i]), float(n))
        assert float(n) == fx["dqn"][i]


def test_fixture_is_what_the_reference_computes(fx):
    """every 8th case regenerated: the stored double is the multiprecision value rounded once"""
    for i in range(0, len(fx["T"]), 8):
        cm, T, which = _case(fx, i)
        assert float(tmp.modelled_max_rate_mp(cm, T, which)) == fx["ref"][i], (i, str(fx["family"][i]))
        assert tmp.rate_A(cm, T, which) == fx["A"][i]
        if fx["dqn"][i] < EPS:
            assert fx["ref"][i] == float(tmp.const_branch_rate_mp(cm, T, which))
    # below the threshold the modelled value is NOT the maximum: the const family shows it
    low = [i for i in range(len(fx["T"])) if fx["family"][i] == "const" and fx["dqn"][i] < EPS]
    gaps = [1.0 - fx["ref"][i] / float(tmp.piece_max_rate_mp(*_case(fx, i))) for i in low[::4]]
    assert min(gaps) >= 0.0 and max(gaps) > 0.05, gaps


def _modelled_float64(cm, T, which, roots):
    """Piece::getMaxVelRate / getMaxAccRate in float64 with the root finder replaced by the reference roots rounded to
    double: candidates {0, roots, 1}, each evaluated as getVel / getAcc do (ascending powers, tn *= t, of the piece at
    t = tau * duration), then squared norm, maximum, square root."""
    best = -np.inf
    for tau in [0.0, 1.0] + [float(r) for r in roots]:
        v = onp.piece_eval(cm, tau * T, which)
        best = max(best, float(v @ v))
    return np.sqrt(best)


def test_bound_is_met_by_the_modelled_procedure_in_float64(fx):
    """The tolerance of the GPU test, 32 eps A / T^which, holds for a correct double-precision method: independent of
    the kernel, for every case above the threshold."""
    worst = {}
    for i in range(len(fx["T"])):
        if fx["dqn"][i] < EPS:
            continue
        cm, T, which = _case(fx, i)
        got = _modelled_float64(cm, T, which, tmp.dq_roots_mp(cm, T, which))
        bound = float(tmp.rate_bound(fx["A"][i], T, which))
        ratio = abs(got - fx["ref"][i]) / bound
        fam = str(fx["family"][i])
        worst[fam] = max(worst.get(fam, 0.0), ratio)
        assert ratio <= 1.0, (i, fam, got, fx["ref"][i], bound)
    print("worst |err| / bound per family:", {k: round(v, 4) for k, v in sorted(worst.items())})


def test_numpy_oracle_meets_the_bound(fx):
    """oracle/minco_np.piece_max_rate, the checker of the older GPU tests, against the fixture at the same bound
    (it evaluates the candidates from the component polynomials; from q it misses the cheb family at s = 4, by a factor 2.7)."""
    for i in range(len(fx["T"])):
        cm, T, which = _case(fx, i)
        got = onp.piece_max_rate(cm, T, which)
        bound = float(tmp.rate_bound(fx["A"][i], T, which))
        assert abs(got - fx["ref"][i]) <= bound, (i, str(fx["family"][i]), got, fx["ref"][i], bound)


@pytest.mark.parametrize("s,N", list(itertools.product((2, 3, 4), (3, 1))))
def test_trajectory_fixture_and_oracle(fx, s, N):
    """The stored evaluation / cost / gradient references are what trajectory_mp computes (a sample regenerated), and
    the numpy oracle agrees with them within the bounds the GPU tests use."""
    p = "tr%d%d_" % (s, N)
    coeffs, T, tq = fx[p + "coeffs"], fx[p + "T"], fx[p + "tq"]
    B, nq = tq.shape
    assert coeffs.shape == (B, N, 3, 2 * s) and set(T.ravel()) <= {0.05, 1.0, 20.0}
    for b in range(B):
        for q, d in itertools.product(range(nq), range(4)):
            ref = fx[p + "ev"][b, d, q]
            if (b + q + d) % 5 == 0:
                assert [float(v) for v in tmp.traj_eval_mp(coeffs[b], T[b], tq[b, q], d)] == list(ref)
            got = onp.traj_eval(coeffs[b], T[b], tq[b, q], d)
            assert (np.abs(got - ref) <= tmp.eval_bound(coeffs[b], T[b], tq[b, q], d)).all(), (b, q, d)
        for k, m34 in enumerate((1400.0, 1440.0)):
            ref = fx[p + "cost"][k, b]
            if b % 3 == 0:
                assert float(tmp.traj_cost_mp(coeffs[b], T[b], s, m34)) == ref
                assert [float(g) for g in tmp.traj_cost_grad_T_mp(coeffs[b], T[b], s, m34)] == list(fx[p + "gradT"][k, b])
            assert abs(onp.traj_cost(coeffs[b], T[b], s, m34) - ref) <= tmp.cost_bound(coeffs[b], T[b], s, m34)
    if s == 4:          # the two constants differ where they should
        assert (fx[p + "cost"][0] != fx[p + "cost"][1]).all()
    else:
        assert np.array_equal(fx[p + "cost"][0], fx[p + "cost"][1])


def test_knot_queries_follow_locatePieceIdx(fx):
    """a query exactly at a knot belongs to the piece that ends there, one beyond the end to the last piece"""
    T, tq = fx["tr33_T"], fx["tr33_tq"]
    for b in range(len(T)):
        assert tmp.locate(T[b], tq[b, 0]) == (0, 0.0)
        assert tmp.locate(T[b], tq[b, 3]) == (0, T[b, 0])
        idx, tl = tmp.locate(T[b], tq[b, 2])
        assert idx == 2 and tl > T[b, 2]
        assert tmp.locate(T[b], tq[b, 4])[0] in (1, 2) and tmp.locate(T[b], tq[b, 4]) == onp.locate(T[b], tq[b, 4])


@pytest.mark.parametrize("path", golden_files())
def test_mp_reference_against_reference_generated_golden(path):
    """trajectory_mp on the golden files made by the reference's own code: positions, velocities and accelerations of
    its trajectory.py, 1/2 z'Qz of its Q (m34 = 1400) and torch.autograd's d/dT through its Q(T)."""
    d = np.load(path)
    s, N = int(d["order"]), int(d["N"])
    z = d["z_eq"].reshape(N, 3, 2 * s)
    T = d["T"]
    for k, key in ((0, "eval_pos"), (1, "eval_vel"), (2, "eval_acc")):
        for j in range(0, len(d["eval_t"]), 4):
            got = np.array([float(v) for v in tmp.traj_eval_mp(z, T, d["eval_t"][j], k)])
            assert np.abs(got - d[key][j]).max() <= 1e-12 * max(1.0, np.abs(d[key]).max())
    e = float(tmp.traj_cost_mp(z, T, s, 1400.0))
    assert abs(e - d["e_eq"]) <= 1e-12 * max(1.0, abs(d["e_eq"]))
    g = np.array([float(v) for v in tmp.traj_cost_grad_T_mp(z, T, s, 1400.0)])
    assert np.abs(g - d["dcost_dT"]).max() <= 1e-10 * max(1.0, np.abs(d["dcost_dT"]).max())
    assert (np.abs(g - _oracle_grad_T(z, T, s, 1400.0)) <= tmp.cost_grad_bound(z, T, s, 1400.0)).all()


def _oracle_grad_T(coeffs, T, s, m34):
    """central difference of the oracle's cost would be too coarse: differentiate its cost block term by term"""
    out = np.zeros(len(T))
    for i in range(len(T)):
        _, dQ = tmp.cost_blocks(s, float(T[i]), m34)
        for ax in range(3):
            out[i] += 0.5 * coeffs[i][ax, :s] @ dQ @ coeffs[i][ax, :s]
    return out


@pytest.mark.parametrize("s", [2, 3, 4])
def test_cost_block_is_the_integral(s):
    """oracle/minco_np.cost_block, order 2 included, against the exact integral of the squared s-th derivative, and
    the |Q| the cost bound is built from against the same block"""
    rng = np.random.default_rng(s)
    for T in (0.05, 1.0, 20.0):
        cm = rng.standard_normal((1, 3, 2 * s))
        ref = float(tmp.traj_cost_mp(cm, [T], s, 1440.0))
        assert abs(onp.traj_cost(cm, np.array([T]), s, 1440.0) - ref) <= tmp.cost_bound(cm, [T], s, 1440.0)
        assert np.allclose(tmp.cost_blocks(s, T, 1440.0)[0], onp.cost_block(s, T, 1440.0), rtol=1e-14, atol=0)
        assert np.allclose(tmp.cost_blocks(s, T, 1400.0)[0], onp.cost_block(s, T, 1400.0), rtol=1e-14, atol=0)


def test_generator_reproduces_the_fixture_arrays(fx):
    """the max-rate inputs come out of the generator's seeded construction again (the references are sampled above)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_max_rate_golden", os.path.join(GOLDEN, "make_max_rate_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    cases = gen.rate_cases()
    assert len(cases) == len(fx["T"])
    for i, (fam, s, which, cm, T) in enumerate(cases):
        assert fam == fx["family"][i] and s == fx["s"][i] and which == fx["which"][i] and T == fx["T"][i]
        assert np.array_equal(cm, fx["cm"][i][:, :2 * s])
