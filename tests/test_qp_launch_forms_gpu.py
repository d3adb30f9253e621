"""Every launch form of the interior-point QP (csrc/qp_ipm.h, selected in csrc/api_qp.hip qp_ipm_launch_form) against the C port
of the method (oracle/qp_ipm_port.c, itself pinned to the dense oracle):

    FUSE                               k_qp_ipm<s, 1, true>    small batches, lone problems, problems whose LDS fills a CU
    throughput, snap, 2 per CU         k_qp_ipm<4, 2, false>
    throughput, jerk, 1-bounded        k_qp_ipm<3, 1, false>
    throughput, jerk, 3 per CU         k_qp_ipm<3, 3, false>   the instantiation that spills

each of the throughput forms in one launch or two.  `qp_ipm_launch_form` says which one a call took; batches are multiples of the
context's compute units so that the defaults select the same forms on a partitioned device.  The tuning switches are read once
per process: forced forms run in child processes, one at a time."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import qp_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, RES, VMAX, AMAX, TSC = 16, 20, 4.0, 6.0, 1.5
PER_CU, THROUGHPUT, TWO_LAUNCHES = 0x3, 0x10, 0x20      # allocnet_amd.qp.IPM_FORM_*
FEW_SAMPLE_SHAPES = [(4, 1, 1), (4, 1, 2), (4, 1, 3), (4, 1, 4), (4, 2, 2), (3, 1, 1), (3, 1, 2), (3, 2, 1), (4, 2, 1),
                     (3, 16, 3), (3, 1, 20), (4, 1, 20)]

_cache = {}


def _form(f):
    """(throughput?, workgroups per CU, launches) of a qp_ipm_launch_form code"""
    return bool(f & THROUGHPUT), f & PER_CU, 2 if f & TWO_LAUNCHES else 1


def _problem(s, N, seed, B):
    """corridor_problem(seed) at M = 16, durations x 1.5; `state` as tests/soak/soak_qp.py builds it.  Cached, never modified."""
    key = ("problem", s, N, seed, B)
    if key not in _cache:
        from allocnet_amd.synth import corridor_problem
        rng = np.random.default_rng(seed)
        head, tail, wps, T, hp = corridor_problem(rng, B, N, 3, M)
        state = np.ascontiguousarray(np.stack([head, tail], axis=1)[..., :3])
        D = 2 * s
        _cache[key] = dict(head=head, tail=tail, T=T * TSC, hp=hp, state=state,
                           d=rng.normal(size=T.shape) * T * TSC * 0.3,      # one direction in T per problem
                           w1=rng.normal(size=(N, 3, D)), w2=rng.uniform(0.0, 1.0, size=(N, 3, D)))
    return _cache[key]


def _port(s, N, seed, B):
    key = ("port", s, N, seed, B)
    if key not in _cache:
        from oracle import cbind
        p = _problem(s, N, seed, B)
        _cache[key] = cbind.qp_ipm_batch(s, p["state"], p["T"], p["hp"], res=RES, vmax=VMAX, amax=AMAX, tol=1e-9, want_coeffs=True,
                                         nthreads=8)
    return _cache[key]


def _gpu_default(ctx, s, N, seed, B):
    """The batch through the default dispatch with the envelope gradient (shared by the tests that compare it)."""
    key = ("gpu", s, N, seed, B)
    if key not in _cache:
        import allocnet_amd as aa
        p = _problem(s, N, seed, B)
        _cache[key] = aa.qp_solve(s, p["head"], p["tail"], p["hp"], p["T"], res=RES, max_vel=VMAX, max_acc=AMAX, time_grad=True, ctx=ctx)
    return _cache[key]


def _child(code, env_over, timeout=600):
    """One fresh process with the ANET_IPM_* switches of `env_over`; its last output line is JSON.  A child that fails fails the
    test here: nothing further is started."""
    assert all(k.startswith("ANET_IPM_") for k in env_over)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **env_over))
    assert p.returncode == 0, (env_over, p.returncode, p.stdout[-1000:], p.stderr[-3000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_default_dispatch_takes_every_form(anet_ctx):
    """Today's selection rules, stated through the query so that a change of a threshold in tuning.h has to change this test:
    FUSE below 2 * cus + 1 problems; above, snap two per CU and jerk one-bounded; jerk three per CU from 16 * cus problems on where
    three workgroups fit the 160 KB LDS; two launches from 2.25 * cus problems on unless the caller gives a launch order."""
    import allocnet_amd as aa
    cus = anet_ctx.compute_units
    B_fuse, B_two, B_three = 64, 3 * cus, 16 * cus
    q = lambda s, N, B, **kw: _form(aa.qp_ipm_launch_form(s, N, B, **dict(dict(res=RES, M=M, ctx=anet_ctx), **kw)))
    assert q(3, 5, B_fuse) == (False, 1, 1) and q(4, 8, B_fuse) == (False, 1, 1)
    assert q(4, 8, B_two) == (True, 2, 2)
    assert q(3, 5, B_two) == (True, 1, 2)
    assert q(3, 5, B_three) == (True, 3, 2) and q(3, 6, B_three) == (True, 3, 2)
    assert q(3, 7, B_three) == (True, 1, 2)                      # 58 248 B per workgroup: three do not fit
    assert q(3, 16, B_three, res=3, M=6) == (True, 3, 2)         # the longest chain, 51.7 KB per workgroup
    for (s, N, B) in ((4, 8, B_two), (3, 5, B_two), (3, 5, B_three)):
        with_order = q(s, N, B, with_launch_order=True)
        assert with_order == q(s, N, B)[:2] + (1,), (s, N, B, with_order)
    # errors, and the empty batch
    assert aa.qp_ipm_launch_form(3, 5, 0, ctx=anet_ctx) == 0
    for bad in ((2, 5, 64), (3, 0, 64), (3, 5, -1)):
        with pytest.raises(aa.AnetError):
            aa.qp_ipm_launch_form(*bad, ctx=anet_ctx)
    with pytest.raises(aa.AnetError):
        aa.qp_ipm_launch_form(3, 40, 64, res=20, M=16, ctx=anet_ctx)     # does not fit the LDS: the solve refuses it too


@pytest.mark.parametrize("N,seed", [(5, 41), (6, 42)])
def test_three_per_cu_jerk_form_against_the_port(anet_ctx, N, seed):
    """k_qp_ipm<3, 3, false> -- bounded to 168 registers, the only instantiation with scratch, and the one the published jerk
    figure comes from -- on 16 * cus problems in the default environment: objectives and verdicts of the whole batch against the
    port (bars of tests/soak/soak_qp.py and test_randomised_soak_against_the_c_port), and the returned coefficients of sixteen
    problems against the dense rows (bar of test_interior_point_and_backward_pass_random_shapes)."""
    import allocnet_amd as aa
    from tests.test_qp_solve_gpu import _dense
    s, B = 3, 16 * anet_ctx.compute_units
    assert _form(aa.qp_ipm_launch_form(s, N, B, res=RES, M=M, ctx=anet_ctx)) == (True, 3, 2)
    p, ref = _problem(s, N, seed, B), _port(s, N, seed, B)
    g = _gpu_default(anet_ctx, s, N, seed, B)
    gs, ps = g["status"] == 1, ref["status"] >= 1
    both = gs & (ref["status"] == 1)
    rel = np.abs(g["obj"][both] - ref["obj"][both]) / np.maximum(1.0, np.abs(ref["obj"][both]))
    port_only, gpu_only = int((ps & ~gs).sum()), int((gs & ~ps).sum())
    print(f"three per CU N={N}: {B} problems, compared {int(both.sum())} ({both.mean():.4f}), worst objective difference "
          f"{rel.max():.3e}, port only {port_only}, kernel only {gpu_only}")
    assert both.mean() >= 0.90
    assert rel.max() <= 2e-5
    assert port_only <= 0.001 * B and gpu_only <= 0.05 * B, (port_only, gpu_only, B)
    assert np.isfinite(g["grad_T"][both]).all()
    idx = np.nonzero(both)[0]
    idx = idx[::max(1, len(idx) // 16)][:16]
    assert len(idx) == 16
    worst = 0.0
    for b in idx:
        Q, A, bb, G, h = _dense(s, p["head"][b], p["tail"][b], p["hp"][b], p["T"][b], RES, VMAX, AMAX)
        zg = g["coeffs"][b].reshape(-1)
        viol = qp_np.kkt_violation(Q, A, bb, G, h, zg) / max(1.0, np.abs(h).max())
        worst = max(worst, viol)
        assert viol <= 1e-6, (b, viol)
        assert abs(g["obj"][b] - 0.5 * zg @ Q @ zg) <= 1e-9 * max(1.0, abs(g["obj"][b]))      # the objective is that of the coefficients
    print(f"three per CU N={N}: worst scaled violation of the dense rows on 16 problems {worst:.3e}")


def test_three_and_two_per_cu_agree(anet_ctx, tmp_path):
    """The same 16 * cus five-piece jerk problems through k_qp_ipm<3, 3, false> (default) and, in a child process with
    ANET_IPM_THREE_PER_CU_MIN_BATCH=0, through k_qp_ipm<3, 1, false>.  The two instantiations differ in their register bound alone
    (the spills move values, they do not reorder arithmetic) and were measured bit-identical on 4096 problems -- verdicts, Newton
    steps, objectives, coefficients and time gradients --, so that is what is asserted: stricter than the bars of
    test_interior_point_launch_forms_agree (steps within one, objectives within 2e-6, coefficients within 1e-4)."""
    import allocnet_amd as aa
    s, N, seed, B = 3, 5, 41, 16 * anet_ctx.compute_units
    one = _gpu_default(anet_ctx, s, N, seed, B)
    assert _form(aa.qp_ipm_launch_form(s, N, B, res=RES, M=M, ctx=anet_ctx)) == (True, 3, 2)
    out = str(tmp_path / "one_bounded.npz")
    code = ("import sys, json, numpy as np; sys.path.insert(0, %r); import allocnet_amd as aa\n"
            "from allocnet_amd.synth import corridor_problem\n"
            "head, tail, wps, T, hp = corridor_problem(np.random.default_rng(%d), %d, %d, 3, %d)\n"
            "r = aa.qp_solve(%d, head, tail, hp, T * %r, res=%d, max_vel=%r, max_acc=%r, time_grad=True)\n"
            "np.savez(%r, **{k: r[k] for k in ('coeffs', 'obj', 'status', 'iters', 'grad_T')})\n"
            "print(json.dumps(dict(form=aa.qp_ipm_launch_form(%d, %d, %d, res=%d, M=%d))))\n"
            ) % (ROOT, seed, B, N, M, s, TSC, RES, VMAX, AMAX, out, s, N, B, RES, M)
    info = _child(code, dict(ANET_IPM_THREE_PER_CU_MIN_BATCH="0"))
    assert _form(info["form"]) == (True, 1, 2)
    two = np.load(out)
    for k in ("status", "iters", "obj", "coeffs", "grad_T"):
        assert np.array_equal(two[k], one[k], equal_nan=k in ("obj", "coeffs", "grad_T")), k
    assert (one["status"] == 1).mean() > 0.9


_SHAPES_CHILD = r"""
import sys, json, numpy as np
sys.path.insert(0, %(root)r)
import allocnet_amd as aa
from allocnet_amd.synth import corridor_problem
from oracle import cbind
from tests.soak import soak_qp
ctx = aa.default_context(0)
forms = {}
plain_solve = aa.qp_solve
def recording_solve(s, head, tail, hp, T, res=20, **kw):      # what each shape of the soak took
    B, N, Mr = hp.shape[0], hp.shape[1], hp.shape[2]
    forms['%%d,%%d,%%d,%%d,%%d' %% (s, N, Mr, res, B)] = aa.qp_ipm_launch_form(s, N, B, res=res, M=Mr, ctx=ctx)
    return plain_solve(s, head, tail, hp, T, res=res, **kw)
aa.qp_solve = recording_solve
compared, worst, port_only, gpu_only, total = soak_qp.run(40, seed=777, ctx=ctx, verbose=False, batches=(64,))
few = []
for (s, N, res) in %(shapes)r:
    for Mr in (6, 16):
        B = 64
        head, tail, wps, T, hp = corridor_problem(np.random.default_rng(100 * s + 10 * N + res), B, N, 3, Mr)
        T = T * 1.5
        g = aa.qp_solve(s, head, tail, hp, T, res=res, max_vel=4.0, max_acc=6.0, ctx=ctx)
        state = np.ascontiguousarray(np.stack([head, tail], axis=1)[..., :3])
        p = cbind.qp_ipm_batch(s, state, T, hp, res=res, vmax=4.0, amax=6.0, tol=1e-9, want_coeffs=True, nthreads=4)
        gs, ps = g['status'] == 1, p['status'] >= 1
        both = gs & (p['status'] == 1)
        rel = np.abs(g['obj'][both] - p['obj'][both]) / np.maximum(1.0, np.abs(p['obj'][both]))
        few.append(dict(shape=[s, N, res, Mr], disagree=float((gs != ps).mean()), compared=int(both.sum()),
                        port_solved=int((p['status'] == 1).sum()), worst=float(rel.max()) if rel.size else 0.0))
print(json.dumps(dict(soak=[compared, worst, port_only, gpu_only, total], forms=forms, few=few)))
"""


def test_throughput_forms_at_the_shapes_that_break_kernels(anet_ctx):
    """The shapes that found the bugs of the FUSE form -- the forty random shapes of the soak (orders 3 / 4, 1..16 pieces, 6..16
    rows, 3 / 8 / 20 samples, durations x 0.3..4) and the few-sample problems of test_few_samples_per_problem, with one piece (no
    twist) and sixteen (the longest twisted chain) at both ends -- through the throughput forms: children with the two- and
    three-per-CU thresholds at 1, once in two launches and once in one, batches of 64, against the port with the bars of the
    tests the cases come from."""
    seen = set()
    for name, over in (("two launches", dict(ANET_IPM_SPLIT_MIN_BATCH="1")), ("one launch", dict(ANET_IPM_SPLIT_STEPS="0"))):
        env = dict(over, ANET_IPM_TWO_PER_CU_MIN_BATCH="1", ANET_IPM_THREE_PER_CU_MIN_BATCH="1")
        r = _child(_SHAPES_CHILD % dict(root=ROOT, shapes=FEW_SAMPLE_SHAPES), env)
        compared, worst, port_only, gpu_only, total = r["soak"]
        taken = sorted(set(_form(f) for f in r["forms"].values()))
        print(f"{name}: soak compared {compared} of {total}, worst {worst:.3e}, port only {port_only}, kernel only {gpu_only}; "
              f"forms (throughput, per CU, launches) {taken}")
        print(f"{name}: forms by shape (s,N,M,res,B) {r['forms']}")
        assert total == 40 * 64
        assert compared > 0.5 * total
        assert worst <= 2e-5
        assert port_only <= 0.001 * total and gpu_only <= 0.05 * total, (name, port_only, gpu_only, total)
        want_launches = 2 if name == "two launches" else 1
        for f in r["forms"].values():
            thr, per_cu, launches = _form(f)
            assert launches == (want_launches if thr else 1), (name, f)
            seen.add((thr, per_cu))
        assert len(r["few"]) == 2 * len(FEW_SAMPLE_SHAPES)
        for c in r["few"]:
            print(f"{name}: few-sample shape (s,N,res,M) {c['shape']}: verdicts differ {c['disagree']:.4f}, compared {c['compared']}, "
                  f"worst {c['worst']:.3e}")
            assert c["disagree"] <= 0.02, (name, c)
            assert c["worst"] <= 2e-5, (name, c)
            assert c["compared"] > 0 or c["port_solved"] < 32, (name, c)
    assert {(True, 1), (True, 2), (True, 3)} <= seen, seen


def _gradients_against_the_port(ctx, s, N, seed, B, port_tol, sample=None):
    """Backward pass and envelope gradient of a batch against central differences through the PORT along one direction per
    problem.  Returns (usable share, misses of the backward pass, misses of the envelope gradient, usable problems, worst ratios)."""
    import allocnet_amd as aa
    from oracle import cbind
    p = _problem(s, N, seed, B)
    kw = dict(res=RES, max_vel=VMAX, max_acc=AMAX, ctx=ctx)
    tight = aa.qp_settings(method=aa.qp.QP_METHOD_INTERIOR_POINT, eps_abs=1e-10, eps_rel=1e-10)
    base = aa.qp_solve(s, p["head"], p["tail"], p["hp"], p["T"], settings=tight, time_grad=True, **kw)
    gz = p["w1"][None] + p["w2"][None] * base["coeffs"]
    back = aa.qp_solve_vjp(s, p["head"], p["tail"], p["hp"], p["T"], gz, **kw)
    n = min(sample or B, B)
    idx = (np.arange(n) * B) // n                          # the reference on a strided sample, if any; the GPU solves the whole batch
    d = p["d"][idx]

    def port(Tn):
        return cbind.qp_ipm_batch(s, p["state"][idx], Tn, p["hp"][idx], res=RES, vmax=VMAX, amax=AMAX, tol=port_tol, max_iter=200,
                                  want_coeffs=True, nthreads=8)

    def loss(z):
        return (p["w1"] * z).sum(axis=(1, 2, 3)) + 0.5 * (p["w2"] * z * z).sum(axis=(1, 2, 3))
    lp, lm = port(p["T"][idx] + 1e-5 * d), port(p["T"][idx] - 1e-5 * d)
    ok = (base["status"][idx] == 1) & (back["status"][idx] == 1) & (lp["status"] == 1) & (lm["status"] == 1)
    out = [float(ok.mean()), int(ok.sum())]
    for name, grad, fd in (("backward pass", back["grad_T"][idx], (loss(lp["coeffs"]) - loss(lm["coeffs"])) / 2e-5),
                           ("envelope gradient", base["grad_T"][idx], (lp["obj"] - lm["obj"]) / 2e-5)):
        an = (grad * d).sum(axis=1)
        sc = np.abs(grad * d).sum(axis=1) + 1e-300
        ratio = (np.abs(an - fd) / sc)[ok]
        print(f"s={s} N={N} B={B}: {name}: usable {int(ok.sum())} of {n}, |analytic - quotient| / sum|grad_T d|: median "
              f"{np.median(ratio):.2e}, 99th percentile {np.percentile(ratio, 99):.2e}, worst {ratio.max():.2e}, "
              f"above 1e-3: {int((ratio > 1e-3).sum())}")
        out.append(int((ratio > 1e-3).sum()))
    return out


@pytest.mark.parametrize("s,N,seed,per_cu_batch,form", [(3, 5, 41, 3, (True, 1, 2)), (3, 5, 41, 16, (True, 3, 2)), (4, 3, 41, 3, (True, 2, 2))])
def test_backward_pass_and_time_gradient_in_the_throughput_forms(anet_ctx, s, N, seed, per_cu_batch, form):
    """anet_qp_solve_vjp and the envelope gradient of anet_qp_solve_time_grad in the epilogues of the register-bounded
    instantiations (3 * cus and 16 * cus problems; the fixtures and finite differences elsewhere stop at 8 problems, the FUSE
    form).  Reference: central differences (T +- 1e-5 d, one random direction per problem) through the PORT at 1e-10, of an
    arbitrary loss of the coefficients for the backward pass and of the optimal objective for the envelope gradient; bar 1e-3 of
    sum |grad_T d| as in test_interior_point_and_backward_pass_random_shapes.  An active set that changes inside the step
    makes a quotient meaningless: at most 1 % of the usable problems may miss, and 85 % must be usable.
    What the reference alone allows (CPU, 640 problems of seed 41, quotients at steps 1e-5 and 2e-5 against each other in units of
    the bar's own scale, sum |g_i d_i| with g by component differences of the port):
      five jerk pieces:  usable 0.903; loss quotients agree to 1.2e-7 at the 99th percentile (worst 8.0e-6), objective quotients to
                         1.6e-6 (worst 3.5e-6); none above 1e-3.
      three snap pieces: usable 0.884; loss 2.3e-5 at the 99th percentile (worst 2.9e-3, one of 566 above 1e-3), objective 4.0e-5
                         (worst 6.7e-4).  Both inside 1e-4 at the 99th percentile, so three snap pieces at the port tolerance of
                         the jerk case are the snap case (four pieces: 2.4e-4 / 4.4e-4 at 1e-9 and 0.78 usable at 1e-10; five and
                         eight are worse).
    The reference is the whole batch at 3 * cus problems and a strided sample of 640 at 16 * cus (the kernel solves all of them).
    Measured on 256 CUs (misses of the backward pass / of the envelope gradient among the usable problems):
      five jerk pieces,  768 problems, one-bounded:  usable 689 of 768, 6 / 1 above the bar (99th percentile 4.2e-4 / 6.6e-6)
      five jerk pieces, 4096 problems, three per CU: usable 574 of 640, 4 / 0 (1.4e-4 / 2.6e-6)
      three snap pieces, 768 problems, two per CU:   usable 690 of 768, 0 / 0 (2.5e-5 / 2.9e-5; worst 1.0e-4 / 2.1e-4)
    The jerk misses are the REFERENCE's, not an active set that changes: on each of them the FUSE form returns the same
    gradient to 1e-11, the kernel's gradient equals the kernel's own difference quotient to 1e-4, and its objective is the
    dense oracle's at 1e-11 (problem 38 of the 768: 1.734971e-3) where the port at 1e-10 stops a step early (1.735031e-3; its
    tolerance is absolute and these objectives are 1e-3..1e-1) -- at the same step for T + h d and T - h d, so that its quotients
    at two step sizes agree with each other and still differentiate an iterate, not the optimum.  They use most of the 1 %
    allowance (6 of 689): a port that scales its tolerance by the objective would be the better reference."""
    import allocnet_amd as aa
    B = per_cu_batch * anet_ctx.compute_units
    assert _form(aa.qp_ipm_launch_form(s, N, B, res=RES, M=M, ctx=anet_ctx)) == form
    usable, n_ok, miss_vjp, miss_env = _gradients_against_the_port(anet_ctx, s, N, seed, B, port_tol=1e-10,
                                                                   sample=640 if per_cu_batch == 16 else None)
    assert usable >= 0.85, usable
    assert miss_vjp <= 0.01 * n_ok, (miss_vjp, n_ok)
    assert miss_env <= 0.01 * n_ok, (miss_env, n_ok)
