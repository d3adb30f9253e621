"""Every L-BFGS update kernel form through every exit of the step, against the multiprecision reference tests/lbfgs_mp.py.

The step logic exists twice in allocnet_amd/csrc: lbfgs_step.h (the lane form k_lbfgs_update and the register-resident form)
and the hand-written copy in lbfgs_update_wave_body (every k_lbfgs_update_wave<...>).  The library exposes no predicate for
the form a shape takes, so the rule of lbfgs_drive (api_lbfgs.hip) is restated in lbfgs_mp.kernel_form and pinned per shape:

    n > 128 or mem_size > 64            k_lbfgs_update (one lane per problem)
    n <= 32, mem_size <= 8              k_lbfgs_update_wave<8, 1, true>   (two problems per wave)
    otherwise <MREG, NV>                MREG = 8 / 20 / 0 for mem_size <= 8 / <= 20 / <= 64,  NV = 1 for n <= 64, else 2

What is compared, for EVERY selected case (lbfgs_mp.select_cases: the mp, float64 and fsum runs agree in their counters and
the mp run keeps a relative margin of 1e-6 at every branch, so no rounding can excuse a mismatch): (status, iters, evals)
exactly; f within 1e-9 max(1, |f|) and x within 1e-8 max(1, |x|_inf) of the 50-digit values (the bars of
test_generic_device_objective_matches_the_restatement; tests/test_lbfgs_mp_cpu.py holds the C port to a tenth of them).  A
failed search returns the reverted point and the last trial's value, -1012 the NaN / inf itself.  A problem still running at
an exhausted budget holds a trial point, not an iterate: its counters are compared, its x and f are not.
"""
import ctypes
import math

import numpy as np
import pytest

from tests import lbfgs_mp as L

pytestmark = pytest.mark.gpu

F_BAR, X_BAR = 1.0e-9, 1.0e-8
GUARD = 64
X_SENTINEL, I_SENTINEL = -7.0, -77
WORST = dict(f=0.0, x=0.0, cases=0)


def _interleaved(cases):
    """Families interleaved: neighbouring columns (and the two halves of a paired wave) hold different families."""
    return sorted(cases, key=lambda c: (c.seed, L.FAMILIES.index(c.family)))


def _run_batch(ctx, cases, ld, set_name, mem_size):
    """One anet_lbfgs_optimize_dev call on the columns `cases` (row stride ld), with guard words around x and the three
    counter rows, NaN in every padded column from the start, and NaN fed to a problem from the evaluation after its last
    (C4: a finished problem is frozen).  Returns per column (status, iters, evals, f, x) as numpy, bits intact."""
    import torch
    import allocnet_amd as aa
    n, B = cases[0].n, len(cases)
    dev = torch.device("cuda", ctx.device)
    prm, bounded = L.set_params(set_name, mem_size)
    mode = L.set_mode(set_name)
    param = aa.lbfgs_parameter_t(**prm)
    pp = ctypes.cast(ctypes.pointer(param), ctypes.c_void_p)
    xflat = torch.full((n * ld + 2 * GUARD,), X_SENTINEL, device=dev, dtype=torch.float64)
    x = xflat[GUARD:GUARD + n * ld].view(n, ld)
    obj = L.TorchBatch([c.desc for c in cases], ld, dev)
    x[:, :B] = obj.x0[:, :B]
    f = torch.zeros(ld, device=dev, dtype=torch.float64)
    g = torch.zeros(n, ld, device=dev, dtype=torch.float64)
    work = torch.empty(ctx.lib.anet_lbfgs_workspace(n, ld, pp), device=dev, dtype=torch.float64)
    iflat = [torch.full((ld + 2 * GUARD,), I_SENTINEL, device=dev, dtype=torch.int32) for _ in range(3)]
    status, iters, evals = (t[GUARD:GUARD + ld] for t in iflat)
    last = torch.zeros(ld, device=dev, dtype=torch.int64)
    last[:B] = torch.tensor([c.ref.evals for c in cases], device=dev)
    calls = [0]
    err = []

    def _cb(_inst, _x, _f, _g, _b, _ld, _n, _stream):
        try:
            calls[0] += 1
            obj(x, f, g)
            dead = last < calls[0]              # finished by the reference's count (and every padded column): garbage from here on
            f[dead] = float("nan")
            g[:, dead] = float("nan")
            return 0
        except Exception as exc:
            err.append(exc)
            return 1
    from allocnet_amd.lbfgs import _EVAL_T
    cb = _EVAL_T(_cb)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    bound_from, bound_min = L.bound_of(n) if bounded else (n, 0.0)
    flag = torch.ones(1, dtype=torch.int32, device=dev) if mode.get("cancel") else None
    if flag is not None:
        ctx.set_cancel_flag(flag)
    try:
        rc = ctx.lib.anet_lbfgs_optimize_dev(ctx.handle, n, B, ld, p(x), p(f), p(g), ctypes.cast(cb, ctypes.c_void_p), None, pp,
                                             int(mode.get("max_evals", 400)), int(bound_from), float(bound_min), p(work),
                                             p(status), p(iters), p(evals), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    finally:
        if flag is not None:
            ctx.set_cancel_flag(None)
    if err:
        raise err[0]
    ctx.check(rc)
    torch.cuda.synchronize()
    # guard words: nothing outside the batch's columns was written
    assert bool((xflat[:GUARD] == X_SENTINEL).all()) and bool((xflat[GUARD + n * ld:] == X_SENTINEL).all()), "x: a write outside the rows"
    assert bool((x[:, B:] == X_SENTINEL).all()), "x: a column past the batch was written"
    for t in iflat:
        assert bool((t[:GUARD] == I_SENTINEL).all()) and bool((t[GUARD + B:] == I_SENTINEL).all()), "a counter row past the batch was written"
    assert bool(torch.isnan(f[B:]).all())
    return (status[:B].cpu().numpy(), iters[:B].cpu().numpy(), evals[:B].cpu().numpy(), f[:B].cpu().numpy(),
            np.ascontiguousarray(x[:, :B].cpu().numpy().T))


def _same_value(a, b, bar):
    if math.isnan(b) or math.isinf(b):
        return (math.isnan(a) and math.isnan(b)) or a == b
    return abs(a - b) <= bar * max(1.0, abs(b))


def _compare(cases, out, tag):
    st, it, ev, f, x = out
    for b, c in enumerate(cases):
        r = c.ref
        assert (int(st[b]), int(it[b]), int(ev[b])) == r.counters, (tag, b, c, (st[b], it[b], ev[b]), r.counters, r.which, r.min_margin)
        if r.status == L.RUNNING:
            continue
        xs = max(1.0, np.abs(r.x).max())
        dx = np.abs(x[b] - r.x).max() / xs
        assert _same_value(float(f[b]), r.f, F_BAR), (tag, b, c, f[b], r.f)
        assert dx <= X_BAR, (tag, b, c, dx)
        if math.isfinite(r.f):
            WORST["f"] = max(WORST["f"], abs(float(f[b]) - r.f) / max(1.0, abs(r.f)))
        WORST["x"] = max(WORST["x"], dx)
        WORST["cases"] += 1


def _bits(out, b):
    st, it, ev, f, x = out
    return (int(st[b]), int(it[b]), int(ev[b]), f[b:b + 1].tobytes(), x[b].tobytes())


@pytest.mark.parametrize("n,mem_size", list(L.SHAPES))
def test_every_form_takes_every_exit(anet_ctx, n, mem_size):
    """C1-C6 at one shape: per parameter set a mixed batch of a filled workgroup plus one problem, the same batch reversed (in
    the paired form every case changes to the other half of its wave), an odd batch of 5, and every case alone -- each compared
    with the mp reference, each frozen once finished (NaN fed from the evaluation after its last; guard words in _run_batch),
    and the bits of a case (x, f, counters) the same in all of them.  The bounded sets run the built-in bound against the
    restatement's; at one shape per form the cancel word (status 2 at k = 1, the iterate of the max_iterations = 1 run) and a
    budget of 3 evaluations (LBFGS_RUNNING with evals == 3)."""
    import allocnet_amd as aa
    form = L.SHAPES[(n, mem_size)]
    assert L.kernel_form(n, mem_size) == form
    waves, per = L.FORM_GROUP[form]
    full = waves * per + 1
    ld = aa.recommended_ld(full)
    seen = set()
    by_set = {}
    for set_name, cases in L.selected(n, mem_size).items():
        cases = _interleaved(cases)
        assert len(cases) >= 3, (set_name, len(cases))
        cols = [cases[i % len(cases)] for i in range(full)]
        runs = {"mixed": (cols, _run_batch(anet_ctx, cols, ld, set_name, mem_size))}
        # reversed, then rotated by one: column b goes to `full - b`, and `full` is odd -- the other half of a paired wave
        back = cols[:1] + cols[:0:-1]
        runs["reversed"] = (back, _run_batch(anet_ctx, back, ld, set_name, mem_size))
        five = [cases[(i + 2) % len(cases)] for i in range(5)]
        runs["five"] = (five, _run_batch(anet_ctx, five, ld, set_name, mem_size))
        alone = {}
        for c in cases:
            out = _run_batch(anet_ctx, [c], ld, set_name, mem_size)
            _compare([c], out, (set_name, "alone"))
            alone[c.id] = _bits(out, 0)
        for name, (cs, out) in runs.items():
            _compare(cs, out, (set_name, name))
            for b, c in enumerate(cs):
                assert _bits(out, b) == alone[c.id], (set_name, name, b, c, "bits depend on the neighbours")
        seen |= {c.ref.status for c in cases}
        by_set[set_name] = (cases, alone)
    assert seen >= {0, 1, -1006, -1007, -1008, -1009, -1010, -1011, -1012}, seen
    if (n, mem_size) in L.MODE_SHAPES:
        assert seen >= {2, L.RUNNING}
        cases, alone = by_set["cancel"]
        it1_cases, it1_alone = by_set["default_it1"]
        first = {(c.family, c.seed): it1_alone[c.id] for c in it1_cases}
        checked = 0
        for c in cases:
            if c.ref.status == 2:
                assert c.ref.k == 1
                one = first.get((c.family, c.seed))
                if one is not None and one[0] == L.ERR_MAXIMUMITERATION:
                    assert alone[c.id][1:] == one[1:], (c, "the cancelled iterate is not the max_iterations = 1 iterate")
                    checked += 1
        assert checked >= 3
        for c in by_set["budget"][0]:
            if c.ref.status == L.RUNNING:
                assert c.ref.evals == 3
    print("shape (%d, %d) %s: worst so far over %d comparisons |f - f_mp| / max(1, |f|) = %.3g, |x - x_mp| / max(1, |x|_inf) = %.3g"
          % (n, mem_size, form, WORST["cases"], WORST["f"], WORST["x"]))


def test_host_callback_entry_takes_every_exit(anet_ctx):
    """anet_lbfgs_optimize_host drives the lane kernel with one problem and the reference's three host callbacks: one case per
    return code (the bound as its proc_stepbound, the cancel word as its proc_progress; it has no evaluation budget), the same
    comparison."""
    import allocnet_amd as aa
    picked = {}
    for set_name, cases in L.selected(33, 8).items():
        if "max_evals" in L.set_mode(set_name):
            continue
        for c in cases:
            picked.setdefault(c.ref.status, c)
    assert set(picked) == {0, 1, 2, -1006, -1007, -1008, -1009, -1010, -1011, -1012}
    for status, c in sorted(picked.items()):
        prm, bounded = L.set_params(c.set_name, c.mem_size)
        kw = {}
        if bounded:
            kw["stepbound"] = lambda xp, d, bnd=L.bound_of(c.n): L.step_bound(xp, d, *bnd)[0]
        if L.set_mode(c.set_name).get("cancel"):
            kw["progress"] = lambda *a: 1

        def fun(x, desc=c.desc):
            f, g = L.evaluate(desc, x, L._F64)
            return f, np.array(g)
        ret, x, f, it, ev = aa.lbfgs_optimize(c.desc["x0"], fun, param=aa.lbfgs_parameter_t(**prm), ctx=anet_ctx, **kw)
        _compare([c], (np.array([ret]), np.array([it]), np.array([ev]), np.array([f]), x[None, :]), ("host", status))
