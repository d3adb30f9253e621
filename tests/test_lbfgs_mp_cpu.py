"""The multiprecision L-BFGS reference (tests/lbfgs_mp.py) is pinned before it judges any kernel: its float64 mode replays
the committed traces of the independent restatement, the C port agrees with it on every selected case at a tenth of the bars
the GPU forms are held to, and the selected set takes every exit of the step it claims to take."""
import importlib.util
import json
import math
import os
import re

import numpy as np

from oracle import cbind
from tests import lbfgs_mp as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# the bars of tests/test_lbfgs_forms_gpu.py (f within F_BAR max(1, |f|), x within X_BAR max(1, |x|_inf)); the C port: a tenth
F_BAR, X_BAR = 1.0e-9, 1.0e-8
# every return code a family reaches with margin (lbfgs_mp's docstring has why -1005 is not among them)
REACHED = {0, 1, 2, -1006, -1007, -1008, -1009, -1010, -1011, -1012, L.RUNNING}


def _trace_problem(t, gen):
    """(description or callable, x0) of a committed trace; None where it needs the MVIE data."""
    name, n = t["problem"], len(t["x0"])
    d = L._blank(n)
    if name == "quadratic_n6":
        d["qw"], d["qs"] = np.array([1.0, 4.0, 25.0, 100.0, 400.0, 2500.0]), np.array([1.0, -2.0, 0.5, 3.0, -1.0, 0.25])
    elif name == "quadratic_n12_mem3":
        r = gen.Lcg(7)                       # the generator's own stream: diagonal, shift, then the start point
        d["qw"] = np.array([1.0 + 40.0 * r.u() for _ in range(12)])
        d["qs"] = np.array([r.u() for _ in range(12)])
    elif name.startswith("rosenbrock"):
        d["rosen"] = 1.0
    elif name == "nonsmooth_n5":
        d["qw"], d["qs"] = np.ones(n), np.full(n, 0.3)
        d["ac"][0], d["ac"][1], d["as"][1] = 1.0, 3.0, 1.0
    elif name == "already_stationary":
        d["qw"], d["qs"] = np.array([1.0, 2.0]), np.array([0.5, -0.5])
    elif name == "uphill_direction":
        return (lambda x, ar: (-(x[0] * x[0]), [2.0 * x[0]])), t["x0"]           # the gradient has the wrong sign
    else:
        return None
    return d, t["x0"]


def test_float64_mode_replays_the_committed_traces():
    """Every trace of tests/golden/lbfgs_traces.json that needs no MVIE data, in the float64 mode: counters exact where the
    trace is not order sensitive, x and f within 1e-9 -- the bar the C port is held to (tests/test_lbfgs_cpu.py)."""
    spec = importlib.util.spec_from_file_location("make_lbfgs_traces", os.path.join(HERE, "golden", "make_lbfgs_traces.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    traces = json.load(open(os.path.join(HERE, "golden", "lbfgs_traces.json")))
    replayed, problems = 0, set()
    for t in traces:
        prob = _trace_problem(t, gen)
        if prob is None:
            assert "mvie" in t, t["problem"]
            continue
        desc, x0 = prob
        r = L.run(desc, "f64", x0=x0, **dict(t["params"], max_iterations=t["max_iterations"]))
        key = (t["problem"], t["max_iterations"])
        assert r.status == t["status"], key
        if t["order_sensitive"]:
            assert abs(r.f - t["f"]) <= 2e-3 * max(1.0, abs(t["f"])), key
            continue
        assert (r.k, r.evals) == (t["k"], t["evals"]), key
        tol = 1e-9
        assert np.abs(r.x - np.array(t["x"])).max() <= tol * max(1.0, np.abs(t["x"]).max()), key
        assert abs(r.f - t["f"]) <= tol * max(1.0, abs(t["f"])), key
        replayed += 1
        problems.add(t["problem"])
    assert replayed >= 20 and len(problems) >= 6, (replayed, problems)


def _same_value(a, b, bar):
    if math.isnan(b) or math.isinf(b):
        return (math.isnan(a) and math.isnan(b)) or a == b
    return abs(a - b) <= bar * max(1.0, abs(b))


def test_c_port_agrees_with_the_mp_reference_on_every_selected_case():
    """cbind.lbfgs_optimize (with the built-in bound as its proc_stepbound, the cancel word as its proc_progress) returns the
    mp reference's (status, k, evals) on every selected case, its x and f within ONE TENTH of the bars the GPU forms are held
    to: those bars are not loose for float64 arithmetic in the reference's own order.  (The C port has no evaluation budget:
    the `budget` cases are the mp / f64 / fsum agreement's alone.)"""
    worst_f = worst_x = 0.0
    checked = 0
    for c in L.all_selected():
        mode = L.set_mode(c.set_name)
        if "max_evals" in mode:
            assert c.ref.status in (L.RUNNING, 0, -1012) and c.ref.evals <= mode["max_evals"], c
            continue
        prm, bounded = L.set_params(c.set_name, c.mem_size)
        bound = L.bound_of(c.n) if bounded else None

        def fun(x, desc=c.desc):
            f, g = L.evaluate(desc, x, L._F64)
            return f, np.array(g)
        kw = {}
        if bound is not None:
            kw["stepbound"] = lambda xp, d: L.step_bound(xp, d, *bound)[0]
        if mode.get("cancel"):
            kw["progress"] = lambda *a: 1
        ret, x, f, it, ev = cbind.lbfgs_optimize(c.desc["x0"], fun, cbind.lbfgs_default_param(**prm), **kw)
        r = c.ref
        assert (ret, ev) == (r.status, r.evals), (c, ret, it, ev, r.counters)
        if r.evals > 1:                       # (an already stationary start leaves k unset in lbfgs.hpp)
            assert it == r.k, (c, it, r.k)
        assert _same_value(f, r.f, 0.1 * F_BAR), (c, f, r.f)
        xs = max(1.0, np.abs(r.x).max())
        assert np.abs(x - r.x).max() <= 0.1 * X_BAR * xs, (c, np.abs(x - r.x).max())
        if math.isfinite(r.f):
            worst_f = max(worst_f, abs(f - r.f) / max(1.0, abs(r.f)))
        worst_x = max(worst_x, np.abs(x - r.x).max() / xs)
        checked += 1
    print("C port against the mp reference, %d cases: worst |f - f_mp| / max(1, |f|) = %.3g (bar %.1g), worst |x - x_mp| / "
          "max(1, |x|_inf) = %.3g (bar %.1g)" % (checked, worst_f, 0.1 * F_BAR, worst_x, 0.1 * X_BAR))
    assert checked >= 1000


def test_selected_set_takes_every_exit():
    """Every reached return code at every kernel form's shapes, a skipped cautious update, a max_step second chance that is
    used and does not end in LBFGSERR_MAXIMUMSTEP, ring buffers that wrap, and the margin rule itself."""
    everything = L.all_selected()
    assert {c.ref.status for c in everything} == REACHED
    forms = {}
    for shape, form in L.SHAPES.items():
        assert L.kernel_form(*shape) == form
        got = {c.ref.status for cases in L.selected(*shape).values() for c in cases}
        forms.setdefault(form, set()).update(got)
        # the exits of the step proper at EVERY shape; the two modes (2, RUNNING) at one shape per form
        assert got >= REACHED - {2, L.RUNNING}, (shape, REACHED - got)
    assert len(forms) == 8 and all(got == REACHED for got in forms.values()), forms
    for c in everything:
        assert c.ref.min_margin >= L.MIN_MARGIN
    assert any(c.ref.skipped > 0 and c.ref.k > 1 for c in everything)
    assert any(c.ref.second_chance > 0 and c.ref.status != L.ERR_MAXIMUMSTEP for c in everything)
    assert any(c.ref.status == L.ERR_MAXIMUMSTEP for c in everything)
    for shape in ((32, 1), (32, 3), (65, 1), (65, 3), (32, 8), (128, 8)):       # more accepted steps than history slots
        assert any(c.ref.k - 1 - c.ref.skipped > shape[1] for cases in L.selected(*shape).values() for c in cases), shape
    # failed searches return the reverted point and the last trial's value; -1012 returns the NaN / inf itself
    bad = [c for c in everything if c.ref.status == L.ERR_INVALID_FUNCVAL]
    assert any(math.isnan(c.ref.f) for c in bad) and any(math.isinf(c.ref.f) for c in bad)
    # what the rule drops is dropped for a stated reason, and it does drop: the cliff at the default machine_prec ends in
    # -1007 at 50 digits and in -1009 at float64
    dropped = L.select_cases(32, 8, "default_it12")[1]
    assert any(tag.startswith("cliff") and "mp (-1007" in why for tag, why in dropped), dropped


def test_workgroup_sizes_are_the_headers():
    """lbfgs_mp.FORM_GROUP (the batch sizes of tests/test_lbfgs_forms_gpu.py fill a workgroup and one problem more) against LbfgsWaveShape<MREG>::kWaves."""
    src = open(os.path.join(ROOT, "allocnet_amd", "csrc", "lbfgs_kernels.h")).read()
    m = re.search(r"kWaves = \(LBFGS_WAVE_MREG > 8\) \? (\d+) : \(LBFGS_WAVE_MREG > 0\) \? (\d+) : (\d+);", src)
    assert m, "LbfgsWaveShape::kWaves is no longer written the way this test reads it"
    w20, w8, w0 = (int(v) for v in m.groups())
    for form, (waves, per) in L.FORM_GROUP.items():
        if form != "lane":
            assert waves == {"8": w8, "20": w20, "0": w0}[form[5:form.index(",")]], form
            assert per == (2 if "half" in form else 1)
