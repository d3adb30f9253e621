"""tests/firi_mp.py (the 50-digit FIRI reference the GPU tests of tests/test_firi_stages_gpu.py stand on) against the float64
restatement oracle/firi_np.py + oracle/lbfgs_oracle.c, on the restatement's own ellipsoids; the branch coverage of the scene
families of tests/firi_scenes.py; and the true minimiser of costMVIE those GPU tests measure the device's ellipsoids against.
The two sides share no code: where they agree to 1e-12, a mistake would have to be made twice, independently."""
import collections

import numpy as np
import pytest

from oracle import cbind, firi_np as F
from tests import firi_mp as FM, firi_scenes as S

pytest.importorskip("mpmath")

CLOSE = 1e-9
_memo = {}


def _trace():
    """[(family, case, trace of F.firi with 4 passes, [reference plane pass of each trace ellipsoid])], computed once."""
    if "t" not in _memo:
        out = []
        for fam, c in S.cases():
            tr = []
            ok, _ = F.firi(*c, iterations=4, trace=tr)
            assert ok and len(tr) == 4
            out.append((fam, c, tr, [FM.planes(c[0], c[1], c[2], c[3], t["R"], t["p"], t["r"]) for t in tr]))
        _memo["t"] = out
    return _memo["t"]


def test_scene_families_keep_their_promises():
    cs = S.cases()
    assert len(cs) == 24 and [f for f, _ in cs] == ["scene"] * 8 + ["hug"] * 8 + ["wall"] * 8
    n = [len(c[1]) for _, c in cs]
    assert min(n) >= 25 and max(n) == 400 and 257 in n
    for fam, (bd, pts, a, b) in cs:
        dd = b - a
        t = np.clip(((pts - a) @ dd) / (dd @ dd), 0, 1)
        assert np.linalg.norm(pts - (a + t[:, None] * dd), axis=1).min() > 0.05                 # clear of the segment
        assert (pts @ bd[:, :3].T + bd[:, 3]).max() < 0.0 and (bd @ np.r_[a, 1.0]).max() < 0 and (bd @ np.r_[b, 1.0]).max() < 0
        L = np.linalg.norm(dd)
        if fam == "hug":
            assert 2.5 <= L <= 6.0
            off = np.linalg.norm(np.cross(pts - a, dd / L), axis=1)                             # distance from the LINE
            assert (off <= 0.5).sum() >= 0.45 * len(pts)
        if fam == "wall":
            assert abs(L - 2.5) < 1e-12


def test_plane_pass_matches_the_restatement():
    """Same count, same order, rows to 1e-12 max(1, |row|), on every trace ellipsoid of every family.  A pass where the reference's
    margin between two boundary rows is below 1e-9 (pass 1: the box is symmetric about the midpoint, opposite faces tie exactly and
    float64 rounding orders them either way) is compared as a set; one where a point is within 1e-9 of a decision is left out."""
    worst, left_out, as_set, passes = 0.0, 0, 0, 0
    for fam, c, tr, refs in _trace():
        for k, (t, ref) in enumerate(zip(tr, refs)):
            passes += 1
            m = ref["margins"]
            if min(m["argmin_pt"], m["tangent"], m["cut"]) < CLOSE:
                left_out += 1
                continue
            bar = 1e-12 * np.maximum(1.0, np.abs(ref["rows"]).max(axis=1))
            tie = m["argmin_bd"] < CLOSE
            as_set += tie
            assert not tie or k == 0, (fam, k, m)
            w = FM.match_rows(t["hPoly"], ref["rows"], bar, as_set=tie)
            assert w <= 1.0, (fam, k, w, t["hPoly"].shape, ref["rows"].shape)
            worst = max(worst, w)
    print("plane pass vs restatement: %d passes, %d as a set, %d left out, worst row at %.3g of its bar" % (passes, as_set, left_out, worst))
    assert 20 * left_out <= passes


def test_every_branch_is_reached_with_room_to_spare():
    """On the restatement's ellipsoids, passes 2 to 4: at least 20 selected rows toward a and toward b each and 5 through a, b
    and q; the wall seeds give at least 5 selected rows of form 3 whose own `> eps` tests are 1e-3 clear of their threshold.
    Margins: every class that involves a point above 1e-9 in at least 19 of 20 passes, over all four passes; the class between two
    boundary rows over passes 2 to 4 (in pass 1 opposite faces of the box tie by construction, which the comparison handles as a
    set and which no pass after the first inherits)."""
    kinds, forms = collections.Counter(), collections.Counter()
    wall3 = 0
    close = collections.Counter()
    passes = 0
    for fam, c, tr, refs in _trace():
        for k, ref in enumerate(refs):
            passes += 1
            for name, v in ref["margins"].items():
                if v < CLOSE and not (name == "argmin_bd" and k == 0):
                    close[name] += 1
            if k == 0:
                continue
            kinds.update(int(x) for x in ref["kind"]); forms.update(int(x) for x in ref["form"])
            if fam == "wall":
                wall3 += sum(1 for kd, i in zip(ref["kind"], ref["index"]) if kd == 3 and ref["pt_margin"][i] > 1e-3)
    print("selected rows by form:", dict(kinds), "points by form:", dict(forms), "wall form-3 rows with margin > 1e-3:", wall3,
          "close calls:", dict(close))
    assert kinds[1] >= 20 and kinds[2] >= 20 and kinds[3] >= 5, kinds
    assert wall3 >= 5
    for name in ("argmin_bd", "argmin_pt", "tangent", "cut"):
        assert 20 * close[name] <= passes, (name, close[name], passes)


def _iterates(A, x0):
    xs = []
    prm = cbind.lbfgs_default_param(mem_size=18, g_epsilon=0.0, min_step=1e-32, past=3, delta=1e-7)
    cbind.lbfgs_optimize(x0, lambda x: cbind.cost_mvie(A, 1e-2, 1e3, x), prm, progress=lambda x, g, fx, step, k, ls: xs.append(x) or 0)
    return xs


def test_cost_matches_the_restatement_at_its_iterates():
    """firi_mp.cost_mvie (a function of the ellipsoid) against oracle_cost_mvie (a function of the nine variables) at the
    iterates of the restatement's L-BFGS, to 1e-12 of the sum of the magnitudes of the terms -- the penalty and the three
    logarithms; relative to the value alone is not what a float64 sum can promise near a unit-volume ellipsoid, where they
    cancel."""
    worst, n = 0.0, 0
    for fam, c, tr, refs in _trace()[::3]:
        for k in range(3):
            hp = tr[k]["hPoly"]
            st = F.mvie_setup(hp, tr[k]["R"], tr[k]["p"], tr[k]["r"])
            _, interior, A, x0 = st
            xs = _iterates(A, x0)
            for x in [x0] + xs[:3] + xs[-2:]:
                f, _ = cbind.cost_mvie(A, 1e-2, 1e3, x)
                ref, mag = FM.cost_mvie(hp, interior, FM.factor_q(x, np.finfo(np.float64).eps), x[:3] + interior, parts=True)
                err = abs(f - float(ref)) / max(float(mag), abs(float(ref)))
                worst = max(worst, err); n += 1
                assert err <= 1e-12, (fam, k, f, float(ref), err)
    print("cost_mvie vs restatement: %d iterates, worst %.3g" % (n, worst))


def test_true_minimiser_is_pinned_and_the_restatement_is_near_it():
    """f*: BFGS at gtol 1e-10 from the set-up's x0 and from the restatement's end point, both scored at 50 digits, agree to 1e-9 on
    every committed case and pass; every Chebyshev centre is a non-degenerate vertex, and the polished centre is the
    restatement's (exact enumeration) to rounding.  The restatement's own gap G is printed: it is the allowance of the GPU test."""
    G, worst_spread = [], 0.0
    for fam, c, tr, refs in _trace():
        for k in range(3):
            hp = tr[k]["hPoly"]
            cc, depth, unique = FM.chebyshev_centre(hp)
            assert unique, (fam, k)
            cf = np.array([float(v) for v in cc])
            st = F.mvie_setup(hp, tr[k]["R"], tr[k]["p"], tr[k]["r"])
            assert np.abs(cf - st[1]).max() <= 1e-12 * max(1.0, np.abs(cf).max()) and abs(float(depth) - st[0]) <= 1e-12
            x0 = FM.x_of_ellipsoid(tr[k]["R"], tr[k]["p"], tr[k]["r"], cf)
            assert np.abs(x0 - st[3]).max() <= 1e-12 * max(1.0, np.abs(x0).max())
            nxt = tr[k + 1]
            fs, spread = FM.f_star(hp, cc, [x0, FM.x_of_ellipsoid(nxt["R"], nxt["p"], nxt["r"], cf)])
            worst_spread = max(worst_spread, spread)
            assert spread <= 1e-9, (fam, k, spread)
            gap = float(FM.score(hp, cc, nxt["R"], nxt["p"], nxt["r"]) - fs)
            assert gap >= -1e-9, (fam, k, gap)
            G.append(gap)
    G = np.array(G)
    print("restatement's gap above f*: max %.3g, upper quartile %.3g, median %.3g; largest spread of f* %.3g"
          % (G.max(), np.quantile(G, 0.75), np.median(G), worst_spread))
