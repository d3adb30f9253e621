"""The two numerical stages of the batched FIRI (csrc/firi_kernels.h) against the 50-digit reference of tests/firi_mp.py, on
the scene families of tests/firi_scenes.py (which reach all four tangent forms):

  a. the final polytope IS the plane pass of the ellipsoid the device returns (rows, order and count, at rounding level);
  b. every ellipsoid minimises costMVIE of the previous pass's polytope, to the optimiser's own tolerance;
  c. the same for per-corridor pass counts, through the host and the device-pointer entry points;
  d. edges at one pass: the row-count boundary, NaN behind n_points, an endpoint exactly on a box face, exact ties.

Nothing here is compared with a float64 restatement of the same algorithm except the allowance G of (b), which is by its
definition the restatement's own distance from the true minimum.  Measured figures: DESIGN.md 8c."""
import collections

import numpy as np
import pytest

from oracle import firi_np as F
from tests import firi_mp as FM, firi_scenes as S

pytestmark = pytest.mark.gpu

MAX_ROWS = 96
CLOSE = 1e-9            # a reference decision margin below this makes the pass's outcome a matter of rounding
_ref_memo, _dev_memo = {}, {}


def _cases():
    return [c for _, c in S.cases()]


def _dev(ctx, iters):
    """The 24 corridors with a common pass count, once per count (the kernels are deterministic; the suite asserts it)."""
    import allocnet_amd as aa
    if iters not in _dev_memo:
        bd, pc, npts, a, b = S.pack(_cases(), capacity=600 if iters == 2 else None)
        _dev_memo[iters] = aa.firi(bd, pc, a, b, n_points=npts, max_rows=MAX_ROWS, params=aa.firi_params(iterations=iters), ctx=ctx)
    return _dev_memo[iters]


def _ref(idx, ell):
    key = (idx, np.asarray(ell[:15]).tobytes())
    if key not in _ref_memo:
        bd, pts, a, b = _cases()[idx]
        _ref_memo[key] = FM.planes(bd, pts, a, b, ell[:9].reshape(3, 3), ell[9:12], ell[12:15])
    return _ref_memo[key]


class PlaneStats:
    def __init__(self):
        self.passes = self.left_out = self.as_set = 0
        self.worst = 0.0
        self.kinds = collections.Counter()
        self.bad = []

    def check(self, tag, idx, hpoly, n_rows, ell, ref=None):
        """(a) for one corridor: hpoly (H, 4), n_rows, ell (15,) as the device returned them."""
        ref = ref or _ref(idx, ell)
        self.passes += 1
        m = ref["margins"]
        if not (hpoly[n_rows:] == 0).all():
            self.bad.append((tag, idx, "rows behind n_rows are not zero"))
        if min(m["argmin_pt"], m["tangent"], m["cut"]) < CLOSE:
            self.left_out += 1
            return
        r = ell[12:15]
        bar = 1e-12 * (r.max() / r.min()) * np.maximum(1.0, np.abs(ref["rows"]).max(axis=1))
        as_set = m["argmin_bd"] < CLOSE            # two boundary rows tie: either order is a correct pass
        self.as_set += as_set
        w = FM.match_rows(hpoly[:n_rows], ref["rows"], bar, as_set)
        self.worst = max(self.worst, w)
        if not w <= 1.0:
            self.bad.append((tag, idx, "n_rows %d, reference %d, worst row at %.3g bars" % (n_rows, len(ref["rows"]), w)))
        self.kinds.update(int(k) for k in ref["kind"])

    def report(self, what):
        print("%s: %d corridor passes, %d left out (a point within %.0e of a decision), %d compared as a set; worst row at %.3g "
              "of its bar; selected rows by form: boundary %d, plain %d, toward a %d, toward b %d, through a, b, q %d"
              % (what, self.passes, self.left_out, CLOSE, self.as_set, self.worst, self.kinds[-1], self.kinds[0], self.kinds[1],
                 self.kinds[2], self.kinds[3]))

    def verdict(self):
        assert not self.bad, self.bad
        assert 20 * self.left_out <= self.passes, (self.left_out, self.passes)


@pytest.mark.parametrize("iters", [2, 3, 4])
def test_final_polytope_is_the_plane_pass_of_the_returned_ellipsoid(anet_ctx, iters):
    """(a) out["ellipsoid"] is, by the kernels' contract, the ellipsoid the last polytope was built around.  The reference plane
    pass of exactly those doubles must give the same rows in the same order: each within 1e-12 kappa max(1, max|row|), kappa =
    r_max / r_min the condition number of the forward map, i.e. the suite's iterations = 1 bar times kappa.  A pass whose reference
    decision margin is below 1e-9 is compared as a set of rows when the close call is between two boundary rows, and is left
    out when it involves a point (at most 1 pass in 20)."""
    out = _dev(anet_ctx, iters)
    assert (out["ok"] == 1).all(), out["ok"]
    st = PlaneStats()
    for i in range(len(_cases())):
        st.check(iters, i, out["hpoly"][i], int(out["n_rows"][i]), out["ellipsoid"][i])
    st.report("plane pass, iterations = %d" % iters)
    st.verdict()


def test_every_tangent_form_is_reached_on_the_device_ellipsoids(anet_ctx):
    """Coverage of (a), judged by the reference on the DEVICE's ellipsoids: at least 20 selected rows each toward a and toward
    b and at least one through a, b and q over the passes 2 to 4."""
    kinds = collections.Counter()
    for iters in (2, 3, 4):
        out = _dev(anet_ctx, iters)
        for i in range(len(_cases())):
            kinds.update(int(k) for k in _ref(i, out["ellipsoid"][i])["kind"])
    print("selected rows by form on the device's ellipsoids:", dict(kinds))
    assert kinds[1] >= 20 and kinds[2] >= 20 and kinds[3] >= 1, kinds


@pytest.mark.parametrize("k", [2, 3, 4])
def test_each_ellipsoid_minimises_cost_mvie_of_the_previous_polytope(anet_ctx, k):
    """(b) The polytope of pass k-1 (a call with iterations = k-1) and the ellipsoid of pass k (a call with iterations = k).
    With the Chebyshev centre c of that polytope at 50 digits and f* the minimum of costMVIE (BFGS at gtol 1e-10 from two starts,
    both end points scored at 50 digits and required to agree to 1e-9):  f(Q_dev, p_dev) - f* <= max(10 G, 1e-9), G the largest
    such gap of the float64 restatement's own optimisation on the same polytopes.  Ten, because both stop on the same relative
    decrease test (1e-7 over 3 iterations) at different iterates.  On top of that bar, which one hard case of the restatement
    sets for all, a rank statement: the device's MEDIAN gap is at most ten times the restatement's upper quartile -- an
    optimiser that is systematically off (another penalty weight, say) moves every gap, not the worst one."""
    prev, cur = _dev(anet_ctx, k - 1), _dev(anet_ctx, k)
    assert (prev["ok"] == 1).all() and (cur["ok"] == 1).all()
    gaps_dev, gaps_np, left_out = [], [], 0
    for i in range(len(_cases())):
        hp = prev["hpoly"][i, :prev["n_rows"][i]]
        e0, e1 = prev["ellipsoid"][i], cur["ellipsoid"][i]
        c, depth, unique = FM.chebyshev_centre(hp)
        if not unique:
            left_out += 1
            continue
        cf = np.array([float(v) for v in c])
        ok, R, p, r = F.max_vol_ins_ellipsoid(hp, e0[:9].reshape(3, 3), e0[9:12], e0[12:15])
        assert ok
        fs, spread = FM.f_star(hp, c, [FM.x_of_ellipsoid(e0[:9].reshape(3, 3), e0[9:12], e0[12:15], cf), FM.x_of_ellipsoid(R, p, r, cf)])
        if spread > 1e-9:
            left_out += 1
            continue
        gaps_np.append(float(FM.score(hp, c, R, p, r) - fs))
        gaps_dev.append(float(FM.score(hp, c, e1[:9].reshape(3, 3), e1[9:12], e1[12:15]) - fs))
    gaps_dev, gaps_np = np.array(gaps_dev), np.array(gaps_np)
    G = gaps_np.max()
    print("MVIE of pass %d: gap_dev max %.3g median %.3g; restatement G = %.3g, upper quartile %.3g, median %.3g; %d left out"
          % (k, gaps_dev.max(), np.median(gaps_dev), G, np.quantile(gaps_np, 0.75), np.median(gaps_np), left_out))
    assert 20 * left_out <= len(_cases()), left_out
    assert gaps_dev.min() >= -1e-9, gaps_dev.min()             # nothing beats the minimum
    assert gaps_dev.max() <= max(10 * G, 1e-9), (gaps_dev.max(), G, int(gaps_dev.argmax()))
    assert np.median(gaps_dev) <= max(10 * np.quantile(gaps_np, 0.75), 1e-9), (np.median(gaps_dev), np.quantile(gaps_np, 0.75))


def test_pass_counts_per_corridor_through_both_entry_points(anet_ctx):
    """(c) One batch with iterations = [4, 1, 2, 3, ...]: every corridor keeps the polytope of ITS last pass and the ellipsoid
    that polytope was built around (no ellipsoid after the last pass) -- checked as in (a), per corridor, for the host entry
    point and for anet_firi_var_dev."""
    import torch
    import allocnet_amd as aa
    cs = _cases()
    bd, pc, npts, a, b = S.pack(cs)
    its = np.array([4, 1, 2, 3] * (len(cs) // 4), dtype=np.int32)
    host = aa.firi(bd, pc, a, b, n_points=npts, max_rows=MAX_ROWS, iterations=its, ctx=anet_ctx)
    dev = torch.device("cuda", 0)
    t = lambda x, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dtype=dt)
    o = aa.firi_dev(t(bd), t(pc), t(npts, torch.int32), t(a), t(b), max_rows=MAX_ROWS, ctx=anet_ctx, iterations=t(its, torch.int32))
    torch.cuda.synchronize()
    devo = {key: o[key].cpu().numpy() for key in ("hpoly", "n_rows", "ok", "ellipsoid")}
    for name, out in (("host entry", host), ("device-pointer entry", devo)):
        assert (out["ok"] == 1).all(), (name, out["ok"])
        st = PlaneStats()
        for i in range(len(cs)):
            st.check(name, i, out["hpoly"][i], int(out["n_rows"][i]), out["ellipsoid"][i])
            if its[i] == 1:        # one pass: the unit ball at the midpoint, exactly
                assert np.array_equal(out["ellipsoid"][i], np.r_[np.eye(3).ravel(), 0.5 * (a[i] + b[i]), np.ones(3)]), (name, i)
        st.report("mixed pass counts, " + name)
        st.verdict()


def test_batch_of_1_and_65_and_point_capacities_257_and_600(anet_ctx):
    """The 64-lane blocks of k_firi_init / k_firi_mvie_finish (B = 1, 65) and the 256-thread stride of the point loops (capacity
    257 with 257 points; 600): (a) again on what these calls return."""
    import allocnet_amd as aa
    cs = _cases()
    one = [i for i, c in enumerate(cs) if len(c[1]) == 257][0]
    bd, pc, npts, a, b = S.pack([cs[one]])
    assert pc.shape[1] == 257
    out = aa.firi(bd, pc, a, b, n_points=npts, max_rows=MAX_ROWS, params=aa.firi_params(iterations=4), ctx=anet_ctx)
    st = PlaneStats()
    assert out["ok"][0] == 1
    st.check("B=1", one, out["hpoly"][0], int(out["n_rows"][0]), out["ellipsoid"][0])
    idx = [i % len(cs) for i in range(65)]
    bd, pc, npts, a, b = S.pack([cs[i] for i in idx], capacity=600)
    out = aa.firi(bd, pc, a, b, n_points=npts, max_rows=MAX_ROWS, params=aa.firi_params(iterations=3), ctx=anet_ctx)
    assert (out["ok"] == 1).all()
    for q, i in enumerate(idx):
        st.check("B=65", i, out["hpoly"][q], int(out["n_rows"][q]), out["ellipsoid"][q])
    # copies of a corridor in one batch: the same bits (lane 0 of the second block of k_firi_init included)
    for q, i in enumerate(idx):
        assert np.array_equal(out["hpoly"][q], out["hpoly"][i]) and np.array_equal(out["ellipsoid"][q], out["ellipsoid"][i]), q
    st.report("B = 1 / capacity 257 and B = 65 / capacity 600")
    st.verdict()


# ------------------------------------------------------------------------------------------------------------------------------
# (d) edges at one pass: the ellipsoid is the unit ball at the midpoint, kappa = 1


def _unit(a, b):
    return np.r_[np.eye(3).ravel(), 0.5 * (a + b), np.ones(3)]


def _one_pass_reference(c):
    return FM.planes(c[0], c[1], c[2], c[3], np.eye(3), 0.5 * (c[2] + c[3]), np.ones(3))


def _check_one_pass(st, tag, i, c, out, ref=None):
    assert np.array_equal(out["ellipsoid"][i], _unit(c[2], c[3]))
    st.check(tag, i, out["hpoly"][i], int(out["n_rows"][i]), out["ellipsoid"][i], ref=ref or _one_pass_reference(c))


def test_row_count_boundary(anet_ctx):
    """max_rows equal to the reference's row count: ok = 1 with every row.  One less: ok = -1 for that corridor only, and the
    other corridors keep their bits."""
    import allocnet_amd as aa
    cs = [_cases()[i] for i in (0, 3, 9, 16, 20)]
    refs = [_one_pass_reference(c) for c in cs]
    K = [len(r["rows"]) for r in refs]
    top = int(np.argmax(K))
    keep = [i for i in range(len(cs)) if i == top or K[i] < K[top]]      # the corridor with the most rows, alone at the top
    cs, refs, K = [cs[i] for i in keep], [refs[i] for i in keep], [K[i] for i in keep]
    top = int(np.argmax(K))
    assert len(cs) >= 3 and K[top] - 1 >= 4
    bd, pc, npts, a, b = S.pack(cs)
    full = aa.firi(bd, pc, a, b, n_points=npts, max_rows=K[top], params=aa.firi_params(iterations=1), ctx=anet_ctx)
    assert (full["ok"] == 1).all() and list(full["n_rows"]) == K, (full["ok"], full["n_rows"], K)
    st = PlaneStats()
    for i, c in enumerate(cs):
        _check_one_pass(st, "max_rows = K", i, c, full, refs[i])
    st.verdict()
    less = aa.firi(bd, pc, a, b, n_points=npts, max_rows=K[top] - 1, params=aa.firi_params(iterations=1), ctx=anet_ctx)
    others = [i for i in range(len(cs)) if i != top]
    assert less["ok"][top] == -1 and (less["ok"][others] == 1).all(), less["ok"]
    assert np.array_equal(less["n_rows"][others], full["n_rows"][others])
    assert np.array_equal(less["hpoly"][others], full["hpoly"][others][:, :K[top] - 1])
    assert np.array_equal(less["ellipsoid"][others], full["ellipsoid"][others])


@pytest.mark.parametrize("iters", [1, 4])
def test_nan_behind_n_points_changes_no_bit(anet_ctx, iters):
    import allocnet_amd as aa
    cs = [_cases()[i] for i in (0, 5, 11, 17)]
    res = []
    for fill in (0.0, np.nan):
        bd, pc, npts, a, b = S.pack(cs, capacity=513, fill=fill)
        assert np.isnan(pc).any() == np.isnan(fill)
        res.append(aa.firi(bd, pc, a, b, n_points=npts, max_rows=MAX_ROWS, params=aa.firi_params(iterations=iters), ctx=anet_ctx))
    assert (res[0]["ok"] == 1).all()
    for key in ("hpoly", "n_rows", "ok", "ellipsoid"):
        assert np.array_equal(res[0][key], res[1][key]), key


def test_endpoint_exactly_on_a_box_face(anet_ctx):
    """A boundary value of exactly 0 at an endpoint is inside (the reference rejects `> 0` only); one ulp further it is outside."""
    import allocnet_amd as aa
    made = []
    for i in (1, 10, 18):
        bd, pts, a, b = _cases()[i]
        ax = int(np.argmax(a - b))                       # a is the larger along ax: the upper face moves onto a
        bd = bd.copy(); bd[2 * ax, 3] = -a[ax]
        assert (bd @ np.r_[a, 1.0]).max() == 0.0 and (bd @ np.r_[b, 1.0]).max() < 0.0
        made.append((bd, pts[pts[:, ax] < a[ax] - 1e-3], a, b))
    bd, pc, npts, a, b = S.pack(made)
    out = aa.firi(bd, pc, a, b, n_points=npts, max_rows=MAX_ROWS, params=aa.firi_params(iterations=1), ctx=anet_ctx)
    assert (out["ok"] == 1).all(), out["ok"]
    st = PlaneStats()
    for i, c in enumerate(made):
        _check_one_pass(st, "on the face", i, c, out)
        assert F.firi(*c, iterations=1)[0]
    st.verdict()
    bd2 = bd.copy()
    ax = int(np.argmax(a[1] - b[1]))
    bd2[1, 2 * ax, 3] = -np.nextafter(a[1, ax], -np.inf)          # the face one ulp below a: h.a + h3 > 0
    assert (bd2[1] @ np.r_[a[1], 1.0]).max() > 0.0
    out2 = aa.firi(bd2, pc, a, b, n_points=npts, max_rows=MAX_ROWS, params=aa.firi_params(iterations=1), ctx=anet_ctx)
    assert list(out2["ok"]) == [1, 0, 1] and out2["n_rows"][1] == 0
    assert np.array_equal(out2["hpoly"][[0, 2]], out["hpoly"][[0, 2]])


def test_exact_ties_between_points_take_the_first(anet_ctx):
    """Mirror images of a point in the plane z = 1 that holds the segment, all coordinates dyadic: at one pass the forward map is
    the identity, both distances are the same double, the tangent planes differ and neither cuts the other point.  The reference
    (firi.hpp's scan with a strict >) takes the lower index; the rows come out in that order."""
    import allocnet_amd as aa
    a = np.array([0.0, 0.0, 1.0]); b = np.array([1.0, 0.5, 1.0])
    lo = np.array([-1.625, -2.125, -1.625]); hi = np.array([2.5, 2.5, 3.5])      # six different distances from the midpoint
    bd = np.zeros((6, 4))
    for ax in range(3):
        bd[2 * ax, ax] = 1.0; bd[2 * ax, 3] = -hi[ax]
        bd[2 * ax + 1, ax] = -1.0; bd[2 * ax + 1, 3] = lo[ax]
    p = 0.5 * (a + b)
    d = np.array([[0.25, 0.5, 0.75], [-0.5, 0.75, 0.5], [1.0, -0.25, 0.625], [-0.75, -0.5, 0.875], [0.5, -1.0, 0.375]])
    up, down = p + d, p + d * [1, 1, -1]
    # the member above the plane comes first in pairs 0 and 2, the one below in pair 1; pairs 3 and 4 straddle the 256-thread stride
    # (indices 146, 147 against 298, 299); 300 points in all, so that all four waves hold candidates
    first = np.where((np.arange(5) % 2 == 0)[:, None], up, down); second = np.where((np.arange(5) % 2 == 0)[:, None], down, up)
    rng = np.random.default_rng(4)
    far = p + rng.uniform(1.7, 1.9, size=(290, 1)) * (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(290, 3)))
    pts = np.vstack([first[:3], far[:140], second, far[140:], first[3:]])
    assert (np.linalg.norm(up - p, axis=1) == np.linalg.norm(down - p, axis=1)).all()
    c = (bd, pts, a, b)
    ref = _one_pass_reference(c)
    m = ref["margins"]
    assert m["argmin_pt"] == 0.0 and m["argmin_bd"] > 1e-3 and min(m["tangent"], m["cut"]) > 1e-3, m      # ties, and nothing else close
    tied = [i for i in ref["index"][ref["kind"] >= 0] if i < 3 or 143 <= i < 148 or i >= 298]
    assert len(tied) == 10                                  # every one of the ten is selected
    bdp, pc, npts, aa_, bb_ = S.pack([c])
    out = aa.firi(bdp, pc, aa_, bb_, n_points=npts, max_rows=MAX_ROWS, params=aa.firi_params(iterations=1), ctx=anet_ctx)
    assert out["ok"][0] == 1 and out["n_rows"][0] == len(ref["rows"])
    k = len(ref["rows"])
    err = np.abs(out["hpoly"][0, :k] - ref["rows"]).max(axis=1) / np.maximum(1.0, np.abs(ref["rows"]).max(axis=1))
    print("exact ties: %d rows, worst %.3g of the 1e-12 bar" % (k, err.max() / 1e-12))
    assert err.max() <= 1e-12, (err.argmax(), ref["kind"][err.argmax()], ref["index"][err.argmax()])
