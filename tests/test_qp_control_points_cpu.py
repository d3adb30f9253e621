"""CPU suite: the numpy restatement of the control-point row form (tests/qp_control_points_np.py) has the properties the form
rests on -- end-point interpolation, the elevated control values carry the same curve, the curve lies in their hull -- and the
constant, the ctypes prototypes, the Python helpers and the headers agree."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import qp_control_points_np as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    rng = np.random.default_rng(7)
    for s in (3, 4):          # (order 2 is refused by every QP entry point: nothing to restate)
        for K in (1, 2, 3):
            for _ in range(3):
                yield s, K, rng.normal(size=(3, 2 * s)) * rng.uniform(0.1, 3.0), rng.uniform(0.4, 3.0)


@pytest.mark.parametrize("d", [0, 1, 2])
def test_control_values_interpolate_the_segment_ends(d):
    for s, K, coef, T in _cases():
        D = 2 * s
        beta = cp.control_values(coef, T, s, K, d)
        for q in range(K):
            ends = cp.poly_eval(coef, np.array([q * T / K, (q + 1) * T / K]), d)
            scale = max(1.0, np.abs(beta).max())
            assert np.abs(beta[q * D] - ends[0]).max() <= 1e-12 * scale
            assert np.abs(beta[q * D + D - 1] - ends[1]).max() <= 1e-12 * scale


@pytest.mark.parametrize("d", [0, 1, 2])
def test_elevated_control_values_carry_the_curve_and_bound_it(d):
    sigma = np.linspace(0.0, 1.0, 401)
    for s, K, coef, T in _cases():
        D = 2 * s
        beta = cp.control_values(coef, T, s, K, d)
        for q in range(K):
            bq = beta[q * D:(q + 1) * D]
            dense = cp.poly_eval(coef, (q + sigma) * T / K, d)
            scale = max(1.0, np.abs(bq).max())
            # the D elevated values are the degree D - 1 Bernstein coefficients of p^(d) on the segment
            assert np.abs(cp.bernstein_eval(bq, sigma) - dense).max() <= 1e-12 * scale
            # hull: every sample within [min, max] of the control values, per axis (rounding of the samples themselves allowed)
            assert (dense <= bq.max(axis=0) + 1e-12 * scale).all() and (dense >= bq.min(axis=0) - 1e-12 * scale).all()


def test_functionals_are_exact_partitions_of_the_derivative():
    """Exact arithmetic: the rows of derivative 0 sum to one on the constant, the weights of an elevation are convex, and halving a
    segment reproduces the parent's end values -- the three facts the nesting argument uses."""
    for s in (3, 4):
        D = 2 * s
        for K in (1, 2, 4):
            for q in range(K):
                W = cp.functional_exact(s, 0, q, K)
                assert all(W[r][0] == 1 for r in range(D))              # beta^0_r of the constant 1
                for d in (1, 2):
                    Wd = cp.functional_exact(s, d, q, K)
                    assert all(Wd[r][k] == 0 for r in range(D) for k in range(d))
        for d in (0, 1, 2):
            whole = cp.functional_exact(s, d, 0, 1)
            left, right = cp.functional_exact(s, d, 0, 2), cp.functional_exact(s, d, 1, 2)
            assert left[0] == whole[0] and right[D - 1] == whole[D - 1] and left[D - 1] == right[0]


def test_dense_rows_keep_the_sample_forms_shape_and_order():
    polys = [np.arange(8.0).reshape(2, 4) + 1, np.arange(12.0).reshape(3, 4) + 1]
    T = np.array([1.3, 0.7])
    for s in (3, 4):
        for K in (1, 2):
            res = K * 2 * s
            G0, h0 = cp.dense_G_h(s, polys, T, K, 3.0, 4.0, 0)
            G1, h1 = cp.dense_G_h(s, polys, T, K, 3.0, 4.0, 1)
            assert G0.shape == G1.shape == (res * (5 + 24), 3 * 2 * s * 2)
            assert sorted(map(tuple, np.c_[G0, h0])) == sorted(map(tuple, np.c_[G1, h1]))     # the same rows, another order
            piece, kind = cp.row_groups(polys, res)
            assert (h0[kind == 1] == 3.0).all() and (h0[kind == 2] == 4.0).all() and np.isin(h0[kind == 0], [4.0, 8.0, 12.0]).all()
            for i in range(2):      # a row touches its own piece's columns only
                assert not G0[piece == i][:, (1 - i) * 6 * s:(2 - i) * 6 * s].any()


def test_constant_prototypes_and_headers_agree():
    import allocnet_amd as aa
    from allocnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "allocnet_amd.h")).read()
    assert int(re.search(r"#define ANET_QP_ROWS_CONTROL_POINTS (0x[0-9a-fA-F]+)", hdr).group(1), 16) == aa.qp.QP_ROWS_CONTROL_POINTS == 0x100
    assert re.search(r"#define ANET_ABI_VERSION 2\b", hdr) or _lib.load().anet_abi_version() == 2
    # the flag travels in words that exist already: no prototype and no struct layout changed
    assert dict(_lib.QpSettings._fields_)["method"] is ctypes.c_int32
    assert aa.qp.QP_ROWS_CONTROL_POINTS & (aa.qp.QP_METHOD_ADMM | aa.qp.QP_METHOD_INTERIOR_POINT | aa.qp.ORDER_PYTHON) == 0
    st = aa.qp_settings(rows="control_points")
    assert st.method == aa.qp.QP_METHOD_INTERIOR_POINT | 0x100
    assert aa.qp_settings(method=aa.qp.QP_METHOD_ADMM, rows="control_points").method == 0x100
    assert aa.qp_settings(method=st.method, rows="samples").method == aa.qp.QP_METHOD_INTERIOR_POINT
    assert aa.qp_settings().method == aa.qp.QP_METHOD_INTERIOR_POINT
    with pytest.raises(ValueError):
        aa.qp_settings(rows="bernstein")
    assert aa.qp.control_point_res(4) == 8 and aa.qp.control_point_res(3, 3) == 18
    with pytest.raises(ValueError):
        aa.qp.control_point_res(3, 0)
    solver = aa.QPSolver(aa.QPConfig())
    solver.setRowForm("control_points", segments=2)
    with pytest.raises(ValueError):
        solver.setRowForm("control_points", segments=0)
    with pytest.raises(ValueError):
        solver.setRowForm("hull")
    facade = open(os.path.join(ROOT, "include", "allocnet_amd", "qp_solver.hpp")).read()
    assert "setRowForm" in facade and "ANET_QP_ROWS_CONTROL_POINTS" in facade
