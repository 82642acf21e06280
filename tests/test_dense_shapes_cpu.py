"""The inputs and references of ``test_gpu_1_solver_shapes.py``, checked without a GPU: the helper's own conditions
at every (N, M) and dtype the GPU file uses, and the helper functions against independent arithmetic."""
import numpy as np
import pytest
import scipy.linalg as sla
from scipy.linalg import lapack

import _dense_np as dn
from oracle import tinygp_np as o

@pytest.mark.parametrize("n,d,dtype", [(n, d, "float64") for n in dn.NS for d in (1, 3)]
                         + [(n, d, "float32") for n in dn.FP32_NS for d in (1, 3)])
def test_factor_conditions_hold_at_every_n(n, d, dtype):
    X, diag = dn.train(n, d, dtype)
    assert X.dtype == diag.dtype == np.dtype(dtype) and X.shape == ((n,) if d == 1 else (n, 3))
    assert X.min() >= 0.0 and X.max() <= (4.0 if d == 1 else 3.0)  # the box does not grow with N
    assert d != 1 or np.all(np.diff(X) >= 0)
    assert diag.min() >= 0.05 - 1e-7 and diag.max() <= 0.15 + 1e-7
    ref = dn.reference(n, d, dtype)  # asserts the tile-norm and cond(K) conditions
    np.testing.assert_allclose(ref.L @ ref.L.T, ref.K, rtol=0, atol=1e-12 * np.abs(ref.K).max() * n)
    assert not ref.L.flags.writeable and not ref.K.flags.writeable


@pytest.mark.parametrize("case", dn.COND_CASES, ids=lambda c: "-".join(map(str, c)))
def test_cross_covariance_condition_and_reference_at_every_case(case):
    d, n, m, xt_given, test_noise, other, dtype = case
    C, var = dn.conditional(*case)  # asserts min|Ks| >= 1e-3 max|Ks| on top of reference()'s conditions
    assert C.shape == (m, m) and var.shape == (m,)
    np.testing.assert_array_equal(C, C.T)
    nz = dn.query_points(m, d, dtype)[1].astype(np.float64) if test_noise else 0.0
    np.testing.assert_allclose(np.diag(C) - nz, var, rtol=1e-12, atol=1e-12)
    if other or m > 65:
        return
    assert var.min() > 0.0  # (with the solver's own kernel; a foreign kernel's "variance" need not be positive)
    # the same matrix from the normal equations: Kss - Ks^T K^-1 Ks
    ref = dn.reference(n, d, dtype)
    kern = dn.kernel(o, d)
    Xt = dn.query_points(m, d, dtype)[0].astype(np.float64) if xt_given else ref.X
    Ks = kern(ref.X, Xt)
    want = kern(Xt, Xt) - Ks.T @ np.linalg.solve(ref.K, Ks) + np.diag(np.broadcast_to(nz, (m,)))
    np.testing.assert_allclose(C, want, rtol=1e-9, atol=1e-9)


def test_every_width_and_public_route_shape_is_covered():
    used = {(c[1], c[2]) for c in dn.COND_CASES}
    assert {(n, m) for n in dn.NS for m in dn.WIDTHS} <= used
    assert {(100, 129), (100, 300)} <= used  # M > N with ragged N
    for n in dn.NS:  # the public-route test: M = 200 in 1-D
        dn.conditional(1, n, 200, True, True, False)


def test_dot_reference_and_bar():
    rng = np.random.default_rng(0)
    L = np.tril(rng.normal(size=(37, 37)))
    Z = rng.normal(size=(37, 5))
    want, mag = dn.dot_reference(L + np.triu(np.full((37, 37), np.nan), 1), Z)  # the upper triangle is never read
    assert want.dtype == np.longdouble
    np.testing.assert_allclose(want.astype(np.float64), L @ Z, rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(mag, np.abs(L) @ np.abs(Z))
    bar = dn.dot_bar(37, np.float64, mag)
    assert np.all(np.abs((L @ Z) - want) <= bar)  # float64 BLAS sits inside its own gamma_N bound
    assert np.all(dn.dot_bar(37, np.float32, mag) > 1e8 * bar)
    # a dropped 128-column tile of L is far outside the bar at every N with more than one tile
    for n in (129, 300, 1100):
        ref, Z = dn.reference(n, 1), dn.rhs(n)[:, :9]
        want, mag = dn.dot_reference(ref.L, Z)
        Lbad = np.array(ref.L)
        Lbad[-1, :dn.TILE] = 0.0
        miss = np.abs(Lbad @ Z - want)[-1]
        assert np.all(miss > 1e6 * dn.dot_bar(n, np.float64, mag)[-1])


def test_solve_reference_and_bars():
    ref = dn.reference(129, 3)
    Y = dn.rhs(129)[:, :7]
    for tr in (False, True):
        X = dn.solve_reference(ref.L, Y, tr)
        np.testing.assert_allclose((ref.L.T if tr else ref.L) @ X, Y, rtol=0, atol=1e-11)
    assert dn.solve_bar(np.float64, np.array([2.0, -4.0])) == (1e-10, 4e-10)
    assert dn.solve_bar(np.float32, np.array([2.0, -4.0])) == (0.0, 8e-3)
    assert dn.posterior_bar(np.float64) == dict(rtol=5e-7, atol=5e-7)
    assert dn.posterior_bar(np.float32) == dict(rtol=5e-4, atol=5e-4)
    assert dn.rhs(300).shape == (300, 300) and not dn.rhs(300).flags.writeable


def test_failing_noise_stops_lapack_in_the_second_tile():
    X, _ = dn.train(300, 1)
    K = dn.kernel(o, 1)(X, X) + np.diag(dn.failing_noise())
    _, info = lapack.dpotrf(K, lower=1)
    assert info == 201 and dn.TILE < info <= 2 * dn.TILE
    assert dn.train(300, 1)[1].min() > 0  # the cached diagonal is untouched
