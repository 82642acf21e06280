"""The sequential statement of the quasiseparable posterior sampler (``_quasisep_sample_np``) against dense LAPACK:
fed the unit vectors of its normals it is a linear map S whose S S^T must be the conditional covariance, and at zero
normals it must give the conditional mean.  Also what ``sample_conditional`` checks before it touches the device, and
the C ABI's declarations.  No GPU needed."""
import re
from pathlib import Path

import numpy as np
import pytest

from tinygp_amd import _ffi
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.solvers import QuasisepSolver

import _quasisep_sample_np as so
from _quasisep_cases import CASES

ROOT = Path(__file__).resolve().parents[1]
SIZES = [(5, 3), (70, 40)]


@pytest.mark.parametrize("n,m", SIZES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_linear_map_has_the_conditional_covariance(name, n, m):
    """Bar 1e-12 on every entry of the joint covariance of data and test points and of the mean: the construction
    reaches a few 1e-15 in fp64; the bar leaves room for LAPACK differences and no more."""
    k = CASES[name](q)
    t, noise, r, xt = so.problem(n, m)
    J = k._ssm().J
    xi, eps = so.unit_normals(n, m, J)
    S = np.vstack(so.sample(k, t, noise, np.zeros(n), xt, xi, eps))
    mean = np.vstack(so.sample(k, t, noise, r, xt, np.zeros((n + m, J, 1)), np.zeros((n, 1))))[:, 0]
    wmean, wcov = so.dense(k, t, noise, r, np.concatenate([t, xt]))
    ecov, emean = np.abs(S @ S.T - wcov).max(), np.abs(mean - wmean).max()
    print(f"sample oracle {name} n={n} m={m}: max |S S^T - cov| = {ecov:.2e}, max |mean - dense| = {emean:.2e}")
    assert ecov <= 1e-12 and emean <= 1e-12


def test_a_tie_gets_one_value_and_cosine_draws_once():
    """dt = 0 gives A = I and chol(Q) = 0 exactly; ``Cosine``'s Q is zero in exact arithmetic and falls under the guard
    at every lag, so nothing is drawn past the first point."""
    rng = np.random.default_rng(2)
    for name in sorted(CASES):
        k = CASES[name](q)
        A, Lq = so.process_noise(k, 0.0)
        assert np.array_equal(A, np.eye(len(A))) and not Lq.any(), name
    t, noise, r, xt = so.problem(20, 6)
    k = CASES["matern52"](q)
    xi = rng.standard_normal((26, 3, 4))
    f = so.prior(k, t, xt, xi)
    assert xt[1] == t[6] == t[7]
    assert np.array_equal(f[6], f[7]) and np.array_equal(f[20 + 1], f[6])  # the tie, and the test point on it
    for dt in (1e-9, 0.3, 7.0, 1e3):
        assert not so.process_noise(CASES["cosine"](q), dt)[1].any(), dt


def test_guarded_cholesky():
    rng = np.random.default_rng(3)
    B = rng.standard_normal((5, 5))
    S = B @ B.T
    L = so.chol_psd(S, np.diag(S))
    np.testing.assert_allclose(L, np.linalg.cholesky(S), rtol=1e-12, atol=1e-12)
    v = rng.standard_normal((5, 2))  # rank 2: three columns fall under the guard, L L^T is still S
    S = v @ v.T
    L = so.chol_psd(S, np.diag(S))
    assert np.count_nonzero(np.diag(L)) == 2
    np.testing.assert_allclose(L @ L.T, S, rtol=0, atol=1e-14 * np.abs(S).max())
    assert not so.chol_psd(np.zeros((3, 3)), np.ones(3)).any()


def test_merged_grid_puts_data_before_test_points_at_a_tie():
    cat, order = so.merged_grid([0.0, 1.0, 1.0, 2.0], [1.0, -1.0, 1.0, 2.0])
    np.testing.assert_array_equal(order, [5, 0, 1, 2, 4, 6, 3, 7])


def _bare_solver(n, kernel):
    """A solver without a handle: enough for the checks that run before the device is touched."""
    s = QuasisepSolver.__new__(QuasisepSolver)
    s.n, s._ssm, s.dtype, s._handle = n, kernel._lower_ssm(), np.dtype(np.float64), None
    return s


def test_wrong_shapes_name_the_expected_shape():
    s = _bare_solver(6, CASES["matern32"](q))
    r, xt = np.zeros(6), np.linspace(0.0, 1.0, 3)
    with pytest.raises(ValueError, match=r"xi must have shape \(9, 2\) or \(9, 2, R\); got \(6, 2, 4\)"):
        s.sample_conditional(r, xt, xi=np.zeros((6, 2, 4)), eps=np.zeros((6, 4)))
    with pytest.raises(ValueError, match=r"xi must have shape \(6, 2\) or \(6, 2, R\); got \(6, 3\)"):
        s.sample_conditional(r, xi=np.zeros((6, 3)), eps=np.zeros(6))
    with pytest.raises(ValueError, match=r"eps must have shape \(6, 4\) .* got \(6, 5\)"):
        s.sample_conditional(r, xt, xi=np.zeros((9, 2, 4)), eps=np.zeros((6, 5)))
    with pytest.raises(ValueError, match=r"eps must have shape \(6,\) .* got \(6, 1\)"):
        s.sample_conditional(r, xt, xi=np.zeros((9, 2)), eps=np.zeros((6, 1)))
    with pytest.raises(ValueError, match="X_test must be finite"):
        s.sample_conditional(r, np.array([0.0, np.nan, 1.0]), xi=np.zeros((9, 2)), eps=np.zeros(6))
    with pytest.raises(ValueError, match=r"must have shape \(6, R\); got \(5, 2\)"):
        s._predict_mean_cols(np.zeros((5, 2)), False, xt)


def test_entry_points_are_declared_and_bound():
    header = (ROOT / "include" / "tgp_hip.h").read_text()
    for name, nargs in (("tgp_qsep_sample", 10), ("tgp_qsep_predict_mean", 7)):
        assert re.search(rf"\bint\s+{name}\s*\(", header)
        assert len(_ffi.SIGNATURES[name]) == nargs
