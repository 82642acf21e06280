"""Conditional mean and variance at test points in O(N + M) on the device (``QuasisepSolver.predict_mean_var`` and
the two hooks ``GaussianProcess`` reaches it through) against dense LAPACK, the sequential oracle and DirectSolver.

The bar is the project's posterior bar, rtol = atol = 5e-7 (README "Parity"), for kernels of amplitude O(1)."""
import numpy as np
import pytest

from tinygp_amd import GaussianProcess
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.noise import Diagonal
from tinygp_amd.solvers import DirectSolver, QuasisepSolver

import _quasisep_predict_np as po
from _quasisep_cases import CASES
from _quasisep_edges import _test_points

pytestmark = pytest.mark.gpu

BAR = dict(rtol=5e-7, atol=5e-7)
LC = 16  # chunk length below 65 536 points


def _jitter(dtype):
    """``condition`` adds sqrt(eps) to the predictive variance when no noise is given for the test points."""
    return np.sqrt(np.finfo(dtype).eps)


def _series(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, 0.05 * n + 1, n))
    return t, rng.uniform(0.05, 0.2, n), rng.standard_normal(n)


def _report(tag, mean, var, wmean, wvar):
    print(f"{tag}: max |mean - ref| = {np.abs(mean - wmean).max():.3e}, max |var - ref| = "
          f"{np.abs(var - wvar).max():.3e}, min var = {wvar.min():.3e}")


@pytest.mark.parametrize("n", [515, 1999])
@pytest.mark.parametrize("name", sorted(CASES))
def test_vs_dense(name, n):
    k = CASES[name](q)
    t, noise, r = _series(n, seed=n + len(name))
    t[7] = t[6]
    t[LC] = t[LC - 1]  # a tie across a chunk boundary
    xt = np.concatenate([_test_points(t, 300, seed=n), t[[6, 7, LC - 1, LC]]])
    s = QuasisepSolver(k, t, Diagonal(noise))
    mean, var = s.predict_mean_var(r, xt)
    assert mean.shape == var.shape == xt.shape and mean.dtype == var.dtype == np.float64
    wmean, wvar = po.dense(k, t, noise, r, xt)
    _report(f"{name} n={n}", mean, var, wmean, wvar)
    np.testing.assert_allclose(mean, wmean, **BAR)
    np.testing.assert_allclose(var, wvar, **BAR)
    # (M, 1) input, the mean alone, and the variance alone through the hook
    np.testing.assert_array_equal(s.predict_mean_var(r, xt[:, None], return_var=False), mean)
    np.testing.assert_array_equal(s.condition_variance(k, xt), var)


@pytest.mark.parametrize("n", [1, 2, 16, 17])
def test_tiny_series(n):
    k = CASES["m32cos_plus_sho"](q)
    t, noise, r = _series(n, seed=n)
    xt = np.concatenate([t, [t[0] - 0.5, t[-1] + 0.5, 0.5 * (t[0] + t[-1])]])
    mean, var = QuasisepSolver(k, t, Diagonal(noise)).predict_mean_var(r, xt)
    wmean, wvar = po.dense(k, t, noise, r, xt)
    np.testing.assert_allclose(mean, wmean, **BAR)
    np.testing.assert_allclose(var, wvar, **BAR)


def test_all_test_points_in_one_interval():
    k = CASES["celerite4"](q)
    t, noise, r = _series(700, seed=1)
    xt = np.random.default_rng(2).uniform(t[300], t[301], 257)
    mean, var = QuasisepSolver(k, t, Diagonal(noise)).predict_mean_var(r, xt)
    wmean, wvar = po.dense(k, t, noise, r, xt)
    np.testing.assert_allclose(mean, wmean, **BAR)
    np.testing.assert_allclose(var, wvar, **BAR)


LARGE = {"matern32": 0, "m32cos_plus_sho": 1}  # J = 2 and J = 6


def _large_problem(name, n):
    t, _, r = _series(n, seed=20 + LARGE[name])
    xt = _test_points(t, 4096, seed=n, lc=16 if n <= 1 << 16 else 256)  # the solver's chunk lengths
    assert len(xt) == 4096
    return CASES[name](q), t, np.full(n, 1e-2), r, xt


@pytest.mark.parametrize("name", sorted(LARGE))
def test_vs_oracle_65536(name):
    k, t, noise, r, xt = _large_problem(name, 1 << 16)
    mean, var = QuasisepSolver(k, t, Diagonal(noise), assume_sorted=True).predict_mean_var(r, xt)
    wmean, wvar = po.predict(k, t, noise, r, xt)
    _report(f"{name} n=2^16", mean, var, wmean, wvar)
    np.testing.assert_allclose(mean, wmean, **BAR)
    np.testing.assert_allclose(var, wvar, **BAR)


@pytest.fixture(scope="module", params=sorted(LARGE))
def million(request):
    """N = 2^20, M = 4 096: the problem, the oracle's answer (one sequential run per kernel) and the device's."""
    k, t, noise, r, xt = _large_problem(request.param, 1 << 20)
    want = po.predict(k, t, noise, r, xt)
    got = QuasisepSolver(k, t, Diagonal(noise), assume_sorted=True).predict_mean_var(r, xt)
    return request.param, (k, t, noise, r, xt), want, got


def test_vs_oracle_million(million):
    name, _, (wmean, wvar), (mean, var) = million
    _report(f"{name} n=2^20", mean, var, wmean, wvar)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
    np.testing.assert_allclose(mean, wmean, **BAR)
    np.testing.assert_allclose(var, wvar, **BAR)


def test_gp_predict_forms_no_cross_covariance(million, monkeypatch):
    """``predict(..., return_var=True)`` at N = 2^20, M = 4 096 with the dense host kernel forbidden."""
    name, (k, t, noise, r, xt), (wmean, wvar), (mean, var) = million

    def forbidden(self, X1, X2):
        raise AssertionError(f"dense host kernel matrix {np.shape(X1)} x {np.shape(X2)} requested")

    monkeypatch.setattr(q.Quasisep, "_host_matrix", forbidden)
    gp = GaussianProcess(k, t, diag=1e-2, assume_sorted=True)
    gmean, gvar = gp.predict(r, xt, return_var=True)
    assert gmean.shape == gvar.shape == (4096,)
    assert np.all(np.isfinite(gmean)) and np.all(np.isfinite(gvar))
    np.testing.assert_allclose(gmean, mean, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gvar, var + _jitter(np.float64), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gmean, wmean, **BAR)
    np.testing.assert_allclose(gvar, wvar + _jitter(np.float64), **BAR)


def test_vs_direct_solver():
    """The route it replaces: DirectSolver on the equal stationary kernel."""
    n, m = 4096, 512
    t, noise, r = _series(n, seed=31)
    xt = _test_points(t, m, seed=32)
    k = q.Matern32(1.5, sigma=1.2) * q.Cosine(3.0) + 0.5 * q.Exp(0.7)  # also lowers to the dense kernel program
    gq = GaussianProcess(k, t, noise=Diagonal(noise))
    gd = GaussianProcess(k, t, noise=Diagonal(noise), solver=DirectSolver)
    assert isinstance(gq.solver, QuasisepSolver) and isinstance(gd.solver, DirectSolver)
    assert gd.solver._prog is not None
    mq, vq = gq.predict(r, xt, return_var=True)
    md, vd = gd.predict(r, xt, return_var=True)
    _report("vs DirectSolver", mq, vq, md, vd)
    np.testing.assert_allclose(mq, md, **BAR)
    np.testing.assert_allclose(vq, vd, **BAR)


def test_other_kernel_and_no_test_points_keep_the_dense_route(monkeypatch):
    k1, k2 = q.SHO(omega=2.0, quality=3.0), q.Matern32(5.0)
    k = k1 + k2
    n = 600
    t, noise, r = _series(n, seed=41)
    xt = _test_points(t, 100, seed=42)
    K = k(t, t) + np.diag(noise)
    a = np.linalg.solve(K, r)
    gp = GaussianProcess(k, t, noise=Diagonal(noise))
    jit = _jitter(np.float64)
    calls = []
    real = QuasisepSolver._predict
    monkeypatch.setattr(QuasisepSolver, "_predict", lambda self, *args: calls.append(1) or real(self, *args))

    # one term of the sum at test points
    mean, var = gp.predict(r, xt, kernel=k1, return_var=True)
    Ks = k1(t, xt)
    np.testing.assert_allclose(mean, Ks.T @ a, **BAR)
    np.testing.assert_allclose(var, k1(xt) - np.sum(Ks * np.linalg.solve(K, Ks), axis=0) + jit, **BAR)
    # X_test = None: the data themselves, own kernel and one term
    mean, var = gp.predict(r, return_var=True)
    Kd = k(t, t)
    np.testing.assert_allclose(mean, Kd @ a, **BAR)
    np.testing.assert_allclose(var, np.diag(Kd - Kd @ np.linalg.solve(K, Kd)) + jit, **BAR)
    mean = gp.predict(r, kernel=k2)
    np.testing.assert_allclose(mean, k2(t, t) @ a, **BAR)
    assert not calls  # none of these took the device route
    # the full conditional covariance at test points: its mean is the device's, the matrix is dense
    cond = gp.condition(r, xt[:50]).gp
    assert len(calls) == 1
    Ks = k(t, xt[:50])
    want = k(xt[:50], xt[:50]) - Ks.T @ np.linalg.solve(K, Ks) + jit * np.eye(50)
    np.testing.assert_allclose(cond.covariance, want, **BAR)
    np.testing.assert_allclose(cond.loc, Ks.T @ a, **BAR)
    assert len(calls) == 1

    gp.predict(r, xt, return_var=True)
    assert len(calls) == 3  # the mean and the variance


def test_fp32():
    k = q.Matern32(2.0) + q.Cosine(3.0, sigma=0.5)
    t, noise, r = _series(3000, seed=4)
    t32, n32, r32 = t.astype(np.float32), noise.astype(np.float32), r.astype(np.float32)
    xt32 = _test_points(t32.astype(np.float64), 300, seed=5).astype(np.float32)
    s = QuasisepSolver(k, t32, Diagonal(n32))
    mean, var = s.predict_mean_var(r32, xt32)
    assert mean.dtype == var.dtype == np.float32
    f64 = lambda a: a.astype(np.float64)  # noqa: E731
    wmean, wvar = po.predict(k, f64(t32), f64(n32), f64(r32), f64(xt32))
    np.testing.assert_allclose(mean, wmean, rtol=5e-4, atol=5e-4)
    np.testing.assert_allclose(var, wvar, rtol=5e-4, atol=5e-4)
    gmean, gvar = GaussianProcess(k, t32, noise=Diagonal(n32)).predict(r32, xt32, return_var=True)
    assert gmean.dtype == gvar.dtype == np.float32
    np.testing.assert_allclose(gmean, wmean, rtol=5e-4, atol=5e-4)
    np.testing.assert_allclose(gvar, wvar + _jitter(np.float32), rtol=5e-4, atol=5e-4)


def test_failed_factor_gives_nan():
    k = q.Matern32(1.0)
    t, noise, r = _series(300, seed=6)
    noise[100:] = -5.0
    s = QuasisepSolver(k, t, Diagonal(noise))
    mean, var = s.predict_mean_var(r, np.linspace(-1, 20, 50))
    assert s.info == 101
    assert mean.shape == var.shape == (50,)
    assert np.all(np.isnan(mean)) and np.all(np.isnan(var))


def test_no_test_points():
    k = CASES["sho_under"](q)
    t, noise, r = _series(100, seed=7)
    s = QuasisepSolver(k, t, Diagonal(noise))
    mean, var = s.predict_mean_var(r, np.zeros(0))
    assert mean.shape == var.shape == (0,) and mean.dtype == np.float64
    assert s.predict_mean_var(r, np.zeros((0, 1)), return_var=False).shape == (0,)


def test_bit_identical_repeats():
    k = CASES["celerite4"](q)
    t, noise, r = _series(50000, seed=8)
    xt = _test_points(t, 1000, seed=9)
    s = QuasisepSolver(k, t, Diagonal(noise))
    a = [s.predict_mean_var(r, xt) for _ in range(2)]
    assert np.array_equal(a[0][0], a[1][0]) and np.array_equal(a[0][1], a[1][1])
    b = QuasisepSolver(k, t, Diagonal(noise)).predict_mean_var(r, xt)
    assert np.array_equal(a[0][0], b[0]) and np.array_equal(a[0][1], b[1])
