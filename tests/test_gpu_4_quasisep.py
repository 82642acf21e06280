"""QuasisepSolver on the device: likelihoods, solves, L @ z, conditioning, sampling, failure and determinism."""
import numpy as np
import pytest

from tinygp_amd import GaussianProcess, kernels
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.noise import Diagonal
from tinygp_amd.solvers import DirectSolver, QuasisepSolver

import _quasisep_np as o
from _quasisep_cases import CASES

pytestmark = pytest.mark.gpu

# straddle the chunk length (16 steps below 65 536 points), the scan fan-in (64 chunks) and a second scan level
SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 1000, 1023, 1024, 1025, 4097, 16 * 64 * 64 + 1]


def _dense_logp(K, noise, r):
    L = np.linalg.cholesky(K + np.diag(noise))
    z = np.linalg.solve(L, r)
    return -0.5 * z @ z - np.sum(np.log(np.diag(L))) - 0.5 * len(r) * np.log(2 * np.pi)


def _series(n, seed=0, clustered=False):
    rng = np.random.default_rng(seed)
    if clustered:
        dt = np.where(rng.uniform(size=n) < 0.5, rng.exponential(0.001, n), rng.exponential(0.3, n))
        dt[rng.uniform(size=n) < 0.05] = 0.0
        t = np.cumsum(dt)
    else:
        t = np.sort(rng.uniform(0, 0.05 * n + 1, n))
    return t, rng.uniform(0.05, 0.2, n), rng.standard_normal(n)


@pytest.mark.parametrize("name", sorted(CASES))
def test_logp_matches_golden(name):
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_quasisep.npz"))
    k = CASES[name](q)
    s = QuasisepSolver(k, g["t"], Diagonal(g["noise"]))
    assert s.log_probability(g["r"]) == pytest.approx(float(g[f"{name}__logp"]), rel=1e-8)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["matern32", "m32cos_plus_sho", "celerite4", "sho_crit"])
def test_logp_vs_dense_or_oracle(name, n):
    k = CASES[name](q)
    t, noise, r = _series(n, seed=n)
    got = GaussianProcess(k, t, noise=Diagonal(noise)).log_probability(r)
    want = _dense_logp(k(t, t), noise, r) if n <= 4097 else o.log_probability(k, t, noise, r)
    assert got == pytest.approx(want, rel=1e-8)


@pytest.mark.parametrize("name", ["matern52", "m52_times_sho", "celerite4"])
def test_large_clustered_vs_oracle(name):
    k = CASES[name](q)
    t, noise, r = _series(1 << 17, seed=3, clustered=True)
    got = GaussianProcess(k, t, noise=Diagonal(noise)).log_probability(r)
    assert got == pytest.approx(o.log_probability(k, t, noise, r), rel=1e-8)


def test_tiny_noise():
    k = q.SHO(omega=2.0, quality=3.0) + q.Matern32(5.0)
    t, _, r = _series(500, seed=5)
    noise = np.full(500, 1e-6 * (1.0 + 1.0))
    got = GaussianProcess(k, t, noise=Diagonal(noise)).log_probability(r)
    assert got == pytest.approx(_dense_logp(k(t, t), noise, r), rel=1e-8)


@pytest.mark.parametrize("R", [1, 7, 64])
def test_solves_and_dot(R):
    k = CASES["m32cos_plus_sho"](q)
    t, noise, _ = _series(700, seed=R)
    y = np.random.default_rng(R).standard_normal((700, R))
    s = QuasisepSolver(k, t, Diagonal(noise))
    L = np.linalg.cholesky(k(t, t) + np.diag(noise))
    np.testing.assert_allclose(s.solve_triangular(y), np.linalg.solve(L, y), rtol=5e-7, atol=5e-7)
    np.testing.assert_allclose(s.solve_triangular(y, transpose=True), np.linalg.solve(L.T, y), rtol=5e-7, atol=5e-7)
    np.testing.assert_allclose(s.dot_triangular(y), L @ y, rtol=5e-7, atol=5e-7)
    np.testing.assert_allclose(s.solve_triangular(y[:, 0]), np.linalg.solve(L, y[:, 0]), rtol=5e-7, atol=5e-7)
    assert s.normalization() == pytest.approx(np.sum(np.log(np.diag(L))) + 350 * np.log(2 * np.pi), rel=1e-10)


def test_condition_and_predict_vs_direct():
    k = q.SHO(omega=2.0, quality=3.0) + q.Matern32(5.0)
    t, noise, r = _series(1500, seed=9)
    xt = np.linspace(t[0] - 1, t[-1] + 1, 200)
    gq = GaussianProcess(k, t, noise=Diagonal(noise))
    gd = GaussianProcess(k, t, noise=Diagonal(noise), solver=DirectSolver)
    assert isinstance(gq.solver, QuasisepSolver) and isinstance(gd.solver, DirectSolver)
    mq, vq = gq.predict(r, xt, return_var=True)
    md, vd = gd.predict(r, xt, return_var=True)
    np.testing.assert_allclose(mq, md, rtol=5e-7, atol=5e-7)
    np.testing.assert_allclose(vq, vd, rtol=5e-7, atol=5e-7)
    cq, cd = gq.condition(r, xt), gd.condition(r, xt)
    assert cq.log_probability == pytest.approx(cd.log_probability, rel=1e-8)
    np.testing.assert_allclose(cq.gp.covariance, cd.gp.covariance, rtol=5e-7, atol=5e-7)
    assert gq.log_probability(r) == pytest.approx(gd.log_probability(r), rel=1e-8)


def test_device_dense_lowering_agrees():
    """Exp / Matern / Cosine trees also run on the dense device path; it agrees with the quasiseparable one."""
    k = q.Matern32(1.5) * q.Cosine(3.0) + 0.5 * q.Exp(0.7)
    t, noise, r = _series(2000, seed=2)
    gd = GaussianProcess(k, t, noise=Diagonal(noise), solver=DirectSolver)
    assert gd.solver._prog is not None
    assert GaussianProcess(k, t, noise=Diagonal(noise)).log_probability(r) == pytest.approx(gd.log_probability(r),
                                                                                           rel=1e-8)


def test_sample_moments():
    k = q.Matern32(1.0, sigma=1.3) + q.SHO(omega=3.0, quality=2.0)
    t = np.linspace(0, 5, 40)
    gp = GaussianProcess(k, t, diag=0.1)
    y = gp.sample(0, shape=(50000,))
    assert y.shape == (50000, 40)
    np.testing.assert_allclose(np.mean(y, axis=0), 0.0, atol=0.05)
    np.testing.assert_allclose(np.cov(y, rowvar=False), gp.covariance, atol=0.1)  # ~5 sigma at var 2.8


def test_fp32():
    k = q.Matern32(2.0) + q.Cosine(3.0, sigma=0.5)
    t, noise, r = _series(3000, seed=4)
    t32, n32, r32 = t.astype(np.float32), noise.astype(np.float32), r.astype(np.float32)
    gp = GaussianProcess(k, t32, noise=Diagonal(n32))
    v = gp.log_probability(r32)
    assert v.dtype == np.float32
    want = o.log_probability(k, t32.astype(np.float64), n32.astype(np.float64), r32.astype(np.float64))
    assert float(v) == pytest.approx(want, rel=5e-4)
    z = gp.solver.solve_triangular(r32)
    assert z.dtype == np.float32
    F = o.factor(k, t32.astype(np.float64), n32.astype(np.float64))
    np.testing.assert_allclose(z, o.solve_lower(F, r32.astype(np.float64)), rtol=5e-4, atol=5e-4)


def test_negative_noise_is_minus_inf_not_raise():
    k = q.Matern32(1.0)
    t, noise, r = _series(300, seed=6)
    noise[100:] = -5.0
    s = QuasisepSolver(k, t, Diagonal(noise))
    assert s.log_probability(r) == -np.inf
    assert s.info == 101
    assert np.all(np.isnan(s.solve_triangular(r)))
    assert np.isnan(s.normalization())


def test_bit_identical_repeats():
    k = CASES["celerite4"](q)
    t, noise, r = _series(50000, seed=8, clustered=True)
    s = QuasisepSolver(k, t, Diagonal(noise))
    a = [s.log_probability(r) for _ in range(3)]
    z = [s.solve_triangular(np.stack([r, 2 * r], 1), transpose=True) for _ in range(2)]
    assert a[0] == a[1] == a[2]
    assert np.array_equal(z[0], z[1])


def test_gradient_not_yet():
    s = QuasisepSolver(q.Exp(1.0), np.arange(5.0), Diagonal(np.ones(5)))
    with pytest.raises(NotImplementedError, match="not yet"):
        s.log_probability_and_grad(np.ones(5))


def test_user_level_million_points():
    n = 1_000_000
    t, noise, r = _series(n, seed=12)
    k = q.SHO(omega=2.0, quality=3.0) + q.Matern32(5.0)
    gp = GaussianProcess(k, t, diag=1e-3)
    got = gp.log_probability(r)
    assert np.isfinite(got)
    assert got == pytest.approx(o.log_probability(k, t, np.full(n, 1e-3), r), rel=1e-8)


def test_large_j8_finite_and_prefix_agrees():
    """N = 2^22, J = 8: finite, and c_n on the first steps equal a sequential fp64 run over that prefix."""
    n = 1 << 22
    t, noise, r = _series(n, seed=13)
    k = CASES["celerite4"](q)
    s = QuasisepSolver(k, t, Diagonal(noise), assume_sorted=True)
    v = s.log_probability(r)
    assert np.isfinite(v) and s.info == 0
    c, w = s.factor_data()
    m = 20000
    F = o.factor(k, t[:m], noise[:m])
    np.testing.assert_allclose(c[:m], F[2], rtol=1e-9)
    np.testing.assert_allclose(w[:m], F[3], rtol=1e-8, atol=1e-12)
    assert np.all(np.isfinite(c)) and np.all(c > 0)
