"""The extended-precision sequential oracle (``_quasisep_np`` with ``dtype=``) against 50-digit mpmath and dense
LAPACK, and the over-damped SHO transition at large arguments.  No GPU, nothing loads the library."""
import os

import numpy as np
import pytest

from tinygp_amd.kernels import quasisep as q

import _quasisep_np as o
import _quasisep_predict_np as po
from _quasisep_cases import CASES, data

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_quasisep.npz"))


def _rel(a, ref):
    """max |a - ref| / max |ref| with the difference formed in mpmath."""
    ref = o.cast(ref, o.MP)
    d = np.abs(o.cast(a, o.MP) - ref)
    return float(np.max(d) / np.max(np.abs(ref)))


def test_extended_dtype_is_wider_than_double():
    """Where np.longdouble is the 80-bit format the tests use it; elsewhere they run on mpmath."""
    assert o.EXT is (np.longdouble if np.finfo(np.longdouble).eps < 1e-18 else o.MP)


@pytest.mark.parametrize("name", sorted(CASES))
def test_extended_oracle_matches_mpmath(name):
    """N = 200, every case.  Bar 1e-15 of each quantity's largest entry: three decades above the extended format's
    own rounding (eps = 1.1e-19, a few hundred steps, moderate conditioning at noise >= 0.05) and below anything a
    float64 computation could meet (eps = 2.2e-16 per operation)."""
    k = CASES[name](q)
    t, noise, r = data(n=200)
    y = np.stack([r, np.random.default_rng(1).standard_normal(len(t))], axis=1)
    Fe, Fm = o.factor(k, t, noise, o.EXT), o.factor(k, t, noise, o.MP)
    for e, m in zip(Fe, Fm):
        assert _rel(e, m) < 1e-15
    for op in (o.solve_lower, o.solve_upper, o.dot_lower):
        assert _rel(op(Fe, y), op(Fm, y)) < 1e-15
    assert _rel(o.log_probability(k, t, noise, r, o.EXT), o.log_probability(k, t, noise, r, o.MP)) < 1e-15
    xt = np.concatenate([np.linspace(-1.0, 13.0, 15), t[[0, 6, 7, 199]]])
    for e, m in zip(po.predict(k, t, noise, r, xt, F=Fe, dtype=o.EXT), po.predict(k, t, noise, r, xt, F=Fm, dtype=o.MP)):
        assert _rel(e, m) < 1e-15
    # and the float64 oracle is a float64 computation of the same thing
    assert o.log_probability(k, t, noise, r) == pytest.approx(float(o.log_probability(k, t, noise, r, o.EXT)), rel=1e-12)


@pytest.mark.parametrize("name", sorted(CASES))
def test_extended_oracle_matches_dense_lapack(name):
    """The bars of ``test_quasisep_cpu.test_oracle_matches_dense_lapack``, on the same well-conditioned input."""
    k, t, noise, r = CASES[name](q), GOLDEN["t"], GOLDEN["noise"], GOLDEN["r"]
    assert float(o.log_probability(k, t, noise, r, o.EXT)) == pytest.approx(float(GOLDEN[f"{name}__logp"]), rel=1e-10)
    F = o.factor(k, t, noise, o.EXT)
    L = np.linalg.cholesky(GOLDEN[f"{name}__K"] + np.diag(noise))
    np.testing.assert_allclose(o.to_f64(o.dense_factor(F)), L, atol=1e-11 * np.abs(L).max())
    y = np.stack([r, r ** 2], axis=1)
    np.testing.assert_allclose(o.to_f64(o.solve_lower(F, y)), np.linalg.solve(L, y), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(o.to_f64(o.solve_upper(F, y)), np.linalg.solve(L.T, y), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(o.to_f64(o.dot_lower(F, y)), L @ y, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("arg", [1.0, 100.0, 700.0, 720.0, 5000.0])
@pytest.mark.parametrize("quality", [0.3, 0.05])
def test_overdamped_sho_at_large_arguments(quality, arg):
    """exp(-a) cosh(arg) is 0 * inf beyond arg ~ 710; the transition and the kernel value stay finite and agree with
    mpmath's textbook form.  rtol 1e-12: the exponents reach a few thousand and carry a relative error of a few eps
    each, so the values carry up to ~1e-12; atol 1e-300 lets a value below the double range be 0."""
    k = q.SHO(omega=1.5, quality=quality, sigma=1.3)
    f = np.sqrt(1 - 4 * quality ** 2)
    dt = np.array([arg * 2 * quality / (f * 1.5)])
    assert 0.5 * f * 1.5 * dt[0] / quality == pytest.approx(arg, rel=1e-14)
    A = k._phi(dt)
    assert np.all(np.isfinite(A))
    s = k._ssm()
    Am = o.model_transitions(s, dt, o.MP)
    np.testing.assert_allclose(A, o.to_f64(Am), rtol=1e-12, atol=1e-300)
    want = o.cast(s.h, o.MP) @ Am[0] @ o.cast(s.Pinf, o.MP) @ o.cast(s.h, o.MP)
    for got in (k.evaluate(0.0, dt[0]), k(np.zeros(1), dt)[0, 0], k(dt, np.zeros(1))[0, 0]):
        assert np.isfinite(got)
        np.testing.assert_allclose(got, float(want), rtol=1e-12, atol=1e-300)
    if o.EXTENDED:  # the helper's own stable form, against its textbook form
        np.testing.assert_allclose(o.to_f64(o.model_transitions(s, dt, np.longdouble)), o.to_f64(Am), rtol=1e-15,
                                   atol=1e-300)


def test_overdamped_sho_long_series_is_finite():
    """The suite's ``sho_over`` over a span of 2 000 time units with one gap of 400: k(t, t) and the oracle are finite."""
    k = CASES["sho_over"](q)
    rng = np.random.default_rng(0)
    t = np.sort(np.concatenate([rng.uniform(0, 800, 150), rng.uniform(1200, 2000, 150)]))
    noise, r = rng.uniform(0.05, 0.2, 300), rng.standard_normal(300)
    K = k(t, t)
    assert np.all(np.isfinite(K))
    L = np.linalg.cholesky(K + np.diag(noise))
    z = np.linalg.solve(L, r)
    want = -0.5 * z @ z - np.sum(np.log(np.diag(L))) - 150 * np.log(2 * np.pi)
    assert o.log_probability(k, t, noise, r) == pytest.approx(want, rel=1e-10)
    assert float(o.log_probability(k, t, noise, r, o.EXT)) == pytest.approx(want, rel=1e-10)
