"""``QuasisepSolver.value_and_grad`` on the device: the gradient of the log-likelihood with respect to the kernel
parameters, the noise and the mean, against the sequential oracle (``_quasisep_grad_np``) and dense LAPACK.

Bars: the project's gradient bars of ``tests/test_gpu_2_grad.py`` -- kernel 2e-6, noise 1e-6, mean 1e-7, each with
atol = bar x the largest reference entry; the value at 1e-8 relative.  Against the dense gradient (dK by central
differences at two steps, combined to cancel the truncation term: the plain difference alone is 1.2e-5 off for
``cosine`` at N = 1999, see ``_quasisep_grad_np``) the kernel part is held at that reference's own floor, 1e-6 of the
largest component, as in ``tests/test_quasisep_grad_cpu.py``; the noise and mean parts keep the project's bars.  Every
test prints the figures it asserts."""
import numpy as np
import pytest

from tinygp_amd import GaussianProcess
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.noise import Diagonal
from tinygp_amd.solvers import QuasisepSolver

import _quasisep_grad_np as og
from _quasisep_cases import CASES
from _quasisep_edges import _levels

pytestmark = pytest.mark.gpu

UNDEFINED = {"sho_crit": {1}}  # the quality of a critically damped SHO: NaN by contract
THREE_LEVELS = (1 << 20) + 1
# name -> (N, lc, levels)
SHAPES = [(515, 16, 1), (131073, 64, 2), (1 << 20, 256, 2), (THREE_LEVELS, 256, 3)]


def _series(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, 0.05 * n + 1, n))
    if n > 8:
        t[n // 3] = t[n // 3 - 1]  # a repeated coordinate
    return t, rng.uniform(0.05, 0.2, n), rng.standard_normal(n)


_ORACLE = {}


def _oracle(name, n):
    """The sequential oracle of (case, N), computed once per session (minutes at N = 2^20)."""
    if (name, n) not in _ORACLE:
        t, noise, r = _series(n, seed=n)
        _ORACLE[name, n] = og.value_and_grad(CASES[name](q), t, noise, r)
    return _ORACLE[name, n]


def _compare(tag, got, want, skip=(), kernel_bar=2e-6, noise_bar=1e-6, mean_bar=1e-7):
    ll, g = got
    wll, wg, wgn, walpha = want
    gk = np.asarray(g["kernel"])
    keep = [i for i in range(len(wg)) if i not in skip]
    ks, ns, ms = np.abs(wg[keep]).max(), np.abs(wgn).max(), np.abs(walpha).max()
    print(f"{tag}: value rel {abs(ll - wll) / abs(wll):.2e}; kernel {np.abs(gk[keep] - wg[keep]).max() / ks:.2e} of max; "
          f"noise {np.abs(g['noise_diag'] - wgn).max() / ns:.2e} of max; mean {np.abs(g['mean'] - walpha).max() / ms:.2e} "
          f"of max")
    assert np.isfinite(ll) and len(gk) == len(wg)
    assert all(np.isnan(gk[i]) for i in skip)
    assert g["transform"] is None
    assert ll == pytest.approx(wll, rel=1e-8)
    np.testing.assert_allclose(gk[keep], wg[keep], rtol=kernel_bar, atol=kernel_bar * ks)
    np.testing.assert_allclose(g["noise_diag"], wgn, rtol=noise_bar, atol=noise_bar * ns)
    np.testing.assert_allclose(g["mean"], walpha, rtol=mean_bar, atol=mean_bar * ms)


def _device(name, n, **kw):
    t, noise, r = _series(n, seed=n)
    s = QuasisepSolver(CASES[name](q), t, Diagonal(noise), **kw)
    out = s.value_and_grad(r)
    assert s.info == 0
    s.close()
    return out


@pytest.mark.parametrize("n", [515, 1999])
@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_the_oracle(name, n):
    _compare(f"{name} n={n}", _device(name, n), _oracle(name, n), skip=UNDEFINED.get(name, ()))


@pytest.mark.parametrize("n", [515, 1999])
@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_dense_lapack(name, n):
    t, noise, r = _series(n, seed=n)
    skip = UNDEFINED.get(name, set())
    want = og.dense_value_and_grad(CASES[name](q), t, noise, r, skip=skip)[:4]
    _compare(f"{name} n={n} dense", _device(name, n), want, skip=skip, kernel_bar=1e-6)


@pytest.mark.parametrize("n", [1 << 16, 1 << 20])
@pytest.mark.parametrize("name", ["matern32", "celerite4"])  # J = 2 and J = 8
def test_large_matches_the_oracle(name, n):
    _compare(f"{name} n={n}", _device(name, n, assume_sorted=True), _oracle(name, n))


def test_large_directional_derivative_matches_a_central_difference():
    """N = 2^20: the derivative along the kernel gradient against a central difference of the device's own
    ``log_probability``, step 1e-3 and rtol 2e-3 as ``test_grad_at_n65536_matches_a_central_difference`` (a
    log-probability of ~1e6 carries ~1e-8 relative rounding: a smaller step would leave too few digits)."""
    n = 1 << 20
    t, noise, r = _series(n, seed=n)
    k = q.SHO(omega=2.0, quality=3.0) + q.Matern32(5.0)
    s = QuasisepSolver(k, t, Diagonal(noise), assume_sorted=True)
    ll, g = s.value_and_grad(r)
    gk = np.asarray(g["kernel"])
    assert np.isfinite(ll) and np.all(np.isfinite(gk))
    d = gk / np.linalg.norm(gk)
    theta, h = og.get_parameters(k), 1e-3
    vals = []
    for sgn in (1.0, -1.0):
        og.set_parameters(k, theta + sgn * h * d)
        s.refactor(k)
        vals.append(float(s.log_probability(r)))
    fd = (vals[0] - vals[1]) / (2 * h)
    print(f"directional derivative {np.linalg.norm(gk):.8e}, central difference {fd:.8e}")
    np.testing.assert_allclose(fd, np.linalg.norm(gk), rtol=2e-3)
    s.close()


def test_sizes_reach_the_shapes_they_name():
    assert [(n,) + _levels(n) for n, _, _ in SHAPES] == SHAPES


@pytest.mark.parametrize("n", [n for n, _, _ in SHAPES])
def test_scan_shapes(n):
    """(lc, levels) = (16, 1), (64, 2), (256, 2), (256, 3): chunk length and scan depth are functions of N."""
    lc, levels = _levels(n)
    _compare(f"matern32 n={n} lc={lc} levels={levels}", _device("matern32", n, assume_sorted=True),
             _oracle("matern32", n))


def test_direction_batches_equal_single_direction_calls():
    """``celerite4`` has 16 parameters, a batch holds 8 directions: two batches, and every derivative equals, bit for
    bit, the call that carries that direction alone."""
    n = 1999
    k = CASES["celerite4"](q)
    t, noise, r = _series(n, seed=n)
    s = QuasisepSolver(k, t, Diagonal(noise))
    ll, g = s.value_and_grad(r)
    tang = k._ssm_tangents()
    assert len(tang) == 16 == len(g["kernel"])
    for i, tg in enumerate(tang):
        v, one, gn, alpha = s._grad_call(r, tg.dleaves[None], tg.dh[None], tg.dPinf[None], vectors=False)
        assert gn is None and alpha is None
        assert v == ll and one[0] == g["kernel"][i], (i, one[0], g["kernel"][i])
    s.close()


def test_through_the_gaussian_process():
    """The documented entry point returns the solver's numbers, and ``kernel.parameters()`` lines up with
    ``grads["kernel"]``: each entry against a central difference of ``log_probability`` in that attribute (relative
    step 1e-5, rtol = atol = 1e-4 of the largest component: the cross-check bar of ``tests/test_gpu_2_grad.py``)."""
    n = 515
    t, noise, y = _series(n, seed=3)
    k = CASES["m32cos_plus_sho"](q)
    gp = GaussianProcess(k, t, diag=noise)
    assert isinstance(gp.solver, QuasisepSolver)
    ll, g = gp.log_probability_and_grad(y)
    ll2, g2 = gp.solver.value_and_grad(y)
    assert ll == ll2 and g["kernel"] == g2["kernel"]
    assert np.array_equal(g["noise_diag"], g2["noise_diag"]) and np.array_equal(g["mean"], g2["mean"])
    assert ll == gp.log_probability(y)
    pars = k.parameters()
    assert len(pars) == len(g["kernel"]) == 7
    fd = []
    for obj, attr in pars:
        v0 = getattr(obj, attr)
        step = 1e-5 * max(1.0, abs(v0))
        vals = []
        for sgn in (1.0, -1.0):
            setattr(obj, attr, v0 + sgn * step)
            vals.append(float(GaussianProcess(k, t, diag=noise).log_probability(y)))
        setattr(obj, attr, v0)
        fd.append((vals[0] - vals[1]) / (2 * step))
    scale = np.abs(fd).max()
    print("kernel gradient", g["kernel"], "central differences", fd)
    np.testing.assert_allclose(g["kernel"], fd, rtol=1e-4, atol=1e-4 * scale)


def test_direct_solver_is_untouched():
    from tinygp_amd import kernels
    from tinygp_amd.solvers import DirectSolver

    assert not hasattr(DirectSolver, "value_and_grad")
    t, noise, y = _series(200, seed=4)
    gp = GaussianProcess(1.3 * kernels.Matern32(1.5), t, diag=noise)
    ll, g = gp.log_probability_and_grad(y)
    ll2, g2 = gp.solver.log_probability_and_grad(gp._residual(y))
    assert ll == ll2 and g["kernel"] == g2["kernel"]


def test_failed_factor_is_minus_inf_and_nan():
    t, noise, r = _series(300, seed=6)
    noise[100:] = -5.0
    s = QuasisepSolver(q.Matern32(1.0), t, Diagonal(noise))
    ll, g = s.value_and_grad(r)
    assert ll == -np.inf and s.info == 101
    assert len(g["kernel"]) == 2 and np.all(np.isnan(g["kernel"]))
    assert g["noise_diag"].shape == g["mean"].shape == (300,)
    assert np.all(np.isnan(g["noise_diag"])) and np.all(np.isnan(g["mean"]))
    s.close()


def test_fp32():
    k = q.Matern32(2.0) + q.Cosine(3.0, sigma=0.5)
    t, noise, r = _series(3000, seed=4)
    t32, n32, r32 = t.astype(np.float32), noise.astype(np.float32), r.astype(np.float32)
    ll, g = GaussianProcess(k, t32, noise=Diagonal(n32)).log_probability_and_grad(r32)
    assert ll.dtype == np.float32 and g["noise_diag"].dtype == np.float32 and g["mean"].dtype == np.float32
    wll, wg, wgn, walpha = og.value_and_grad(k, t32.astype(np.float64), n32.astype(np.float64), r32.astype(np.float64))
    assert float(ll) == pytest.approx(wll, rel=5e-4)
    np.testing.assert_allclose(g["kernel"], wg, rtol=5e-4, atol=5e-4 * np.abs(wg).max())
    np.testing.assert_allclose(g["noise_diag"], wgn, rtol=5e-4, atol=5e-4 * np.abs(wgn).max())
    np.testing.assert_allclose(g["mean"], walpha, rtol=5e-4, atol=5e-4 * np.abs(walpha).max())


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("name", ["exp", "m32cos_plus_sho"])
def test_one_and_two_points(name, n):
    k = CASES[name](q)
    t, noise, r = np.array([0.3, 0.9])[:n], np.array([0.1, 0.15])[:n], np.array([0.7, -0.4])[:n]
    s = QuasisepSolver(k, t, Diagonal(noise))
    _compare(f"{name} n={n}", s.value_and_grad(r), og.value_and_grad(k, t, noise, r))
    s.close()


def test_bit_identical_repeats():
    k = CASES["celerite4"](q)
    rng = np.random.default_rng(8)
    n = 50000
    dt = np.where(rng.uniform(size=n) < 0.5, rng.exponential(0.001, n), rng.exponential(0.3, n))
    t, noise, r = np.cumsum(dt), rng.uniform(0.05, 0.2, n), rng.standard_normal(n)
    s = QuasisepSolver(k, t, Diagonal(noise))
    runs = [s.value_and_grad(r) for _ in range(3)]
    for ll, g in runs[1:]:
        assert ll == runs[0][0] and g["kernel"] == runs[0][1]["kernel"]
        assert np.array_equal(g["noise_diag"], runs[0][1]["noise_diag"]) and np.array_equal(g["mean"], runs[0][1]["mean"])
    assert np.all(np.isfinite(runs[0][1]["kernel"]))
    s.close()


def test_refactored_handle_of_another_state_dimension():
    """One handle: J = 8, then J = 2 through ``refactor``; the second gradient equals a fresh solver's, bit for bit."""
    t, noise, r = _series(1999, seed=1999)
    k8, k2 = CASES["celerite4"](q), CASES["matern32"](q)
    s = QuasisepSolver(k8, t, Diagonal(noise))
    first = s.value_and_grad(r)
    assert len(first[1]["kernel"]) == 16
    assert s.refactor(k2) == 0
    ll, g = s.value_and_grad(r)
    fresh = QuasisepSolver(k2, t, Diagonal(noise))
    wll, wg = fresh.value_and_grad(r)
    assert ll == wll and g["kernel"] == wg["kernel"] and len(g["kernel"]) == 2
    assert np.array_equal(g["noise_diag"], wg["noise_diag"]) and np.array_equal(g["mean"], wg["mean"])
    _compare("matern32 after celerite4", (ll, g), _oracle("matern32", 1999))
    s.close()
    fresh.close()
