"""The gradient of the quasiseparable log-likelihood on the host: parameters, the tangents of the state-space model,
the transitions' tangents, and the sequential oracle (``_quasisep_grad_np``) against dense LAPACK.  No GPU, nothing
loads the library.

Bars.  Oracle against the dense gradient: 1e-6 of the largest component, the finite-difference floor of dK argued at
the top of ``tests/test_gpu_2_grad.py``; the noise and mean gradients, which difference nothing, 1e-10.  Analytic
tangents against central differences with relative step 1e-6: truncation ~ step^2 and round-off ~ eps / step ~ 2e-10
of the quantity's size, held at 1e-8 of the largest entry."""
import numpy as np
import pytest

from tinygp_amd.kernels import quasisep as q

import _quasisep_grad_np as og
import _quasisep_np as o
from _quasisep_cases import CASES, data

PARAMS = {
    "exp": ["scale", "sigma"], "matern32": ["scale", "sigma"], "matern52": ["scale", "sigma"],
    "cosine": ["scale", "sigma"], "celerite": ["a", "b", "c", "d"], "sho_under": ["omega", "quality", "sigma"],
    "sho_crit": ["omega", "quality", "sigma"], "sho_over": ["omega", "quality", "sigma"],
    "sum_sho_m32": ["omega", "quality", "sigma", "scale", "sigma"],
    "prod_m32_cos": ["scale", "sigma", "scale", "sigma"],
    "scale_m52": ["scale", "sigma", "scale"],
    "m32cos_plus_sho": ["scale", "sigma", "scale", "sigma", "omega", "quality", "sigma"],
    "m52_times_sho": ["scale", "sigma", "omega", "quality", "sigma"],
    "celerite4": ["a", "b", "c", "d"] * 4,
    "scaled_sum": ["scale", "sigma", "scale", "sigma", "scale"],
}
UNDEFINED = {"sho_crit": {1}}  # parameters without a derivative: the quality of a critically damped SHO


def _series(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0, 0.05 * n + 1, n))
    t[n // 3] = t[n // 3 - 1]  # a repeated coordinate
    return t, rng.uniform(0.05, 0.2, n), rng.standard_normal(n)


@pytest.mark.parametrize("name", sorted(CASES))
def test_parameters_order_and_length(name):
    k = CASES[name](q)
    pars = k.parameters()
    assert [attr for _, attr in pars] == PARAMS[name]
    assert all(np.ndim(getattr(obj, attr)) == 0 for obj, attr in pars)
    assert len(k._ssm_tangents()) == len(pars)


def test_parameters_are_depth_first_objects():
    a, b = q.Exp(0.5), q.Matern32(2.0, sigma=0.5)
    k = 1.7 * (a + b)
    assert k.parameters() == [(a, "scale"), (a, "sigma"), (b, "scale"), (b, "sigma"), (k, "scale")]


def _ssm_fd(k, i):
    theta0 = og.get_parameters(k)
    step = 1e-6 * max(1.0, abs(theta0[i]))
    out = []
    for sgn in (1.0, -1.0):
        th = theta0.copy()
        th[i] += sgn * step
        og.set_parameters(k, th)
        out.append(k._ssm())
    og.set_parameters(k, theta0)
    return out[0], out[1], step


@pytest.mark.parametrize("name", sorted(CASES))
def test_ssm_tangents_match_central_differences(name):
    """Every class and every SHO regime: the leaf table, h and P of ``_ssm()`` differenced in each parameter."""
    k = CASES[name](q)
    tang = k._ssm_tangents()
    lags = np.array([0.0, 1e-3, 0.3, 1.7, 9.0])
    for i, tg in enumerate(tang):
        if i in UNDEFINED.get(name, ()):
            assert np.all(np.isnan(tg.dleaves[0, :3]))
            continue
        sp, sm, step = _ssm_fd(k, i)
        assert np.array_equal(sp.leaves[:, 0], sm.leaves[:, 0])  # the same regimes on both sides
        for got, hi, lo in ((tg.dleaves, sp.leaves[:, 1:], sm.leaves[:, 1:]), (tg.dh, sp.h, sm.h),
                            (tg.dPinf, sp.Pinf, sm.Pinf)):
            want = (hi - lo) / (2 * step)
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-8 * max(1.0, np.abs(want).max()))
        # and the whole model's transition tangent, product rule over the leaves included
        th0 = og.get_parameters(k)
        mats = []
        for sgn in (1.0, -1.0):
            th = th0.copy()
            th[i] += sgn * step
            og.set_parameters(k, th)
            mats.append(k._phi(lags))
        og.set_parameters(k, th0)
        want = (mats[0] - mats[1]) / (2 * step)
        got = q.model_dphi(k._ssm(), tg.dleaves, lags)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-8 * max(1.0, np.abs(want).max()))
        assert np.all(got[0] == 0.0)  # every term carries a factor dt


@pytest.mark.parametrize("name", sorted(CASES))
def test_leaf_phi_twin_matches_the_kernel(name):
    k = CASES[name](q)
    s = k._ssm()
    lags = np.array([0.0, 0.2, 3.0])
    if len(s.leaves) == 1:
        np.testing.assert_allclose(q.leaf_phi(s.leaves[0, 0], s.leaves[0, 1:], lags), k._phi(lags), rtol=1e-14,
                                   atol=1e-300)
    np.testing.assert_allclose(o.to_f64(o.model_transitions(s, lags, np.float64)), k._phi(lags), rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("kind,p", [(q.QS_EXP, [0.8]), (q.QS_M32, [1.3]), (q.QS_M52, [0.9]), (q.QS_COS, [2.1]),
                                    (q.QS_CELERITE, [0.5, 1.5]), (q.QS_SHO_UNDER, [2.0, 3.0, np.sqrt(35.0)]),
                                    (q.QS_SHO_CRIT, [1.5]), (q.QS_SHO_OVER, [1.5, 0.3, 0.8])])
def test_leaf_dphi_matches_central_differences(kind, p):
    """Each stored parameter on its own (SHO's f as an independent slot, as the device's leaf_dphi takes it).  The
    over-damped transition is written with 1 - f^2 = 4 Q^2 built in, so it is a function of (omega, Q) only: there
    the directions are omega and Q with f following Q, df = -4 Q / f dQ."""
    p = np.array(list(p) + [0.0] * (4 - len(p)))
    lags = np.array([0.0, 1e-3, 0.4, 2.5, 11.0])
    nstored = {q.QS_CELERITE: 2, q.QS_SHO_UNDER: 3, q.QS_SHO_OVER: 3}.get(kind, 1)
    dirs = np.eye(4)[:nstored]
    if kind == q.QS_SHO_OVER:
        assert p[2] == np.sqrt(1 - 4 * p[1] ** 2)
        dirs = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, -4 * p[1] / p[2], 0.0]])
    for dp in dirs:
        step = 1e-6 * max(1.0, np.abs(p[dp != 0]).max())

        def at(sgn):
            x = p + sgn * step * dp
            if kind == q.QS_SHO_OVER:
                x[2] = np.sqrt(1 - 4 * x[1] ** 2)
            return q.leaf_phi(kind, x, lags)

        want = (at(1.0) - at(-1.0)) / (2 * step)
        got = q.leaf_dphi(kind, p, dp, lags)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-8 * max(1.0, np.abs(want).max()))


def test_critically_damped_sho_has_nan_for_quality_only():
    k = q.SHO(omega=1.5, quality=0.5, sigma=0.8)
    tang = k._ssm_tangents()
    assert [bool(np.any(np.isnan(np.concatenate([x.dleaves.ravel(), x.dh, x.dPinf.ravel()])))) for x in tang] == \
        [False, True, False]
    t, noise, r = data(64)
    _, g, gn, alpha = og.value_and_grad(k, t, noise, r)
    assert np.isfinite(g[0]) and np.isnan(g[1]) and np.isfinite(g[2])
    assert np.all(np.isfinite(gn)) and np.all(np.isfinite(alpha))


@pytest.mark.parametrize("arg", [1.0, 100.0, 700.0, 720.0, 5000.0])
def test_overdamped_sho_tangent_at_large_arguments(arg):
    """The transition's derivative with respect to omega and quality at b = arg, against central differences of the
    textbook transition in 50-digit mpmath (step 1e-20: truncation 1e-40, round-off 1e-30).  Finite everywhere.  Bar
    1e-11 of each entry (absolute: of the largest entry): the exponents reach a few thousand and carry a few eps of
    relative error each, ~1e-12 as for the transition itself (``test_quasisep_oracle_cpu``), and the exponents'
    tangent da - db loses a further 1 / (1 - f) = 5 at Q = 0.3."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    quality, omega = 0.3, 1.5
    k = q.SHO(omega=omega, quality=quality, sigma=1.3)
    f = np.sqrt(1 - 4 * quality ** 2)
    dt = np.array([arg * 2 * quality / (f * omega)])
    s = k._ssm()
    assert int(s.leaves[0, 0]) == q.QS_SHO_OVER
    hstep = mp.mpf(10) ** -20
    for i, tg in enumerate(k._ssm_tangents()[:2]):
        got = q.model_dphi(s, tg.dleaves, dt)[0]
        assert np.all(np.isfinite(got))
        mats = []
        for sgn in (1, -1):
            row = o.cast(s.leaves[0, 1:], o.MP)
            row[i] = row[i] + sgn * hstep
            mats.append(np.array(o._leaf(q.QS_SHO_OVER, row, o.cast(dt, o.MP), o.MP), dtype=object)[:, :, 0])
        want = o.to_f64((mats[0] - mats[1]) / (2 * hstep))
        np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-11 * np.abs(want).max() + 1e-300)


def test_closed_loop_form_of_the_factor_tangent():
    """dD_n = M_n dD_{n-1} M_n^T + G_n with the filter's closed-loop map: what makes the tangent a scan."""
    k = CASES["matern32"](q)
    t, noise, r = data(60)
    gaps = []
    og.value_and_grad(k, t, noise, r, closed_loop_check=gaps)
    assert len(gaps) == 60 and max(gaps) < 1e-12


@pytest.mark.parametrize("n", [64, 500])
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_matches_dense_lapack(name, n):
    k = CASES[name](q)
    t, noise, r = data(64) if n == 64 else _series(n, seed=n)
    skip = UNDEFINED.get(name, set())
    lp, g, gn, alpha = og.value_and_grad(k, t, noise, r, block=128)
    wlp, wg, wgn, walpha, Kinv = og.dense_value_and_grad(k, t, noise, r, skip=skip)
    keep = [i for i in range(len(g)) if i not in skip]
    assert all(np.isnan(g[i]) for i in skip)
    scale = np.abs(wg[keep]).max()
    print(f"{name} n={n}: kernel {np.abs(g[keep] - wg[keep]).max() / scale:.2e} of max |g|, noise "
          f"{np.abs(gn - wgn).max():.2e}, mean {np.abs(alpha - walpha).max():.2e}")
    assert lp == pytest.approx(wlp, rel=1e-10)
    assert lp == pytest.approx(o.log_probability(k, t, noise, r), rel=1e-12)
    np.testing.assert_allclose(g[keep], wg[keep], rtol=0, atol=1e-6 * scale)
    np.testing.assert_allclose(gn, wgn, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(alpha, walpha, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(0.5 * (alpha ** 2 - np.diag(Kinv)), gn, rtol=1e-10, atol=1e-10)
