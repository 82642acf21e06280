"""Quasiseparable kernels and the NumPy factor oracle, without a GPU (no device call, nothing loads the library)."""
import os

import numpy as np
import pytest

from tinygp_amd import GaussianProcess, _device, kernels
from tinygp_amd.kernels import base
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.noise import Dense, Diagonal
from tinygp_amd.solvers import DirectSolver, QuasisepSolver

import _quasisep_np as o
from _quasisep_cases import CASES

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_quasisep.npz"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_values_match_reference(name):
    k, t = CASES[name](q), GOLDEN["t"]
    K = GOLDEN[f"{name}__K"]
    np.testing.assert_allclose(k(t, t), K, rtol=1e-13, atol=1e-13 * np.abs(K).max())
    np.testing.assert_allclose(k(t), GOLDEN[f"{name}__diag"], rtol=1e-13)
    np.testing.assert_allclose(k(t[:, None], t[:5, None]), K[:, :5], rtol=1e-13, atol=1e-13 * np.abs(K).max())
    assert k.evaluate(t[3], t[9]) == pytest.approx(K[3, 9], rel=1e-13)


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_matches_dense_lapack(name):
    k, t, noise, r = CASES[name](q), GOLDEN["t"], GOLDEN["noise"], GOLDEN["r"]
    assert o.log_probability(k, t, noise, r) == pytest.approx(float(GOLDEN[f"{name}__logp"]), rel=1e-10)
    F = o.factor(k, t, noise)
    L = np.linalg.cholesky(GOLDEN[f"{name}__K"] + np.diag(noise))
    scale = np.abs(L).max()
    np.testing.assert_allclose(o.dense_factor(F), L, atol=1e-11 * scale)
    y = np.stack([r, r ** 2], axis=1)
    np.testing.assert_allclose(o.solve_lower(F, y), np.linalg.solve(L, y), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(o.solve_upper(F, y), np.linalg.solve(L.T, y), rtol=1e-9, atol=1e-9)


def test_transitions_are_matrix_exponentials():
    from scipy.linalg import expm

    for k in (q.Exp(1.3), q.Matern32(0.8), q.Matern52(1.1), q.Cosine(2.0), q.Celerite(1.0, 0.2, 0.5, 1.5),
              q.SHO(2.0, 3.0), q.SHO(1.5, 0.5), q.SHO(1.5, 0.3)):
        for dt in (0.0, 0.37, 2.5):
            np.testing.assert_allclose(k._phi(np.array(dt)), expm(k.design_matrix() * dt), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(k.transition_matrix(0.0, 0.37), k._phi(np.array(0.37)).T)


def test_lower_ssm_tables():
    s = q.Matern32(2.0, sigma=1.5)._lower_ssm()
    assert s.J == 2 and s.leaves.shape == (1, 5) and s.leaves[0, 0] == q.QS_M32
    np.testing.assert_allclose(s.leaves[0, 1], np.sqrt(3) / 2.0)
    np.testing.assert_allclose(s.h, [1.5, 0.0])
    np.testing.assert_allclose(s.Pinf, np.diag([1.0, 0.75]))
    a, b = q.Matern32(2.0), q.Cosine(3.0)
    p = (a * b)._lower_ssm()
    np.testing.assert_allclose(p.h, np.kron(a._ssm().h, b._ssm().h))
    np.testing.assert_allclose(p.Pinf, np.kron(a._ssm().Pinf, b._ssm().Pinf))
    np.testing.assert_array_equal(p.state_map, [[0, 0], [0, 1], [1, 0], [1, 1]])
    sm = (a + b + q.Exp(1.0))._lower_ssm()
    assert sm.J == 5
    np.testing.assert_array_equal(sm.state_map, [[0, -1, -1], [1, -1, -1], [-1, 0, -1], [-1, 1, -1], [-1, -1, 0]])
    np.testing.assert_allclose(sm.Pinf[:2, 2:], 0.0)
    np.testing.assert_allclose((3.0 * a)._lower_ssm().Pinf, 3.0 * a._ssm().Pinf)
    assert CASES["m52_times_sho"](q)._lower_ssm().J == 6
    assert CASES["celerite4"](q)._lower_ssm().J == 8
    sho = [q.SHO(1.0, Q)._lower_ssm().leaves[0, 0] for Q in (3.0, 0.5, 0.3)]
    assert sho == [q.QS_SHO_UNDER, q.QS_SHO_CRIT, q.QS_SHO_OVER]


def test_state_dimension_limit():
    k = q.Matern52(1.0) * q.Matern52(2.0)  # J = 9
    with pytest.raises(_device.DeviceLimit, match="J <= 8"):
        k._lower_ssm()
    with pytest.raises(_device.DeviceLimit):
        QuasisepSolver(k, np.arange(4.0), Diagonal(np.ones(4)))


def test_algebra():
    a, b = q.Matern32(1.0), q.SHO(2.0, 3.0)
    assert isinstance(a + b, q.Sum) and isinstance(a * b, q.Product)
    assert isinstance(2.0 * a, q.Scale) and isinstance(a * 2.0, q.Scale)
    assert isinstance(a + kernels.ExpSquared(1.0), base.Sum) and not isinstance(a + kernels.ExpSquared(1.0), q.Quasisep)
    assert isinstance(a * kernels.ExpSquared(1.0), base.Product)
    assert sum([a, b]) is not None
    t = np.linspace(0, 3, 7)
    np.testing.assert_allclose(base.host_matrix(a + kernels.Constant(0.5), t, t), a(t, t) + 0.5)


def test_dense_lowering_to_stationary_program():
    for cls, st in ((q.Exp, kernels.Exp), (q.Matern32, kernels.Matern32), (q.Matern52, kernels.Matern52),
                    (q.Cosine, kernels.Cosine)):
        assert cls(1.7, sigma=0.4).program() == (kernels.Constant(0.16) * st(1.7)).program()[1:2] + [
            (base.K_CONST, 0, 0.4 ** 2, 0.0), (base.K_MUL, 0, 0.0, 0.0)]
    prog, X = (q.Matern32(1.0) * q.Cosine(2.0) + 2.0 * q.Exp(1.0))._lower(np.arange(3.0))
    assert prog[-1][0] == base.K_ADD and X.shape == (3,)
    for k in (q.Celerite(1.0, 0.2, 0.5, 1.5), q.SHO(2.0, 3.0), q.SHO(2.0, 3.0) + q.Matern32(1.0)):
        with pytest.raises(NotImplementedError):
            k._lower(np.arange(3.0))


def test_inputs_and_matmul():
    k = q.Matern32(1.0) + q.SHO(2.0, 3.0)
    t = np.linspace(0, 4, 30)
    y = np.random.default_rng(0).standard_normal((30, 2))
    np.testing.assert_allclose(k.matmul(t[:10], t, y), k(t[:10], t) @ y, rtol=1e-13)
    with pytest.raises(ValueError):
        k(np.zeros((4, 2)), np.zeros((4, 2)))


def test_solver_arguments_without_device():
    k = q.Matern32(1.0)
    with pytest.raises(ValueError, match="must be sorted in order to use the QuasisepSolver"):
        QuasisepSolver(k, np.array([0.0, 2.0, 1.0]), Diagonal(np.ones(3)))
    with pytest.raises(ValueError, match="must be sorted"):
        GaussianProcess(k, np.array([0.0, 2.0, 1.0]), diag=0.1)
    with pytest.raises(TypeError, match="noise.Diagonal"):
        QuasisepSolver(k, np.arange(3.0), Dense(np.eye(3)))
    with pytest.raises(TypeError, match="covariance"):
        QuasisepSolver(k, np.arange(3.0), Diagonal(np.ones(3)), covariance=np.eye(3))


def test_default_solver_selection():
    gp = GaussianProcess(q.Matern32(1.0), np.arange(3.0), diag=0.1, _lazy=True)
    assert gp._solver_cls is QuasisepSolver
    gp = GaussianProcess(q.Matern32(1.0) + kernels.ExpSquared(1.0), np.arange(3.0), diag=0.1, _lazy=True)
    assert gp._solver_cls is DirectSolver
    gp = GaussianProcess(kernels.Matern32(1.0), np.arange(3.0), diag=0.1, _lazy=True)
    assert gp._solver_cls is DirectSolver
