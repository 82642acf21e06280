"""Tile and pass edges of the dense path's kernel evaluation (csrc/kmat.hip): the trace contraction of the gradient at
one tile, an exact tile, one point into a second tile and three tiles with a ragged last one, for each evaluator (the
two-sum one of `amp * leaf` programs, the general one in family 0 and in family 2, and the input-dimension derivative
behind `transforms.Linear`); and `Kernel.matmul` on both sides of its 256-row / 256-column blocks, with more than one
column chunk, for one pass, a full pass of 8 vectors and a second pass of one.

Oracles: oracle/tinygp_np.py and oracle/grad_np.py (the trace identity with central differences of the oracle's kernel
matrix; see tests/test_gpu_2_grad.py for how far it can be trusted), with the reference's Polynomial formula
(kernels/base.py:254-256) restated here because the oracle module has no dot-product kernels.  Tolerances are those
of tests/test_gpu_2_grad.py (gradient 2e-6 of the largest component, noise gradient 1e-6, alpha 1e-7) and of
tests/test_gpu_0_kernels.py (`matmul`: rtol = atol = 1e-12).  The block-column gradient at N = 300, nb = 128,
GRAD_CHUNK = 128 is a case of tests/test_gpu_5_distributed.py::test_gradient_on_the_block_column_path_hip, where the
process-group fixture lives."""
import functools

import numpy as np
import pytest

from oracle import grad_np
from oracle import tinygp_np as o
from tinygp_amd import GaussianProcess, kernels, transforms

pytestmark = pytest.mark.gpu


class _Polynomial(o.Kernel):
    """Reference kernels/base.py:254-256: ((x1 / scale) . (x2 / scale) + sigma^2) ** order"""

    def __init__(self, order, scale, sigma):
        self.order, self.scale, self.sigma = order, scale, sigma

    def evaluate(self, X1, X2):
        return (np.sum((X1 / self.scale) * (X2 / self.scale), axis=-1) + np.square(self.sigma)) ** self.order


def _poly(mod, order, scale, sigma):
    return _Polynomial(order, scale, sigma) if mod is o else mod.Polynomial(order=order, scale=scale, sigma=sigma)


# name -> (theta0, build(module, theta)); g["kernel"] follows kernel.parameters(): Polynomial's are scale, sigma, order
GRAD_PROGRAMS = {
    "fast_amp_m32": ([1.8, 1.5], lambda k, t: t[0] * k.Matern32(t[1])),
    "general_sum_ess": ([2.25, 2.5, 0.3, 1.2, 0.7],
                        lambda k, t: t[0] * k.ExpSquared(t[1]) + t[2] * k.ExpSineSquared(t[3], gamma=t[4])),
    "fam2_expsq_plus_poly": ([1.5, 2.5, 3.0, 1.2, 2.0],
                             lambda k, t: t[0] * k.ExpSquared(t[1]) + _poly(k, t[4], t[2], t[3])),
}


@functools.lru_cache(maxsize=None)
def _series(n, ndim):
    rng = np.random.default_rng(1000 * ndim + n)
    X = np.sort(rng.uniform(0, 8 * n / 300, n)) if ndim == 1 else rng.uniform(0, 3, (n, ndim))
    y = np.sin(X if ndim == 1 else X[:, 0]) + 0.1 * rng.normal(size=n)
    diag = rng.uniform(0.05, 0.15, n)
    for a in (X, y, diag):
        a.setflags(write=False)
    return X, y, diag


def _check_grad(gp, got_params, want, y):
    ll, g = gp
    want_ll, want_g, want_noise, want_alpha = want
    np.testing.assert_allclose(ll, want_ll, rtol=1e-8)
    scale = np.abs(want_g).max() + 1e-12
    np.testing.assert_allclose(got_params, want_g, rtol=2e-6, atol=2e-6 * scale)
    np.testing.assert_allclose(g["noise_diag"], want_noise, rtol=1e-6, atol=1e-6 * np.abs(want_noise).max())
    np.testing.assert_allclose(g["mean"], want_alpha, rtol=1e-7, atol=1e-7 * np.abs(want_alpha).max())


@pytest.mark.parametrize("n", [127, 128, 129, 257])
@pytest.mark.parametrize("name", sorted(GRAD_PROGRAMS))
def test_gradient_at_tile_edges(name, n):
    theta0, build = GRAD_PROGRAMS[name]
    X, y, diag = _series(n, 1)
    gp = GaussianProcess(build(kernels, theta0), X, diag=diag)
    ll, g = gp.log_probability_and_grad(y)
    assert gp.solver.info == 0 and np.isfinite(ll) and gp.solver._prog is not None
    assert len(g["kernel"]) == len(theta0) == len(gp.kernel.parameters())
    want = grad_np.log_probability_and_grad(lambda t: build(o, t), theta0, X, diag, y)
    _check_grad((ll, g), g["kernel"], want, y)


def test_gradient_through_linear_one_point_into_the_second_tile():
    """`which_op < 0`: d ll / d s_q of `transforms.Linear` over a 3-D ExpSquared, N = 129."""
    n = 129
    X, y, diag = _series(n, 3)
    theta0 = [1.5, 1.2, 0.5, 2.0, 1.3]  # amp, ell, s0, s1, s2
    gp = GaussianProcess(theta0[0] * transforms.Linear(np.array(theta0[2:5]), kernels.ExpSquared(theta0[1])), X,
                         diag=diag)
    ll, g = gp.log_probability_and_grad(y)
    assert gp.solver.info == 0 and np.isfinite(ll)
    want = grad_np.log_probability_and_grad(lambda t: t[0] * grad_np.Scaled(t[2:5], o.ExpSquared(t[1])), theta0, X,
                                            diag, y)
    got = np.concatenate([np.asarray(g["kernel"], dtype=np.float64), np.asarray(g["transform"], dtype=np.float64)])
    assert len(g["kernel"]) == 2 and got.shape == (5,)
    _check_grad((ll, g), got, want, y)


MATMUL_PROGRAMS = {
    "fast_amp_m32": lambda k: 1.8 * k.Matern32(1.5),
    "general_sum_ess": lambda k: 2.25 * k.ExpSquared(2.5) + 0.3 * k.ExpSineSquared(1.2, gamma=0.7),
    "fam2_amp_poly": lambda k: 0.05 * _poly(k, 2.0, 3.0, 0.8),  # entries below 2 on [0, 3]^5, like the other two
}


@pytest.mark.parametrize("d", [1, 5])
@pytest.mark.parametrize("name", sorted(MATMUL_PROGRAMS))
def test_matmul_at_block_and_pass_edges(name, d):
    """(n1, n2) on both sides of GV_ROWS = GV_JB = 256 and with several column chunks; 1, 8 and 9 vectors are one
    pass, a full pass of GV_NV = 8, and a second pass of one."""
    k, ko = MATMUL_PROGRAMS[name](kernels), MATMUL_PROGRAMS[name](o)
    rng = np.random.default_rng(40 + d)
    for n1, n2 in [(1, 1), (255, 257), (257, 513)]:
        X1 = rng.uniform(0, 3, (n1, d) if d > 1 else n1)
        X2 = rng.uniform(0, 3, (n2, d) if d > 1 else n2)
        K = ko(X1, X2)
        V = rng.normal(size=(n2, 9))
        for nv in (1, 8, 9):
            v = V[:, 0] if nv == 1 else V[:, :nv]
            got = k.matmul(X1, X2, v)
            assert got.shape == (n1,) + v.shape[1:]
            np.testing.assert_allclose(got, K @ v, rtol=1e-12, atol=1e-12, err_msg=f"{n1}x{n2}, {nv} vectors")
