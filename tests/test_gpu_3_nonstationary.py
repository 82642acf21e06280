"""DotProduct / Polynomial (reference kernels/base.py:212-256) on the device: the DOT leaf and the unary POW of the
kernel program in the tile evaluator, the diagonal, the fused matrix-vector product, the solvers and the gradient.

References: the tests' own NumPy evaluator of the extended program (tests/_nonstationary_np.py) for kernel values, a
SciPy Cholesky of the NumPy matrix for likelihoods and posteriors, central differences of that log-likelihood for
gradients.  Kernel values are held to 1e-13 (fp64) / 5e-6 (fp32) of the scale the DOT rounding lives on,
sum_k |x_ik x_jk| / p0^2 + p1^2, carried through POW as order * bar^order."""
import numpy as np
import pytest
import scipy.linalg as sla

import _nonstationary_np as nsn
from tinygp_amd import GaussianProcess, _device, kernels, transforms

pytestmark = pytest.mark.gpu

LL_RTOL = 1e-8
TOL = dict(rtol=5e-7, atol=5e-7)
VAL_TOL = {np.float64: 1e-13, np.float32: 5e-6}


def _value_cases():
    """name -> (kernel, bound(bar)): the size of an entry's rounding error in units of the tolerance"""
    return {
        "dot": (kernels.DotProduct(), lambda b: b),
        "poly3_sigma0": (kernels.Polynomial(order=3, scale=1.3, sigma=0.0), lambda b: 3 * b**3),
        "poly2.5": (kernels.Polynomial(order=2.5, scale=2.0, sigma=4.0), lambda b: 2.5 * b**2.5),
        "expsq+dot": (1.5**2 * kernels.ExpSquared(2.5) + 0.3 * kernels.DotProduct(), lambda b: 2.25 + 0.3 * b),
        "poly2*m32": (kernels.Polynomial(order=2, scale=1.3, sigma=0.4) * kernels.Matern32(1.2), lambda b: 2 * b**2),
    }


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("d", [1, 5, 16])
@pytest.mark.parametrize("n1,n2", [(256, 128), (200, 77)], ids=["tiles", "ragged"])
@pytest.mark.parametrize("name", sorted(_value_cases()))
def test_matrix_diagonal_and_matmul(name, n1, n2, d, dtype):
    k, bound = _value_cases()[name]
    rng = np.random.default_rng(7 + d)
    X1 = rng.normal(size=(n1, d)).astype(dtype)
    X2 = rng.normal(size=(n2, d)).astype(dtype)
    prog, _ = k._lower(X1)
    tol = VAL_TOL[dtype]

    got = _device.kmat(prog, X1, X2)
    want = nsn.eval_prog(prog, X1, X2)
    assert got.dtype == dtype and got.shape == (n1, n2)
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= tol * bound(nsn.dot_bar(prog, X1, X2))), err.max()
    if name == "poly3_sigma0":  # a negative dot product keeps its sign through pow(v, 3)
        neg = want < -1e3 * tol * bound(nsn.dot_bar(prog, X1, X2))
        assert neg.sum() > n1 * n2 // 8
        assert np.all(got[neg] < 0)

    gd = _device.kdiag(prog, X1)
    wd = nsn.eval_prog_diag(prog, X1)
    bd = np.diag(nsn.dot_bar(prog, X1, X1))
    assert np.all(np.abs(gd.astype(np.float64) - wd) <= tol * bound(bd))

    v = rng.normal(size=(n2, 3)).astype(dtype)
    gm = _device.kmat_gemv(prog, X1, X2, v)
    wm = want @ v.astype(np.float64)
    mbar = bound(nsn.dot_bar(prog, X1, X2)) @ np.abs(v.astype(np.float64))
    assert np.all(np.abs(gm.astype(np.float64) - wm) <= 4 * tol * mbar)

    # the same through the public interface: a tree with a device operand runs on the device
    kk = 1.0 * k
    np.testing.assert_array_equal(kk(X1, X2), _device.kmat(kk._lower(X1)[0], X1, X2))
    np.testing.assert_array_equal(kk(X1), _device.kdiag(kk._lower(X1)[0], X1))


def test_negative_base_with_an_integer_order_on_the_device():
    prog = kernels.Polynomial(order=3).program()
    X1 = np.array([[1.0, -2.0], [1.0, -2.0]])
    X2 = np.array([[-3.0, 1.0], [3.0, 1.0]])
    np.testing.assert_allclose(_device.kmat(prog, X1, X2)[0], [-125.0, 1.0], rtol=1e-15)
    np.testing.assert_allclose(_device.kmat(prog, X1.astype(np.float32), X2.astype(np.float32))[0], [-125.0, 1.0],
                               rtol=1e-6)


def _gp_cases():
    return {
        "dot": kernels.DotProduct(),
        "poly": kernels.Polynomial(order=2, scale=1.5, sigma=0.5),
        "expsq+dot": 1.5**2 * kernels.ExpSquared(2.5) + 0.3 * kernels.DotProduct(),
    }


def _data(n=300, d=2, seed=21):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (n, d))
    y = np.sin(X[:, 0]) + 0.3 * X[:, -1] + 0.1 * rng.normal(size=n)
    Xt = rng.uniform(-2, 2, (23, d))
    return X, y, Xt


@pytest.mark.parametrize("name", sorted(_gp_cases()))
def test_gp_on_the_device_matches_scipy(name):
    k = _gp_cases()[name]
    X, y, Xt = _data()
    diag = 0.2
    gp = GaussianProcess(k, X, diag=diag)
    assert gp.solver._prog is not None and gp.solver._covariance_value is None
    prog = k._lower(X)[0]
    K = nsn.eval_prog(prog, X, X) + diag * np.eye(len(X))
    np.testing.assert_allclose(gp.log_probability(y), nsn.loglik(K, y), rtol=LL_RTOL)
    np.testing.assert_allclose(gp.variance, np.diag(K), **TOL)

    L = sla.cholesky(K, lower=True)
    Ks = nsn.eval_prog(prog, X, Xt)
    A = sla.solve_triangular(L, Ks, lower=True)
    alpha = sla.cho_solve((L, True), y)
    loc = Ks.T @ alpha
    cov = nsn.eval_prog(prog, Xt, Xt) - A.T @ A
    c = gp.condition(y, Xt)
    np.testing.assert_allclose(c.gp.loc, loc, **TOL)
    np.testing.assert_allclose(c.gp.variance, np.diag(cov) + _default_diag(loc), **TOL)
    np.testing.assert_allclose(c.gp.covariance, cov + np.diag(_default_diag(loc)), **TOL)
    mu, var = gp.predict(y, Xt, return_var=True)
    np.testing.assert_allclose(mu, loc, **TOL)
    np.testing.assert_allclose(var, np.diag(cov) + _default_diag(loc), **TOL)
    # re-factoring at new hyper-parameters re-assembles on the device
    k2 = (2.0 * k) if name != "expsq+dot" else 1.1**2 * kernels.ExpSquared(2.0) + 0.5 * kernels.DotProduct()
    K2 = nsn.eval_prog(k2._lower(X)[0], X, X) + diag * np.eye(len(X))
    np.testing.assert_allclose(gp.solver.factor_log_probability(y - gp.loc, k2), nsn.loglik(K2, y), rtol=LL_RTOL)
    assert gp.solver._prog is not None


def _default_diag(loc):
    from tinygp_amd.gp import _default_diag as dd

    return np.broadcast_to(dd(loc), loc.shape)


def _grad_cases():
    return {
        "dot": lambda t: kernels.DotProduct(),
        "poly": lambda t: kernels.Polynomial(order=t[0], scale=t[1], sigma=t[2]),
        "poly*m32": lambda t: (kernels.Polynomial(order=t[0], scale=t[1], sigma=t[2])
                               * kernels.Matern32(1.2, distance=kernels.L2Distance())),
        "expsq+dot": lambda t: 1.5**2 * kernels.ExpSquared(2.5) + 0.3 * kernels.DotProduct(),
        "linear(poly)": lambda t: transforms.Linear(np.array([0.7, 1.6]),
                                                    kernels.Polynomial(order=t[0], scale=t[1], sigma=t[2])),
    }


def _numpy_ll(k, X, diag, y):
    prog, P = k._lower(X)
    return nsn.loglik(nsn.eval_prog(prog, P, P) + diag * np.eye(len(y)), y)


@pytest.mark.parametrize("name", sorted(_grad_cases()))
def test_log_probability_and_grad_central_differences(name):
    X, y, _ = _data(n=200, seed=4)
    diag = 0.3
    # an integer order keeps K positive definite; sigma keeps the base positive (d/d order takes its log)
    k = _grad_cases()[name]([2.0, 2.0, 2.0])
    gp = GaussianProcess(k, X, diag=diag)
    ll, g = gp.log_probability_and_grad(y)
    assert gp.solver._prog is not None
    np.testing.assert_allclose(ll, _numpy_ll(k, X, diag, y), rtol=LL_RTOL)

    def cdiff(set_, x0):  # five-point central difference: truncation O(h^4), round-off eps |ll| cond(K) / h
        h = 1e-3 * max(1.0, abs(x0))
        f = []
        for m in (2, 1, -1, -2):
            set_(x0 + m * h)
            f.append(_numpy_ll(k, X, diag, y))
        set_(x0)
        return (-f[0] + 8 * f[1] - 8 * f[2] + f[3]) / (12 * h)

    want = [cdiff(lambda v, o=obj, a=attr: setattr(o, a, v), getattr(obj, attr)) for obj, attr in k.parameters()]
    assert len(g["kernel"]) == len(want)
    if want:
        scale = np.abs(want).max()
        np.testing.assert_allclose(g["kernel"], want, rtol=1e-6, atol=1e-6 * scale)
    if name.startswith("linear"):
        s = k.scale

        def set_q(q):
            def f(v):
                s[q] = v
            return f

        wt = [cdiff(set_q(q), s[q]) for q in range(len(s))]
        np.testing.assert_allclose(g["transform"], wt, rtol=1e-6, atol=1e-6 * np.abs(wt).max())
    prog, P = k._lower(X)
    alpha = np.linalg.solve(nsn.eval_prog(prog, P, P) + diag * np.eye(len(y)), y)
    np.testing.assert_allclose(g["mean"], alpha, rtol=1e-7, atol=1e-7 * np.abs(alpha).max())


def test_bit_identical_run_to_run():
    X, y, _ = _data(n=1000, d=3, seed=9)
    k = 1.5**2 * kernels.ExpSquared(2.5) + kernels.Polynomial(order=3, scale=1.7, sigma=0.6)
    prog = k._lower(X)[0]
    a, b = _device.kmat(prog, X, X), _device.kmat(prog, X, X)
    assert a.tobytes() == b.tobytes()
    r1 = GaussianProcess(k, X, diag=0.2).log_probability_and_grad(y)
    r2 = GaussianProcess(k, X, diag=0.2).log_probability_and_grad(y)
    assert np.float64(r1[0]).tobytes() == np.float64(r2[0]).tobytes()
    assert np.array(r1[1]["kernel"]).tobytes() == np.array(r2[1]["kernel"]).tobytes()


@pytest.fixture(scope="module")
def pg():
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29633", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    yield dist
    dist.destroy_process_group()


def test_block_column_driver_matches_the_single_gpu_solver(pg):
    from tinygp_amd.solvers import DistributedDirectSolver

    X, y, Xt = _data(n=2000, d=2, seed=31)
    k = 1.5**2 * kernels.ExpSquared(2.5) + 0.3 * kernels.DotProduct()
    ll1, g1 = GaussianProcess(k, X, diag=0.1).log_probability_and_grad(y)
    gp = GaussianProcess(k, X, diag=0.1, solver=DistributedDirectSolver, nb=256, dist=pg)
    np.testing.assert_allclose(gp.log_probability(y), ll1, rtol=1e-10)
    ll2, g2 = gp.log_probability_and_grad(y)
    np.testing.assert_allclose(ll2, ll1, rtol=1e-10)
    scale = np.abs(np.array(g1["kernel"])).max()
    np.testing.assert_allclose(g2["kernel"], g1["kernel"], rtol=1e-6, atol=1e-6 * scale)
    np.testing.assert_allclose(g2["mean"], g1["mean"], rtol=1e-6, atol=1e-7 * np.abs(g1["mean"]).max())
    c1 = GaussianProcess(k, X, diag=0.1).condition(y, Xt)
    c2 = gp.condition(y, Xt)
    np.testing.assert_allclose(c2.gp.loc, c1.gp.loc, **TOL)
    np.testing.assert_allclose(c2.gp.variance, c1.gp.variance, **TOL)
    gp.solver.close()
