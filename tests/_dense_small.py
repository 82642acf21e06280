"""Inputs and references for the batched small dense path (``test_gpu_1_small_batch.py``, ``test_dense_small_cpu.py``).

Inputs: the points and noise of ``_dense_np.train(n, d)`` and its two kernels.  Member b of a batch has the kernel's
parameters scaled by ``1 + 0.04 b`` and the noise by ``1 + 0.1 b``; the residual comes from ``default_rng([7, n])``.

Reference: SciPy LAPACK in float64 on the oracle's matrix.  It asserts its own conditions: cond(K) <= 1e4, and
agreement with a long-double Cholesky to 1e-12 relative (measured over d in {1, 3}, n = 1 .. 200: cond <= 3.4e3,
difference <= 7e-15), so that the project's log-likelihood bar, ``|got - want| <= 1e-8 max(1, |want|)``, measures the
device and not the reference.  Everything returned from a cache is read-only.
"""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla

from oracle import tinygp_np as o
from tinygp_amd import _ffi

import _dense_np as dn

CAP = _ffi.SMALL_MAX_N
EDGE_NS = (1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, CAP - 1, CAP)
DS = (1, 3)
BS = (1, 2, 3)
RAGGED = (1, CAP, 17, 64, 65, 128)
FAIL_CASES = ((65, 0), (65, 1), (65, 63), (65, 64), (CAP, CAP - 1))  # (n, p)
LEAF_N = 33
LEAF_DS = (1, 2, 16)
BAR = 1e-8
COND_MAX = 1e4
LONGDOUBLE_RTOL = 1e-12
LOG_2PI = float(np.log(2.0 * np.pi))


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


def member_kernel(mod, d, b, other=False):
    """``_dense_np.kernel`` (``other_kernel``) with every parameter scaled by ``1 + 0.04 b``."""
    s = 1.0 + 0.04 * b
    if not other:
        if d == 1:
            return (1.3 * s) * mod.ExpSquared(1.5 * s)
        return mod.Matern32(1.5 * s, distance=mod.L2Distance())
    if d == 1:
        return (0.8 * s) * mod.Matern52(2.0 * s)
    return (0.9 * s) * mod.ExpSquared(2.5 * s)


def member_noise(n, d, b, dtype="float64"):
    return _frozen((dn.train(n, d, dtype)[1].astype(np.float64) * (1.0 + 0.1 * b)).astype(dtype))


@functools.lru_cache(maxsize=None)
def resid(n, dtype="float64"):
    return _frozen(np.random.default_rng([7, n]).standard_normal(n).astype(dtype))


def within_bar(got, want):
    return abs(float(got) - float(want)) <= BAR * max(1.0, abs(float(want)))


def _cholesky_longdouble(K):
    A = np.asarray(K, dtype=np.longdouble)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def loglik(K, r):
    """``(value, figures)``: the float64 LAPACK log-likelihood of r under N(0, K), its conditions asserted."""
    K, r = np.asarray(K, dtype=np.float64), np.asarray(r, dtype=np.float64)
    n = K.shape[0]
    cond = float(np.linalg.cond(K))
    assert cond <= COND_MAX, cond
    L = sla.cholesky(K, lower=True)
    z = sla.solve_triangular(L, r, lower=True, check_finite=False)
    value = float(-0.5 * (z @ z) - np.sum(np.log(np.diag(L))) - 0.5 * n * LOG_2PI)
    Lq = _cholesky_longdouble(K)
    zq = np.zeros(n, dtype=np.longdouble)
    rq = r.astype(np.longdouble)
    for i in range(n):
        zq[i] = (rq[i] - Lq[i, :i] @ zq[:i]) / Lq[i, i]
    exact = -0.5 * (zq @ zq) - np.sum(np.log(np.diag(Lq))) - 0.5 * n * np.log(2.0 * np.pi, dtype=np.longdouble)
    diff = float(abs(value - exact) / max(1.0, abs(exact)))
    assert diff <= LONGDOUBLE_RTOL, diff
    return value, SimpleNamespace(cond=cond, longdouble_diff=diff)


@functools.lru_cache(maxsize=None)
def reference(n, d, b, other=False, dtype="float64"):
    """Member b at ``_dense_np.train(n, d)``: ``value`` and the reference's ``figures`` (inputs rounded to ``dtype``)."""
    X = dn.train(n, d, dtype)[0].astype(np.float64)
    noise = member_noise(n, d, b, dtype).astype(np.float64)
    K = member_kernel(o, d, b, other)(X, X) + np.diag(noise)
    value, figures = loglik(K, resid(n, dtype).astype(np.float64))
    return SimpleNamespace(value=value, figures=figures)


# ---- every leaf and operator (n = 33) -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def leaf_points(D):
    """U[0, 3 / D]^D: the L1 distances do not grow with D, so that no leaf's matrix shrinks to the identity."""
    X = np.random.default_rng([11, LEAF_N, D]).uniform(0.0, 3.0 / D, (LEAF_N, D))
    return _frozen(X[:, 0] if D == 1 else X)


def leaf_noise():
    """U[4, 8]: several leaves are not positive definite by themselves at D > 1 (a cosine of a distance, an L1 metric
    under a squared exponential) and have eigenvalues down to about -4 on these points; with this diagonal every
    member's matrix is positive definite with cond <= 1e4 (asserted), and entries of order one still carry weight."""
    return _frozen(np.random.default_rng([12, LEAF_N]).uniform(4.0, 8.0, LEAF_N))


def _as2d(X):
    X = np.asarray(X, dtype=np.float64)
    return X[:, None] if X.ndim == 1 else X


def leaf_members(kernels, transforms):
    """``[(name, product kernel, oracle matrix function of X)]``: one batch of members of different structure.  The
    oracle side is ``oracle.tinygp_np`` for what it has, and the reference's formulas written out for DotProduct /
    Polynomial (kernels/base.py:212-256) and ``transforms.Linear`` (transforms.py:39-72: the kernel at ``scale * x``)."""
    k = kernels

    def both(make):
        return make(k), (lambda X, m=make(o): m(X, X))

    def dot(X):
        return _as2d(X) @ _as2d(X).T

    out = [
        ("Constant",) + both(lambda m: m.Constant(0.7)),
        ("Exp",) + both(lambda m: m.Exp(1.1)),
        ("ExpSquared",) + both(lambda m: m.ExpSquared(1.4)),
        ("Matern32",) + both(lambda m: m.Matern32(1.3)),
        ("Matern52",) + both(lambda m: m.Matern52(0.9)),
        ("Cosine",) + both(lambda m: m.Cosine(5.0)),
        ("ExpSineSquared",) + both(lambda m: m.ExpSineSquared(1.7, gamma=0.6)),
        ("RationalQuadratic",) + both(lambda m: m.RationalQuadratic(1.2, alpha=0.8)),
        ("DotProduct", k.DotProduct(), dot),
        ("Polynomial", k.Polynomial(2.0, scale=2.5, sigma=0.7), lambda X: (dot(X) / 2.5**2 + 0.7**2) ** 2.0),
        ("sum",) + both(lambda m: m.Exp(1.1) + m.Matern32(1.3)),
        ("product",) + both(lambda m: m.Matern52(0.9) * m.Cosine(5.0)),
        ("nested",) + both(lambda m: 0.5 * m.Exp(1.1) + m.Matern52(0.9) * m.Cosine(5.0)
                           + m.Constant(0.2) * (m.ExpSquared(1.4) + m.RationalQuadratic(1.2, alpha=0.8))),
        ("metrics",) + both(lambda m: m.Exp(1.1, distance=m.L2Distance()) + m.ExpSquared(1.4, distance=m.L1Distance())
                            * m.Matern32(1.3, distance=m.L2Distance())),
        ("dot_sum", 0.3 * k.DotProduct() + k.Matern32(1.3),
         lambda X, m=o.Matern32(1.3): 0.3 * dot(X) + m(X, X)),
        ("linear_a", transforms.Linear(0.8, k.Matern32(1.3)), lambda X, m=o.Matern32(1.3): m(0.8 * X, 0.8 * X)),
        ("linear_b", transforms.Linear(1.25, k.Matern32(1.3)), lambda X, m=o.Matern32(1.3): m(1.25 * X, 1.25 * X)),
    ]
    return out


def leaf_reference(oracle_matrix, D, b):
    X = np.asarray(leaf_points(D), dtype=np.float64)
    K = oracle_matrix(X) + np.diag(leaf_noise() * (1.0 + 0.1 * b))
    return loglik(K, resid(LEAF_N))
