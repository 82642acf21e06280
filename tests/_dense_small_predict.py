"""Inputs and references for the predictions of the batched small dense path (``test_gpu_1_small_predict.py``,
``test_dense_small_predict_cpu.py``).

Inputs: points, noise, kernels and residuals are those of ``_dense_small.py`` (``dn.train(n, d)``, ``member_kernel``,
``member_noise``, ``resid``).  The test points of a case are ``dn.query_points(m, d)[0]`` followed by the member's first
and last data point, each shifted by +0.01 in every coordinate: a test point beside a data point puts weight on that
row of v = L^-1 k*, and the last row is where a forward substitution loses first (with random points alone the last
row's share of sum v^2 falls to 1.8e-8).

Reference: SciPy LAPACK in float64 on the oracle's matrices: ``cholesky``, ``solve_triangular``, mean = A^T z,
var = k** - colsum(A^2) with A = L^-1 K(X, X*).  It asserts its own conditions at every case:
  (a) cond(K) <= 1e4;
  (b) agreement with a long-double forward substitution to 1e-12 of max(1, |want|), for mean and variance;
  (c) for the model's own kernel, the first row, the last row and every 64-row block of v carry at least 100 bars of
      sum v^2 at one test point or more;
  (d) k*_0 alpha_0 and k*_{n-1} alpha_{n-1} carry at least 100 bars of the mean at one test point or more.
A bar is that of ``_dense_np.solve_bar``: rtol 1e-10 plus atol 1e-10 max|want| per member.  Everything returned from a
cache is read-only.
"""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla

from oracle import tinygp_np as o

import _dense_np as dn
import _dense_small as ds

RANDOM_COUNTS = (1, 5)  # the random test points of a case; two more are added
LONGDOUBLE_TOL = 1e-12
WEIGHT_MIN = 100.0
_frozen = ds._frozen


def _as2d(X):
    X = np.asarray(X)
    return X[:, None] if X.ndim == 1 else X


@functools.lru_cache(maxsize=None)
def query(n, d, m_random, dtype="float64"):
    """The (m_random + 2) test points of the member at ``dn.train(n, d)``, in the shape of its points."""
    X = dn.train(n, d, dtype)[0]
    Q = dn.query_points(m_random, d, dtype)[0]
    extra = np.stack([X[0], X[-1]]) + np.asarray(0.01, dtype=X.dtype)
    return _frozen(np.concatenate([Q, extra.astype(X.dtype)], axis=0))


def many_points(m, d):
    """m test points for the test-point edges: ``query(cap, d, m - 2)`` has the two added points last."""
    return dn.query_points(m, d)[0]


def bars(got, want):
    """The largest error of ``got`` in units of the fp64 solve bar of ``want``."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    rtol, atol = dn.solve_bar(np.float64, want)
    return float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want)))) if want.size else 0.0


def check(got, want, what=""):
    rtol, atol = dn.solve_bar(np.float64, want)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)


def _forward_longdouble(Lq, B):
    Bq = np.asarray(B, dtype=np.longdouble)
    out = np.zeros_like(Bq)
    for i in range(Lq.shape[0]):
        out[i] = (Bq[i] - Lq[i, :i] @ out[:i]) / Lq[i, i]
    return out


def posterior(K, r, Ks, kss, own=True):
    """``(value, mean, var, figures)``: the float64 LAPACK posterior of N(0, K) given r at cross covariances ``Ks``
    (n, m) and prior variances ``kss`` (m,), its conditions asserted ((c) only for the model's own kernel)."""
    K, r = np.asarray(K, dtype=np.float64), np.asarray(r, dtype=np.float64)
    n, m = Ks.shape
    value, f = ds.loglik(K, r)  # (a), and the value's own long-double check
    L = sla.cholesky(K, lower=True)
    z = sla.solve_triangular(L, r, lower=True, check_finite=False)
    A = sla.solve_triangular(L, Ks, lower=True, check_finite=False)
    mean, var = A.T @ z, kss - np.sum(A * A, axis=0)
    # (b)
    Lq = ds._cholesky_longdouble(K)
    zq, Aq = _forward_longdouble(Lq, r), _forward_longdouble(Lq, Ks)
    mean_q, var_q = Aq.T @ zq, np.asarray(kss, dtype=np.longdouble) - np.sum(Aq * Aq, axis=0)
    mean_diff = float(np.max(np.abs(mean - mean_q) / np.maximum(1.0, np.abs(mean_q)))) if m else 0.0
    var_diff = float(np.max(np.abs(var - var_q) / np.maximum(1.0, np.abs(var_q)))) if m else 0.0
    assert mean_diff <= LONGDOUBLE_TOL and var_diff <= LONGDOUBLE_TOL, (mean_diff, var_diff)
    fig = SimpleNamespace(cond=f.cond, mean_diff=mean_diff, var_diff=var_diff, first_row=np.inf, last_row=np.inf,
                          block=np.inf, first_term=np.inf, last_term=np.inf,
                          min_var=float(np.min(var / kss)) if m else np.inf)
    if m:
        # (c): the weight of a part of sum v^2 in bars of the variance, the best test point counts
        rtol, atol = dn.solve_bar(np.float64, var)
        vbar = atol + rtol * np.abs(var)
        V2 = A * A
        fig.first_row, fig.last_row = float(np.max(V2[0] / vbar)), float(np.max(V2[n - 1] / vbar))
        fig.block = min(float(np.max(V2[s:s + 64].sum(axis=0) / vbar)) for s in range(0, n, 64))
        if own:
            assert min(fig.first_row, fig.last_row, fig.block) >= WEIGHT_MIN, (fig.first_row, fig.last_row, fig.block)
        # (d): the first and the last term of the mean's sum in bars of the mean
        alpha = sla.solve_triangular(L, z, lower=True, trans=1, check_finite=False)
        rtol, atol = dn.solve_bar(np.float64, mean)
        mbar = atol + rtol * np.abs(mean)
        fig.first_term = float(np.max(np.abs(Ks[0] * alpha[0]) / mbar))
        fig.last_term = float(np.max(np.abs(Ks[n - 1] * alpha[n - 1]) / mbar))
        assert min(fig.first_term, fig.last_term) >= WEIGHT_MIN, (fig.first_term, fig.last_term)
    return value, _frozen(mean), _frozen(var), fig


@functools.lru_cache(maxsize=None)
def reference(n, d, b, m_random, predict_other=False):
    """Member b at ``dn.train(n, d)`` predicted at ``query(n, d, m_random)``, with its own kernel or (``predict_other``)
    with member b's other kernel for k* and k**: ``value``, ``mean``, ``var`` (no jitter) and the ``figures``."""
    X = np.asarray(dn.train(n, d)[0], dtype=np.float64)
    Xt = np.asarray(query(n, d, m_random), dtype=np.float64)
    k = ds.member_kernel(o, d, b)
    pk = ds.member_kernel(o, d, b, other=True) if predict_other else k
    K = k(X, X) + np.diag(ds.member_noise(n, d, b))
    value, mean, var, fig = posterior(K, ds.resid(n), pk(X, Xt), np.diag(pk(Xt, Xt)), own=not predict_other)
    return SimpleNamespace(value=value, mean=mean, var=var, figures=fig)


def cases():
    """(n, d, b, m_random) of every reference the GPU file reads at the edges."""
    return [(n, d, b, mr) for n in ds.EDGE_NS for d in ds.DS for b in range(3) for mr in RANDOM_COUNTS]
