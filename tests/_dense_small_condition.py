"""Inputs and references for the joint posterior of the batched small dense path (``test_gpu_1_small_condition.py``,
``test_dense_small_condition_cpu.py``).

Inputs: points, noise, kernels and residuals are those of ``_dense_small.py``.  The m test points of a case are
``_dense_small_predict.query(n, d, m - 2)`` for m >= 3 (random points plus the member's first and last data point
shifted by 0.01) and ``dn.query_points(m, d)`` for m < 3.  The normals of a case are the first S rows of a fixed
(9, m) block from ``default_rng([21, n, m])``.

Reference: SciPy LAPACK in float64 on the oracle's matrices: ``cholesky``, ``solve_triangular``, mu = A^T z,
Sigma* = Kss + diag(tau) - A^T A with A = L^-1 K(X, X*), L22 = ``cholesky(Sigma*)``, f = mu + L22 xi.  It asserts its
own conditions at every case:
  (a) cond(K) <= 1e4, through ``ds.loglik``;
  (b) with tau = 0.1, cond(Sigma*) <= 1e4;
  (c) with tau = 0.1, agreement of mu, Sigma* and f with a long-double computation (``_cholesky_longdouble`` and a
      forward substitution) to 1e-12 of max(1, |want|);
  (d) with tau = 0.1: in Sigma*, the first row, the last row and every 64-row block of A carry at least 100 bars of
      (A^T A)_ii at one test point or more; in a draw, the first and the last column of L22 carry at least 100 bars of
      f - mu at one row or more.
With the default jitter (tau = sqrt(eps)) Sigma* is conditioned up to 7.7e9: only (a) is asserted, and the float64
reference's own distance from the long-double one is kept per case (``e64``) for the draws' bound.  A bar is that of
``_dense_np.solve_bar``.  Everything returned from a cache is read-only.
"""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla

from oracle import tinygp_np as o

import _dense_np as dn
import _dense_small as ds
import _dense_small_predict as sp

CAP = ds.CAP
TAU = 0.1
JITTER = float(np.sqrt(np.finfo(np.float64).eps))
COND_STAR_MAX = 1e4
LONGDOUBLE_TOL = 1e-12
WEIGHT_MIN = 100.0
SMAX = 9
_frozen = ds._frozen

_EDGES_N = (15, 16, 17, 63, 64, 65, 127, 128, 129)
_EDGES_M = (63, 64, 65, 127, 128, 129)
SHAPES = tuple(
    [(1, 1), (1, 3), (2, 2), (3, 1)]
    + [(n, m) for n in _EDGES_N for m in (1, 3)]
    + [(n, m) for n in (1, 3) for m in _EDGES_M]
    + [(63, 65), (64, 64), (65, 63), (64, 128), (128, 64), (127, 65), (129, 63), (96, 96)]
    + [(1, 191), (191, 1), (189, 3), (3, 189)]
    + [(100, CAP - 1 - 100)])
JITTER_SHAPES = ((17, 7), (64, 64), (128, 64), (1, 191))
assert all(n + m <= CAP for n, m in SHAPES + JITTER_SHAPES)


def test_points(n, d, m):
    """The m test points of the member at ``dn.train(n, d)``, in the shape of its points."""
    return sp.query(n, d, m - 2) if m >= 3 else dn.query_points(m, d)[0]


@functools.lru_cache(maxsize=None)
def normals(n, m):
    """The (9, m) standard normals of the case; a test takes its leading S rows."""
    return _frozen(np.random.default_rng([21, n, m]).standard_normal((SMAX, m)))


def joint(K, r, Ks, Kss, tau, xi, strict):
    """``(value, mu, Sigma*, draws, figures)``: the float64 LAPACK joint posterior of N(0, K) given r at cross
    covariances ``Ks`` (n, m) and prior covariance ``Kss`` (m, m) with ``tau`` (m,) on its diagonal, and
    ``mu + L22 xi_s`` for the rows of ``xi``; (a) always, (b) - (d) with ``strict``."""
    K, r = np.asarray(K, dtype=np.float64), np.asarray(r, dtype=np.float64)
    n, m = Ks.shape
    value, f0 = ds.loglik(K, r)  # (a)
    L = sla.cholesky(K, lower=True)
    z = sla.solve_triangular(L, r, lower=True, check_finite=False)
    A = sla.solve_triangular(L, Ks, lower=True, check_finite=False)
    mu = A.T @ z
    Sig = Kss + np.diag(tau) - A.T @ A
    L22 = sla.cholesky(Sig, lower=True)
    draws = mu + xi @ L22.T
    # the long-double computation
    Lq = ds._cholesky_longdouble(K)
    zq, Aq = sp._forward_longdouble(Lq, r), sp._forward_longdouble(Lq, Ks)
    muq = Aq.T @ zq
    Sigq = np.asarray(Kss, dtype=np.longdouble) + np.diag(np.asarray(tau, dtype=np.longdouble)) - Aq.T @ Aq
    L22q = ds._cholesky_longdouble(Sigq)
    drawsq = muq + np.asarray(xi, dtype=np.longdouble) @ L22q.T

    def rel(a, b):
        return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if b.size else 0.0

    fig = SimpleNamespace(cond=f0.cond, cond_star=float(np.linalg.cond(Sig)), min_eig=float(np.linalg.eigvalsh(Sig)[0]),
                          mean_diff=rel(mu, muq), cov_diff=rel(Sig, Sigq), draw_diff=rel(draws, drawsq),
                          e64=_frozen(np.abs(draws - drawsq).astype(np.float64)),
                          first_row=np.inf, last_row=np.inf, block=np.inf, first_col=np.inf, last_col=np.inf)
    # (d): the weight of a part of (A^T A)_ii in bars of Sigma*_ii, and of a column of L22 in bars of a draw
    rtol, atol = dn.solve_bar(np.float64, Sig)
    vbar = atol + rtol * np.abs(np.diag(Sig))
    V2 = A * A
    fig.first_row, fig.last_row = float(np.max(V2[0] / vbar)), float(np.max(V2[n - 1] / vbar))
    fig.block = min(float(np.max(V2[s:s + 64].sum(axis=0) / vbar)) for s in range(0, n, 64))
    rtol, atol = dn.solve_bar(np.float64, draws)
    fbar = atol + rtol * np.abs(draws)
    fig.first_col = float(np.max(np.abs(np.outer(xi[:, 0], L22[:, 0])) / fbar))
    fig.last_col = float(np.max(np.abs(xi[:, m - 1] * L22[m - 1, m - 1]) / fbar[:, m - 1]))
    if strict:
        assert fig.cond_star <= COND_STAR_MAX, fig.cond_star  # (b)
        assert max(fig.mean_diff, fig.cov_diff, fig.draw_diff) <= LONGDOUBLE_TOL, (fig.mean_diff, fig.cov_diff,
                                                                                    fig.draw_diff)  # (c)
        weights = (fig.first_row, fig.last_row, fig.block, fig.first_col, fig.last_col)
        assert min(weights) >= WEIGHT_MIN, weights  # (d)
    return value, _frozen(mu), _frozen(Sig), _frozen(draws), fig


@functools.lru_cache(maxsize=None)
def reference(n, d, b, m, jitter=False, predict_other=False):
    """Member b at ``dn.train(n, d)`` conditioned at ``test_points(n, d, m)`` with tau = 0.1 (``jitter``: sqrt(eps)),
    with its own kernel or (``predict_other``) member b's other kernel for the rows of the test points: ``value``,
    ``mean``, ``cov``, ``draws`` (9, m) for ``normals(n, m)``, ``tau`` (m,) and the ``figures``."""
    X = np.asarray(dn.train(n, d)[0], dtype=np.float64)
    Xt = np.asarray(test_points(n, d, m), dtype=np.float64)
    k = ds.member_kernel(o, d, b)
    pk = ds.member_kernel(o, d, b, other=True) if predict_other else k
    K = k(X, X) + np.diag(ds.member_noise(n, d, b))
    tau = np.full(m, JITTER if jitter else TAU)
    value, mean, cov, draws, fig = joint(K, ds.resid(n), pk(X, Xt), pk(Xt, Xt), tau, normals(n, m),
                                         strict=not jitter and not predict_other)
    return SimpleNamespace(value=value, mean=mean, cov=cov, draws=draws, tau=_frozen(tau), figures=fig)


def cases():
    """(n, d, b, m) of every tau = 0.1 reference the GPU file reads at the edges."""
    return [(n, d, b, m) for n, m in SHAPES for d in ds.DS for b in range(3)]
