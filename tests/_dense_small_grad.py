"""Inputs and references for the gradients of the batched small dense path (``test_gpu_1_small_grad.py``,
``test_dense_small_grad_cpu.py``).

Inputs: the four programs of ``_dense_grad_np.PROGRAMS`` (``fast``, ``m32c``, ``ess``, and ``linear`` with its three
per-dimension scales) with their analytic dK/dtheta, at ``_dense_grad_np.inputs(n, d)``.  Member b of a batch has theta
scaled by ``1 + 0.04 b`` and the noise by ``1 + 0.1 b``.

Reference: that of ``_dense_grad_np.reference`` without its 128-tile conditions, which mean nothing below one tile:
float64, K from the oracle, LAPACK ``dpotri`` for K^-1, ``cho_solve`` for alpha, analytic dK.  It asserts its own
conditions: cond(K) <= 1e4; agreement with the LU route to 1e-10 of the largest component; and, for n >= 3, the last
row and the first column of K^-1 -- the two places an in-place inversion loses first -- each carry at least 100 bars in
every parameter's sum.  (At n = 2 ``linear`` carries 1.1 bars, hence "n >= 3"; at n = 1 the length-scale derivative is
exactly zero and the atol term of the bar covers it.)  Everything returned from a cache is read-only.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla

from oracle import tinygp_np as o

import _dense_grad_np as dg
import _dense_small as ds

BARS = dg.BARS["float64"]  # ll 1e-8, kernel 2e-6, noise 1e-6, mean 1e-7: rtol, and atol as that fraction of the largest
COND_MAX = 1e4
ROUTE_GAP_MAX = 1e-10
WEIGHT_MIN = 100.0
NAMES = tuple(dg.PROGRAMS)
BS = (1, 3)
_frozen = dg._frozen


def theta(name, b):
    return tuple(t * (1.0 + 0.04 * b) for t in dg.PROGRAMS[name][1])


def member_kernel(name, mod, b):
    """Program ``name`` with every parameter scaled by ``1 + 0.04 b``, from ``tinygp_amd.kernels`` or the oracle."""
    return dg.PROGRAMS[name][2](mod, theta(name, b))


def dim(name):
    return dg.PROGRAMS[name][0]


def member_noise(name, n, b):
    return _frozen(np.asarray(dg.inputs(n, dim(name))[1], dtype=np.float64) * (1.0 + 0.1 * b))


def edge_weights(Kinv, dKs, g):
    """``(last row, first column)``: the smallest ``|sum w_ij Kinv_ij dK_p,ij| / (frac max|g|)`` over the parameters p,
    the sum over the last row resp. the first column of the lower triangle (w = 1/2 on the diagonal, 1 below it)."""
    n = Kinv.shape[0]
    bar = BARS["kernel"] * np.abs(g).max()
    W = np.tril(np.ones((n, n)))
    W[np.diag_indices(n)] = 0.5
    WK = W * Kinv
    last = min(abs(float(np.sum(WK[n - 1] * dK[n - 1]))) for dK in dKs) / bar
    first = min(abs(float(np.sum(WK[:, 0] * dK[:, 0]))) for dK in dKs) / bar
    return last, first


@functools.lru_cache(maxsize=None)
def reference(name, n, b):
    """Member b of program ``name`` at ``_dense_grad_np.inputs(n, d)``: ``ll``, ``g`` (the kernel parameters, then the
    transform's three for ``linear``), ``noise`` = 1/2 diag(G), ``alpha``, and the figures of the conditions."""
    d, _, build, derivs = dg.PROGRAMS[name]
    th = theta(name, b)
    X, _, y = (np.asarray(a, dtype=np.float64) for a in dg.inputs(n, d))
    Xp = X.reshape(n, -1)
    K = build(o, th)(X, X) + np.diag(member_noise(name, n, b))
    L = sla.cholesky(K, lower=True, check_finite=False)
    Kinv, info = sla.lapack.dpotri(L, lower=1)
    assert info == 0
    Kinv = np.tril(Kinv) + np.tril(Kinv, -1).T
    alpha = sla.cho_solve((L, True), y, check_finite=False)
    ll = -0.5 * float(y @ alpha) - float(np.sum(np.log(np.diag(L)))) - 0.5 * n * math.log(2.0 * math.pi)
    G = np.outer(alpha, alpha) - Kinv
    dKs = derivs(th, Xp)
    g = np.array([0.5 * np.sum(G * dK) for dK in dKs])
    # 1. the problem is well posed
    cond = float(np.linalg.cond(K))
    assert cond <= COND_MAX, (name, n, b, cond)
    # 2. a second route to the same numbers: LU instead of Cholesky
    G2 = np.linalg.inv(K)
    a2 = G2 @ y
    G2 = np.outer(a2, a2) - G2
    g2 = np.array([0.5 * np.sum(G2 * dK) for dK in dKs])
    route_gap = float(np.abs(g - g2).max() / np.abs(g).max())
    assert route_gap <= ROUTE_GAP_MAX, (name, n, b, route_gap)
    # 3. the last row and the first column of K^-1 carry weight in every parameter's sum
    last, first = edge_weights(Kinv, dKs, g)
    if n >= 3:
        assert min(last, first) >= WEIGHT_MIN, (name, n, b, last, first)
    return SimpleNamespace(name=name, n=n, b=b, theta=th, ll=ll, g=_frozen(g), noise=_frozen(0.5 * np.diag(G)),
                           alpha=_frozen(alpha), cond=cond, route_gap=route_gap, last_row=last, first_col=first)


def errors(ref, ll, kernel_grad, noise_grad, mean_grad):
    """The worst error of each of the device's numbers in units of its bar (to print; ``check`` asserts)."""
    return dict(ll=abs(float(ll) - ref.ll) / (BARS["ll"] * abs(ref.ll)),
                kernel=dg.in_bars(kernel_grad, ref.g, BARS["kernel"], BARS["kernel"]),
                noise=dg.in_bars(noise_grad, ref.noise, BARS["noise"], BARS["noise"]),
                mean=dg.in_bars(mean_grad, ref.alpha, BARS["mean"], BARS["mean"]))


def check(ref, ll, kernel_grad, noise_grad, mean_grad):
    """The device's numbers against ``ref`` at the project's fp64 bars."""
    np.testing.assert_allclose(ll, ref.ll, rtol=BARS["ll"])
    np.testing.assert_allclose(kernel_grad, ref.g, rtol=BARS["kernel"], atol=BARS["kernel"] * np.abs(ref.g).max())
    np.testing.assert_allclose(noise_grad, ref.noise, rtol=BARS["noise"], atol=BARS["noise"] * np.abs(ref.noise).max())
    np.testing.assert_allclose(mean_grad, ref.alpha, rtol=BARS["mean"], atol=BARS["mean"] * np.abs(ref.alpha).max())


def full_gradient(kernel_grad, transform_grad):
    """The kernel parameters' gradient followed by the transform's (``linear``), as ``reference(...).g`` holds them."""
    if transform_grad is None:
        return np.asarray(kernel_grad, dtype=np.float64)
    return np.concatenate([np.asarray(kernel_grad, dtype=np.float64), np.ravel(transform_grad)])


# (n, b) of every reference the GPU file reads: the edges at B = 1 and 3, the ragged sets, the fail cases' neighbours
def gpu_cases():
    cases = {(n, b) for n in ds.EDGE_NS for b in range(max(BS))}
    cases |= {(n, b) for b, n in enumerate(ds.RAGGED)}
    cases |= {(n, b) for n, _ in ds.FAIL_CASES for b in range(3)}
    cases |= {(8, b) for b in range(7)} | {(ds.CAP, 0), (ds.CAP, 1), (ds.CAP + 1, 0), (ds.CAP + 1, 1), (40, 0), (40, 1)}
    return sorted(cases)
