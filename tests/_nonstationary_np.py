"""A NumPy evaluator of the kernel program extended by the DOT leaf and the unary POW
(include/tgp_hip.h), written from the reference's formulas: kernels/stationary.py:76-235 for the
stationary leaves, kernels/base.py:212-256 for DotProduct / Polynomial.  It is the tests' own
restatement; oracle/ref_prog.py predates the two new ops.

``eval_prog`` evaluates the program for every pair of rows of X1 (n1, D) and X2 (n2, D); the DOT
leaf divides the raw sum x_i . x_j once by p0^2, like the device.  ``dot_bar`` is the scale that
the device's DOT rounding is measured against: sum_k |x_ik x_jk| / p0^2 + p1^2.
"""
import numpy as np

from tinygp_amd.kernels import base

K_EXP, K_EXPSQ, K_M32, K_M52, K_COS, K_ESS, K_RQ = (base.K_EXP, base.K_EXPSQ, base.K_M32, base.K_M52, base.K_COS,
                                                  base.K_ESS, base.K_RQ)


def _leaf(op, metric, p0, p1, X1, X2):
    if op == base.K_CONST:
        return np.full((X1.shape[0], X2.shape[0]), p0)
    if op == base.K_DOT:
        return (X1 @ X2.T) / (p0 * p0) + p1 * p1
    diff = X1[:, None, :] - X2[None, :, :]
    if metric == 1:  # L2: zero-safe sqrt, squared distance
        sq = np.sum(diff * diff, axis=-1)
        dist = np.sqrt(sq)
    else:  # L1: sum |d|, its square
        dist = np.sum(np.abs(diff), axis=-1)
        sq = dist * dist
    if op == K_EXP:
        return np.exp(-dist / p0)
    if op == K_EXPSQ:
        return np.exp(-0.5 * sq / p0**2)
    if op == K_M32:
        a = np.sqrt(3.0) * dist / p0
        return (1 + a) * np.exp(-a)
    if op == K_M52:
        a = np.sqrt(5.0) * dist / p0
        return (1 + a + a * a / 3) * np.exp(-a)
    if op == K_COS:
        return np.cos(2 * np.pi * dist / p0)
    if op == K_ESS:
        return np.exp(-p1 * np.sin(np.pi * dist / p0) ** 2)
    if op == K_RQ:
        return (1 + 0.5 * sq / p0**2 / p1) ** (-p1)
    raise ValueError(f"unknown op {op}")


def eval_prog(prog, X1, X2):
    """(n1, n2) values of the postfix program ``prog`` ([(op, metric, p0, p1), ...])."""
    X1 = np.asarray(X1, dtype=np.float64).reshape(np.shape(X1)[0], -1)
    X2 = np.asarray(X2, dtype=np.float64).reshape(np.shape(X2)[0], -1)
    stack = []
    for op, metric, p0, p1 in prog:
        if op in (base.K_ADD, base.K_MUL):
            b, a = stack.pop(), stack.pop()
            stack.append(a + b if op == base.K_ADD else a * b)
        elif op == base.K_POW:
            stack.append(stack.pop() ** p0)
        else:
            stack.append(_leaf(op, metric, p0, p1, X1, X2))
    assert len(stack) == 1
    return stack[0]


def eval_prog_diag(prog, X):
    """(n,) values k(x_i, x_i)."""
    X = np.asarray(X, dtype=np.float64).reshape(np.shape(X)[0], -1)
    return np.array([eval_prog(prog, X[i:i + 1], X[i:i + 1])[0, 0] for i in range(X.shape[0])])


def dot_bar(prog, X1, X2):
    """Per entry, the largest sum_k |x_ik x_jk| / p0^2 + p1^2 over the program's DOT leaves (1 without one)."""
    A, B = np.abs(np.asarray(X1, dtype=np.float64)), np.abs(np.asarray(X2, dtype=np.float64))
    A, B = A.reshape(A.shape[0], -1), B.reshape(B.shape[0], -1)
    bar = np.ones((A.shape[0], B.shape[0]))
    for op, _, p0, p1 in prog:
        if op == base.K_DOT:
            bar = np.maximum(bar, (A @ B.T) / (p0 * p0) + p1 * p1)
    return bar


def loglik(K, y):
    """Gaussian log-likelihood of y under N(0, K) by a SciPy Cholesky."""
    import scipy.linalg as sla

    L = sla.cholesky(K, lower=True)
    a = sla.solve_triangular(L, y, lower=True)
    return -0.5 * a @ a - np.sum(np.log(np.diag(L))) - 0.5 * len(y) * np.log(2 * np.pi)
