"""Plain NumPy oracles of the prediction of one term of a quasiseparable sum (test infrastructure).

For a ``Sum`` the state is block-diagonal, so the covariance between a term at x and the whole model at the data is
the model's own with the test-side observation vector ``h`` replaced by ``g``, ``h`` masked to the term's states.  With
the notation of ``_quasisep_predict_np`` (D, F, O, B driven by the data-side ``h``, exactly as there):

    q = A_l^T g,   e = P g - A_l D_i q,   e^- = A_r e
    mean_g(x) = q^T F_i + (A_r P g)^T B_{i+1}
    var_g(x)  = g^T P g - q^T D_i q - e^-T O_{i+1} e^-
"""

import numpy as np

import _quasisep_np as o
import _quasisep_predict_np as po


def predict_g(kernel, t, noise, r, xt, g):
    """``(mean, var)`` at ``xt`` of the term whose test-side vector is ``g`` (J,), the model ``kernel`` conditioned on
    the residual ``r``: the loop of ``_quasisep_predict_np.predict`` with ``g`` on the test side.  ``g`` of shape
    (K, J) gives (K, M) arrays from one pass over the data (the recurrences do not depend on ``g``)."""
    g = np.asarray(g, dtype=np.float64)
    if g.ndim == 2:
        shared = _recurrences(kernel, t, noise, r, xt)
        out = [_gather(kernel, t, xt, gk, shared) for gk in g]
        return np.stack([m for m, _ in out]), np.stack([v for _, v in out])
    return _gather(kernel, t, xt, g, _recurrences(kernel, t, noise, r, xt))


def _recurrences(kernel, t, noise, r, xt):
    """D_i, F_i and O_{i+1}, B_{i+1} at the intervals that hold a test point."""
    t = np.asarray(t, dtype=np.float64)
    xt = np.asarray(xt, dtype=np.float64)
    s = kernel._ssm()
    J, n = s.J, len(t)
    h, P = s.h, s.Pinf
    A, _, c, w = o.factor(kernel, t, noise, np.float64)
    a = po.alpha((A, h, c, w), np.asarray(r, dtype=np.float64))
    Ph = P @ h
    idx = po.intervals(t, xt)
    need_left = set(idx[idx >= 0].tolist())
    need_right = set((idx[idx + 1 < n] + 1).tolist())

    left = {}
    D, Fv = np.zeros((J, J)), np.zeros(J)
    for i in range(n):
        D = A[i] @ D @ A[i].T + np.multiply.outer(w[i], w[i])
        Fv = A[i] @ Fv + Ph * a[i]
        if i in need_left:
            left[i] = (D, Fv)

    right = {}
    Om, B = np.zeros((J, J)), np.zeros(J)
    eye = np.eye(J)
    for j in range(n - 1, -1, -1):
        if j + 1 < n:
            T = A[j + 1] @ (eye - np.multiply.outer(w[j], h) / np.sqrt(c[j]))
            Om = T.T @ Om @ T
            B = A[j + 1].T @ B
        Om = Om + np.multiply.outer(h, h) / c[j]
        B = B + h * a[j]
        if j in need_right:
            right[j] = (Om, B)
    return idx, left, right


def _gather(kernel, t, xt, g, shared):
    t = np.asarray(t, dtype=np.float64)
    xt = np.asarray(xt, dtype=np.float64)
    idx, left, right = shared
    n = len(t)
    Pg = kernel._ssm().Pinf @ g
    mean = np.zeros(len(xt))
    var = np.zeros(len(xt)) + g @ Pg
    for m, (x, i) in enumerate(zip(xt, idx)):
        e = Pg
        if i >= 0:
            D, Fv = left[i]
            Al = kernel._phi(np.asarray(x - t[i]))
            q = Al.T @ g
            Dq = D @ q
            mean[m] += q @ Fv
            var[m] -= q @ Dq
            e = Pg - Al @ Dq
        if i + 1 < n:
            Om, B = right[i + 1]
            Ar = kernel._phi(np.asarray(t[i + 1] - x))
            em = Ar @ e
            mean[m] += (Ar @ Pg) @ B
            var[m] -= em @ Om @ em
    return mean, var


def dense_term(model, term, t, noise, r, xt):
    """The same two quantities from dense LAPACK: ``term(t, xt)^T K^-1 r`` and ``term(xt) - diag(Ks^T K^-1 Ks)`` with
    ``K = model(t, t) + diag(noise)`` and ``Ks = term(t, xt)``."""
    t = np.asarray(t, dtype=np.float64)
    xt = np.asarray(xt, dtype=np.float64)
    K = np.asarray(model(t, t), dtype=np.float64) + np.diag(noise)
    Ks = np.asarray(term(t, xt), dtype=np.float64)
    sol = np.linalg.solve(K, np.column_stack([np.asarray(r, dtype=np.float64), Ks]))
    return Ks.T @ sol[:, 0], np.asarray(term(xt), dtype=np.float64) - np.sum(Ks * sol[:, 1:], axis=0)
