"""Plain NumPy, sequential oracle of the quasiseparable conditional mean and variance (test infrastructure).

Notation of ``_quasisep_np``: A_n = A(t_n - t_{n-1}), h, P, factor data c_n, w_n; alpha = K^-1 r.  For a test point
x let i be the last data index with t_i <= x (-1 before the first point), A_l = A(x - t_i), A_r = A(t_{i+1} - x).

    forward    D_n = A_n D_{n-1} A_n^T + w_n w_n^T            F_n = A_n F_{n-1} + P h alpha_n
    backward   O_n = h h^T / c_n + G_n^T A_{n+1}^T O_{n+1} A_{n+1} G_n,   G_n = I - w_n h^T / sqrt(c_n)
               B_n = h alpha_n + A_{n+1}^T B_{n+1}
    q = A_l^T h,   e = P h - A_l D_i q,   e^- = A_r e
    mean(x) = q^T F_i + (A_r P h)^T B_{i+1}
    var(x)  = h^T P h - q^T D_i q - e^-T O_{i+1} e^-

D_{-1}, F_{-1}, O_N and B_N are zero, which drops the terms a point outside the data has no neighbour for.  Only the
states at the intervals that hold a test point are kept, so the memory is O(N J^2) for the transitions and O(M J^2)
for the rest, and the oracle runs at sizes where the dense formula cannot.
"""

import numpy as np

import _quasisep_np as o


def intervals(t, xt):
    """Index of the last data point <= each test point (``side="right"``), -1 before the first."""
    return np.searchsorted(np.asarray(t, dtype=np.float64), np.asarray(xt, dtype=np.float64), side="right") - 1


def alpha(F, r):
    return o.solve_upper(F, o.solve_lower(F, r))


def predict(kernel, t, noise, r, xt, F=None, dtype=np.float64):
    """``(mean, var)`` at the test points ``xt`` (any order) of the GP with covariance k(t, t) + diag(noise)
    conditioned on the residual ``r``.  ``F``: ``_quasisep_np.factor(kernel, t, noise, dtype)`` if already at hand.
    ``dtype``: as in ``_quasisep_np`` (the lags x - t_i are formed in float64, as the device forms them)."""
    t = np.asarray(t, dtype=np.float64)
    xt = np.asarray(xt, dtype=np.float64)
    s = kernel._ssm()
    J, n = s.J, len(t)
    h, P = o.cast(s.h, dtype), o.cast(s.Pinf, dtype)
    phi = kernel._phi if dtype is np.float64 else (lambda lag: o.model_transitions(s, lag, dtype))
    zeros = lambda *shape: o.cast(np.zeros(shape), dtype)  # noqa: E731
    A, _, c, w = o.factor(kernel, t, noise, dtype) if F is None else F
    a = alpha((A, h, c, w), o.cast(r, dtype))
    Ph = P @ h
    idx = intervals(t, xt)
    need_left = set(idx[idx >= 0].tolist())
    need_right = set((idx[idx + 1 < n] + 1).tolist())

    left = {}
    D, Fv = zeros(J, J), zeros(J)
    for i in range(n):
        D = A[i] @ D @ A[i].T + np.multiply.outer(w[i], w[i])
        Fv = A[i] @ Fv + Ph * a[i]
        if i in need_left:
            left[i] = (D, Fv)

    right = {}
    Om, B = zeros(J, J), zeros(J)
    eye = o.cast(np.eye(J), dtype)
    for j in range(n - 1, -1, -1):
        if j + 1 < n:
            T = A[j + 1] @ (eye - np.multiply.outer(w[j], h) / o._sqrt(c[j]))
            Om = T.T @ Om @ T
            B = A[j + 1].T @ B
        Om = Om + np.multiply.outer(h, h) / c[j]
        B = B + h * a[j]
        if j in need_right:
            right[j] = (Om, B)

    mean = zeros(len(xt))
    var = zeros(len(xt)) + h @ Ph
    for m, (x, i) in enumerate(zip(xt, idx)):
        e = Ph
        if i >= 0:
            D, Fv = left[i]
            Al = phi(np.asarray(x - t[i]))
            q = Al.T @ h
            Dq = D @ q
            mean[m] += q @ Fv
            var[m] -= q @ Dq
            e = Ph - Al @ Dq
        if i + 1 < n:
            Om, B = right[i + 1]
            Ar = phi(np.asarray(t[i + 1] - x))
            em = Ar @ e
            mean[m] += (Ar @ Ph) @ B
            var[m] -= em @ Om @ em
    return mean, var


def dense(kernel, t, noise, r, xt):
    """The same two quantities from dense LAPACK: ``Ks^T K^-1 r`` and ``diag(Kss - Ks^T K^-1 Ks)``."""
    t = np.asarray(t, dtype=np.float64)
    xt = np.asarray(xt, dtype=np.float64)
    K = np.asarray(kernel(t, t), dtype=np.float64) + np.diag(noise)
    Ks = np.asarray(kernel(t, xt), dtype=np.float64)
    sol = np.linalg.solve(K, np.column_stack([np.asarray(r, dtype=np.float64), Ks]))
    return Ks.T @ sol[:, 0], np.asarray(kernel(xt), dtype=np.float64) - np.sum(Ks * sol[:, 1:], axis=0)
