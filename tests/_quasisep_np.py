"""Plain NumPy, sequential oracle of the quasiseparable Cholesky factor (test infrastructure).

For sorted t, the covariance K + diag(noise) of a state-space kernel (h, P, A(dt)) has the lower Cholesky factor

    L[n, n] = sqrt(c_n),      L[i, j] = h^T A_i A_{i-1} ... A_{j+1} w_j     (i > j),

where c_n and w_n come from the Riccati (Kalman covariance) recursion, P_0 = 0 before the first point:

    P^-_n = A_n (P_{n-1} - P) A_n^T + P,   g = P^-_n h,   c_n = h^T g + noise_n,
    w_n = g / sqrt(c_n),                   P_n = P^-_n - g g^T / c_n.
"""

import numpy as np


def transitions(kernel, t):
    t = np.asarray(t, dtype=np.float64)
    dt = np.diff(t, prepend=t[:1])
    return kernel._phi(dt)


def factor(kernel, t, noise):
    s = kernel._ssm()
    A = transitions(kernel, t)
    n, J = len(t), s.J
    c = np.empty(n)
    w = np.empty((n, J))
    P = np.array(s.Pinf, copy=True)  # P - P_0 with P_0 = 0
    Pf = np.zeros((J, J))
    for i in range(n):
        Pm = A[i] @ (Pf - s.Pinf) @ A[i].T + s.Pinf if i else P
        g = Pm @ s.h
        c[i] = s.h @ g + noise[i]
        w[i] = g / np.sqrt(c[i])
        Pf = Pm - np.outer(g, g) / c[i]
    return A, s.h, c, w


def solve_lower(F, y):
    """L^-1 y for y (N,) or (N, R)."""
    A, h, c, w = F
    y = np.asarray(y, dtype=np.float64)
    z = np.empty_like(y)
    g = np.zeros((len(h),) + y.shape[1:])
    for i in range(len(c)):
        f = A[i] @ g
        z[i] = (y[i] - h @ f) / np.sqrt(c[i])
        g = f + np.multiply.outer(w[i], z[i])
    return z


def solve_upper(F, z):
    """L^-T z."""
    A, h, c, w = F
    z = np.asarray(z, dtype=np.float64)
    x = np.empty_like(z)
    b = np.zeros((len(h),) + z.shape[1:])
    for i in range(len(c) - 1, -1, -1):
        x[i] = (z[i] - w[i] @ b) / np.sqrt(c[i])
        b = A[i].T @ (b + np.multiply.outer(h, x[i]))
    return x


def dot_lower(F, z):
    """L @ z."""
    A, h, c, w = F
    z = np.asarray(z, dtype=np.float64)
    y = np.empty_like(z)
    g = np.zeros((len(h),) + z.shape[1:])
    for i in range(len(c)):
        f = A[i] @ g
        y[i] = np.sqrt(c[i]) * z[i] + h @ f
        g = f + np.multiply.outer(w[i], z[i])
    return y


def dense_factor(F):
    """L as a dense (N, N) matrix (small N only)."""
    n = len(F[2])
    return np.stack([dot_lower(F, e) for e in np.eye(n)], axis=1)


def log_probability(kernel, t, noise, r):
    F = factor(kernel, t, noise)
    z = solve_lower(F, r)
    return -0.5 * np.sum(z * z) - 0.5 * np.sum(np.log(F[2])) - 0.5 * len(t) * np.log(2 * np.pi)
