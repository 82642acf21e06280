"""Plain NumPy, sequential statement of the quasiseparable posterior sampler (test infrastructure).

Matheron's rule: with f a joint prior draw at data and test points and eps a draw of the noise,

    s(.) = f(.) + k(., X) (K + D)^-1 (r - f(X) - D^1/2 eps)

has the posterior's mean and covariance.  The definition, value for value:

    points      p = 0 ... N + M - 1 of [X; X_test]; the merged grid is np.argsort(concatenation, kind="stable")
    normals     xi (N + M, J, R), row p for point p (not for a sorted position); eps (N, R)
    first       x = chol(P) xi[p]
    later       x_g = A(dt) x_{g-1} + chol(Q(dt)) xi[p_g],   Q(dt) = sym(P - A(dt) P A(dt)^T),   dt >= 0 to the predecessor
    prior       f = h^T x
    chol        unpivoted lower Cholesky of a J x J positive-semidefinite matrix with a guard: a pivot
                d <= 16 * 2^-52 * P[j, j] gives a zero column and leaves the Schur complement untouched
    v           r - f(X) - sqrt(noise) eps, column by column;   alpha = (K + D)^-1 v
    data        f(X) + v - noise alpha   (= f + K alpha)
    test        f(x) + k(x, X) alpha

No noise is added to the result.  The closure (alpha and k(x, X) alpha) is dense LAPACK here; ``dense`` gives the
conditional mean and covariance that the sampler's linear map must reproduce.
"""

import numpy as np

GUARD = 16 * 2.0 ** -52


def chol_psd(S, Pdiag):
    """The guarded Cholesky of the definition; ``Pdiag``: the diagonal of the stationary covariance."""
    S = np.array(S, dtype=np.float64)
    J = len(S)
    L = np.zeros((J, J))
    for j in range(J):
        d = S[j, j]
        if not d > GUARD * Pdiag[j]:
            continue
        sq = np.sqrt(d)
        L[j, j] = sq
        L[j + 1:, j] = S[j + 1:, j] / sq
        S[j + 1:, j + 1:] -= np.multiply.outer(L[j + 1:, j], L[j + 1:, j])
    return L


def merged_grid(t, xt):
    """``(coordinates of [X; X_test], the points in grid order)``."""
    cat = np.concatenate([np.asarray(t, dtype=np.float64), np.asarray(xt, dtype=np.float64).reshape(-1)])
    return cat, np.argsort(cat, kind="stable")


def process_noise(kernel, dt):
    """``(A(dt), chol(Q(dt)))``."""
    s = kernel._ssm()
    P = np.asarray(s.Pinf, dtype=np.float64)
    A = kernel._phi(np.asarray(dt, dtype=np.float64))
    Q = P - A @ P @ A.T
    return A, chol_psd(0.5 * (Q + Q.T), np.diag(P))


def prior(kernel, t, xt, xi):
    """The prior draw ``f`` (N + M, R), by point, from ``xi`` (N + M, J, R)."""
    s = kernel._ssm()
    h, P = np.asarray(s.h, dtype=np.float64), np.asarray(s.Pinf, dtype=np.float64)
    cat, order = merged_grid(t, xt)
    xi = np.asarray(xi, dtype=np.float64)
    f = np.empty((len(cat), xi.shape[2]))
    x = None
    for g, p in enumerate(order):
        if g == 0:
            x = chol_psd(P, np.diag(P)) @ xi[p]
        else:
            A, Lq = process_noise(kernel, cat[p] - cat[order[g - 1]])
            x = A @ x + Lq @ xi[p]
        f[p] = h @ x
    return f


def sample(kernel, t, noise, r, xt, xi, eps):
    """``(data (N, R), test (M, R))``: the draws of the definition for ``xi`` (N + M, J, R) and ``eps`` (N, R);
    ``xt``: the test points (M,), possibly empty."""
    t = np.asarray(t, dtype=np.float64)
    xt = np.asarray(xt, dtype=np.float64).reshape(-1)
    noise = np.asarray(noise, dtype=np.float64)
    n = len(t)
    f = prior(kernel, t, xt, xi)
    v = np.asarray(r, dtype=np.float64)[:, None] - f[:n] - np.sqrt(noise)[:, None] * np.asarray(eps, dtype=np.float64)
    K = np.asarray(kernel(t, t), dtype=np.float64) + np.diag(noise)
    alpha = np.linalg.solve(K, v)
    data = f[:n] + v - noise[:, None] * alpha
    test = f[n:] + np.asarray(kernel(xt, t), dtype=np.float64) @ alpha if len(xt) else np.zeros((0, v.shape[1]))
    return data, test


def unit_normals(n, m, J):
    """Every unit vector of the normals as a column: ``(xi (N + M, J, R), eps (N, R))`` with R = (N + M) J + N."""
    G = n + m
    R = G * J + n
    xi = np.zeros((G, J, R))
    xi.reshape(G * J, R)[np.arange(G * J), np.arange(G * J)] = 1.0
    eps = np.zeros((n, R))
    eps[np.arange(n), G * J + np.arange(n)] = 1.0
    return xi, eps


def dense(kernel, t, noise, r, xt):
    """The conditional mean ``Ks^T (K + D)^-1 r`` and covariance ``Kss - Ks^T (K + D)^-1 Ks`` of the latent process at
    ``xt``, from dense LAPACK."""
    t = np.asarray(t, dtype=np.float64)
    xt = np.asarray(xt, dtype=np.float64).reshape(-1)
    K = np.asarray(kernel(t, t), dtype=np.float64) + np.diag(noise)
    Ks = np.asarray(kernel(t, xt), dtype=np.float64)
    sol = np.linalg.solve(K, np.column_stack([np.asarray(r, dtype=np.float64), Ks]))
    return Ks.T @ sol[:, 0], np.asarray(kernel(xt, xt), dtype=np.float64) - Ks.T @ sol[:, 1:]


MIN_GAP = 0.02


def lattice(rng, count, start=0.0):
    """``count`` increasing coordinates whose neighbours lie 0.02 ... 0.25 apart.

    Why the test problems keep distinct neighbours at least MIN_GAP apart (ties, at distance exactly 0, are exact): the
    definition's Cholesky is unpivoted and its guard is absolute, so where the leading pivot of Q(dt) comes within a few
    orders of the guard -- dt around 1e-5 for the two-state kernels, 1e-4 ... 1e-3 for ``Matern52`` -- either a real
    pivot is dropped or the cancellation error of the pivot (about 2^-52 P[j, j]) is divided into the Schur complement,
    and chol(Q) chol(Q)^T misses Q by up to 8e-10 (measured over the kernels of ``_quasisep_cases`` on dt = 1e-6 ...
    1e-1).  That is far below the 5e-7 posterior bar, but above what the sampler's covariance is held to here (1e-12) and
    on the device (1e-9).  From dt = 5e-3 on the same scan stays at or below 2e-15 for every kernel."""
    return start + np.cumsum(rng.uniform(MIN_GAP, 0.25, count))


def problem(n, m, seed=5):
    """``(t, noise, r, xt)``: N sorted data points with the tie t[7] = t[6] (N > 7) and M unsorted test points drawn
    from one ``lattice``; from M = 4 on the lowest and the highest coordinate are test points, and two test points
    (M >= 2) lie on data points, the tied one among them."""
    rng = np.random.default_rng(seed + 1000 * n + m)
    coords = lattice(rng, n + m)
    pick = rng.permutation(n + m)[:m]
    if m >= 4:
        pick[:2] = [0, n + m - 1]
        pick[2:] = [i for i in rng.permutation(np.arange(1, n + m - 1))][:m - 2]
    is_test = np.zeros(n + m, dtype=bool)
    is_test[pick] = True
    t, xt = coords[~is_test], coords[is_test]
    if n > 7:
        t[7] = t[6]
    xt = np.concatenate([xt[1:-1][rng.permutation(max(m - 2, 0))], xt[:1], xt[-1:]]) if m >= 2 else xt
    if m >= 4:  # keep both ends: the points on data replace two inner ones
        xt[0], xt[1] = t[n // 2], t[min(6, n - 1)]
    elif m >= 2:
        xt[0], xt[-1] = t[n // 2], t[min(6, n - 1)]
    noise = rng.uniform(0.05, 0.2, n)
    r = rng.standard_normal(n)
    return t, noise, r, xt
