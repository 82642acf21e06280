"""Plain NumPy oracles of the gradient of the quasiseparable log-likelihood (test infrastructure).

``value_and_grad`` is sequential and O(N): the tangent of the factor recursion of ``tests/_quasisep_np.py`` and of the
forward solve along every kernel parameter, and the diagonal of K^-1 from the backward recurrence.  Notation, for one
direction (a dot is the derivative):

    D_n = P - P_n,  D^-_n = A_n D_{n-1} A_n^T,  g = (P - D^-) h,  c = h^T g + noise,  w = g / sqrt c,  D_n = D^- + w w^T
    dD^- = dA D A^T + A D dA^T + A dD_{n-1} A^T,    dg = (dP - dD^-) h + (P - D^-) dh,    dc = dh^T g + h^T dg,
    dw = dg / sqrt c - w dc / 2c,                   dD_n = dD^- + dw w^T + w dw^T
    f = A s_{n-1},  z = (r - h^T f) / sqrt c,  s = f + w z,     M = (I - w h^T / sqrt c) A
    u = (I - w h^T / sqrt c) dA s_{n-1} + dw z - w (dh^T f / sqrt c + z dc / 2c),        ds_n = M ds_{n-1} + u
    dz = -(dh^T f + h^T (dA s_{n-1} + A ds_{n-1})) / sqrt c - z dc / 2c
    d log p = -1/2 sum dc / c - sum z dz
    (K^-1)_nn = (1 + u^T O_{n+1} u) / c_n,  u = A_{n+1} w_n,  O_n = T_n^T O_{n+1} T_n + h h^T / c_n,
    T_n = A_{n+1} (I - w_n h^T / sqrt c_n),  O_N = 0;   alpha = L^-T z.

The transitions' tangents come from ``kernels.quasisep.model_dphi`` (held to central differences and to mpmath in
``tests/test_quasisep_grad_cpu.py``); everything else is written here from the formulas.  All directions advance
together (arrays with a leading axis P), transitions are formed a block of steps at a time.

``dense_value_and_grad`` is the O(N^3) textbook identity 1/2 tr((alpha alpha^T - K^-1) dK) with LAPACK and dK by central
differences of the host kernel matrix (relative step h = 1e-6 max(1, |theta|), as ``oracle/grad_np.py``), taken at h and
at 2h and combined as (4 D(h) - D(2h)) / 3.  The plain difference at h carries a truncation error h^2 k''' / 6 per
entry; for ``Cosine(scale=2)`` at lags of 100, k''' / k' is about (2 pi tau / scale^2)^2 = 2.5e4, and at N = 1999 the plain
gradient is off by 1.2e-5 of itself (against a 40-digit evaluation of the rank-two form of that likelihood), above the
1e-6 it is used at.  The combination cancels that term; what is left is the rounding of the kernel matrix over the
step, 2e-7 of the gradient in that case and below 1e-7 in every other.
"""
import numpy as np

from tinygp_amd.kernels.quasisep import model_dphi


def value_and_grad(kernel, t, noise, r, block=4096, closed_loop_check=None):
    """``(log p, d log p / d parameters (P,), d / d noise (N,), alpha (N,))``.  ``closed_loop_check``: an optional
    list that receives max |dD_n - (M dD_{n-1} M^T + G_n)| per step (G_n: the step's tangent from dD_{n-1} = 0)."""
    s = kernel._ssm()
    tang = kernel._ssm_tangents()
    t, noise, r = (np.asarray(a, dtype=np.float64) for a in (t, noise, r))
    n, J, P = len(t), s.J, len(tang)
    h, Pinf = s.h, s.Pinf
    dh = np.stack([x.dh for x in tang]) if P else np.zeros((0, J))
    dPinf = np.stack([x.dPinf for x in tang]) if P else np.zeros((0, J, J))
    dt = np.diff(t, prepend=t[:1])
    eye = np.eye(J)
    D, dD = np.zeros((J, J)), np.zeros((P, J, J))
    sv, ds = np.zeros(J), np.zeros((P, J))
    c, w, z = np.empty(n), np.empty((n, J)), np.empty(n)
    acc_c, acc_z = np.zeros(P), np.zeros(P)

    def factor_tangent(Ai, dAi, D, dD, Dm, g, cn, sq, wn):
        X = dAi @ (D @ Ai.T)
        dDm = X + np.swapaxes(X, 1, 2) + Ai @ dD @ Ai.T
        dg = (dPinf - dDm) @ h + dh @ (Pinf - Dm).T
        dc = dh @ g + dg @ h
        dw = dg / sq - wn * (dc / (2 * cn))[:, None]
        return dDm + dw[:, :, None] * wn + wn[:, None] * dw[:, None, :], dc, dw

    for b0 in range(0, n, block):
        b1 = min(n, b0 + block)
        A = kernel._phi(dt[b0:b1])
        dA = np.stack([model_dphi(s, x.dleaves, dt[b0:b1]) for x in tang]) if P else np.zeros((0, b1 - b0, J, J))
        for i in range(b0, b1):
            Ai, dAi = A[i - b0], dA[:, i - b0]
            Dm = Ai @ D @ Ai.T
            g = (Pinf - Dm) @ h
            cn = h @ g + noise[i]
            sq = np.sqrt(cn)
            wn = g / sq
            dDn, dc, dw = factor_tangent(Ai, dAi, D, dD, Dm, g, cn, sq, wn)
            closed = eye - np.outer(wn, h) / sq
            M = closed @ Ai
            if closed_loop_check is not None and P:
                G = factor_tangent(Ai, dAi, D, np.zeros_like(dD), Dm, g, cn, sq, wn)[0]
                closed_loop_check.append(np.abs(dDn - (M @ dD @ M.T + G)).max())
            # forward solve and its tangent
            f = Ai @ sv
            zn = (r[i] - h @ f) / sq
            dAs = dAi @ sv
            u = dAs @ closed.T + dw * zn - wn * ((dh @ f) / sq + zn * dc / (2 * cn))[:, None]
            dz = -(dh @ f + (dAs + ds @ Ai.T) @ h) / sq - zn * dc / (2 * cn)
            ds = ds @ M.T + u
            sv = f + wn * zn
            D, dD = Dm + np.outer(wn, wn), dDn
            c[i], w[i], z[i] = cn, wn, zn
            acc_c += dc / cn
            acc_z += zn * dz
    logp = -0.5 * (z @ z + np.sum(np.log(c)) + n * np.log(2 * np.pi))
    kgrad = -0.5 * acc_c - acc_z

    # backward: alpha = L^-T z and the diagonal of K^-1
    alpha, kinv = np.empty(n), np.empty(n)
    Om, b = np.zeros((J, J)), np.zeros(J)
    hh = np.outer(h, h)
    for b1 in range(n, 0, -block):
        b0 = max(0, b1 - block)
        nxt = np.append(dt[b0 + 1:b1], dt[b1] if b1 < n else 0.0)  # the lag after each step; none after the last
        A = kernel._phi(dt[b0:b1])
        An = kernel._phi(nxt)
        for i in range(b1 - 1, b0 - 1, -1):
            sq = np.sqrt(c[i])
            Anx = An[i - b0]
            u = Anx @ w[i]
            kinv[i] = (1.0 + u @ Om @ u) / c[i]
            T = Anx @ (eye - np.outer(w[i], h) / sq)
            Om = T.T @ Om @ T + hh / c[i]
            alpha[i] = (z[i] - w[i] @ b) / sq
            b = A[i - b0].T @ (b + h * alpha[i])
    return logp, kgrad, 0.5 * (alpha * alpha - kinv), alpha


def set_parameters(kernel, theta):
    for (obj, name), v in zip(kernel.parameters(), theta):
        setattr(obj, name, float(v))


def get_parameters(kernel):
    return np.array([float(getattr(obj, name)) for obj, name in kernel.parameters()])


def _weighted_central_difference(kernel, t, W, theta0, i, step, rows=256):
    """sum(W * (K(theta_i + step) - K(theta_i - step))) / (2 step) for symmetric ``W`` and ``K``: only the blocks on and
    above the diagonal are evaluated."""
    n, total = len(t), 0.0
    for i0 in range(0, n, rows):
        i1 = min(n, i0 + rows)
        blocks = []
        for sgn in (1.0, -1.0):
            theta = theta0.copy()
            theta[i] = theta0[i] + sgn * step
            set_parameters(kernel, theta)
            blocks.append(np.asarray(kernel(t[i0:i1], t[i0:]), dtype=np.float64))
        prod = W[i0:i1, i0:] * (blocks[0] - blocks[1])
        total += np.sum(prod[:, :i1 - i0]) + 2.0 * np.sum(prod[:, i1 - i0:])
    return total / (2 * step)


def dense_value_and_grad(kernel, t, noise, r, skip=()):
    """LAPACK: ``(log p, kernel gradient (P,), noise gradient (N,), alpha (N,), K^-1)``; entries in ``skip`` are NaN
    (a parameter the host kernel cannot be differenced in: the quality of a critically damped SHO)."""
    t, noise, r = (np.asarray(a, dtype=np.float64) for a in (t, noise, r))
    n = len(t)
    K = np.asarray(kernel(t, t), dtype=np.float64) + np.diag(noise)
    L = np.linalg.cholesky(K)
    Kinv = np.linalg.inv(K)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, r))
    zz = np.linalg.solve(L, r)
    logp = -0.5 * zz @ zz - np.sum(np.log(np.diag(L))) - 0.5 * n * np.log(2 * np.pi)
    W = np.outer(alpha, alpha) - Kinv
    theta0 = get_parameters(kernel)
    g = np.full(len(theta0), np.nan)
    try:
        for i, th in enumerate(theta0):
            if i in skip:
                continue
            step = 1e-6 * max(1.0, abs(th))
            d1, d2 = (_weighted_central_difference(kernel, t, W, theta0, i, m * step) for m in (1.0, 2.0))
            g[i] = 0.5 * (4.0 * d1 - d2) / 3.0
    finally:
        set_parameters(kernel, theta0)
    return logp, g, 0.5 * np.diag(W).copy(), alpha, Kinv
