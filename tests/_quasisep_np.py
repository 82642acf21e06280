"""Plain NumPy, sequential oracle of the quasiseparable Cholesky factor (test infrastructure).

For sorted t, the covariance K + diag(noise) of a state-space kernel (h, P, A(dt)) has the lower Cholesky factor

    L[n, n] = sqrt(c_n),      L[i, j] = h^T A_i A_{i-1} ... A_{j+1} w_j     (i > j),

where c_n and w_n come from the Riccati (Kalman covariance) recursion, P_0 = 0 before the first point:

    P^-_n = A_n (P_{n-1} - P) A_n^T + P,   g = P^-_n h,   c_n = h^T g + noise_n,
    w_n = g / sqrt(c_n),                   P_n = P^-_n - g g^T / c_n.

Every function takes a ``dtype``: ``np.float64`` (the default; transitions from ``kernel._phi``, the oracle the device
is held to), ``np.longdouble`` (the extended-precision reference where it is the x87 80-bit format, see ``EXTENDED``)
or ``MP`` (50-digit ``mpmath`` numbers in object arrays: slow, for cross-checks at small N and as the extended
reference where ``np.longdouble`` is only a double).  Beyond float64 the transitions are evaluated in that dtype by
``model_transitions`` from the leaf table the device reads (``kernel._ssm()``), with leaf formulas written here,
independently of ``kernels/quasisep.py``.
"""

import numpy as np

MP = object  # dtype of the mpmath route
EXTENDED = bool(np.finfo(np.longdouble).eps < 1e-18)  # np.longdouble carries a 64-bit significand
EXT = np.longdouble if EXTENDED else MP  # what the extended-precision tests pass as dtype

# leaf kinds of include/tgp_hip.h (TGP_QS_*)
_EXP, _M32, _M52, _COS, _CELERITE, _SHO_UNDER, _SHO_CRIT, _SHO_OVER = range(8)


def _mp():
    import mpmath

    mpmath.mp.dps = 50
    return mpmath


def cast(a, dtype):
    """``a`` as an array of ``dtype`` (float64 values are taken exactly)."""
    if dtype is MP:
        mpf = _mp().mpf

        def one(v):
            if isinstance(v, mpf):
                return v
            hi = float(v)  # a longdouble is the exact sum of two doubles
            return mpf(hi) + mpf(float(v - hi)) if np.isfinite(hi) else mpf(hi)

        return np.asarray(np.frompyfunc(one, 1, 1)(np.asarray(a, dtype=object)), dtype=object)
    return np.asarray(a, dtype=dtype)


def to_f64(a):
    return np.asarray(a, dtype=np.float64)


def _fn(name, dtype):
    if dtype is MP:
        f = np.frompyfunc(getattr(_mp(), name), 1, 1)
        return lambda x: f(np.asarray(x, dtype=object))
    return getattr(np, name)


def _leaf(kind, p, dt, dtype):
    """Rows of one leaf's A(dt) = expm(F dt) for an array of lags ``dt`` of ``dtype``; ``p``: its float64 table row."""
    exp, cos, sin, sqrt = (_fn(n, dtype) for n in ("exp", "cos", "sin", "sqrt"))
    p = cast(p, dtype)
    one = cast([1.0], dtype)[0]
    if kind == _EXP:
        return [[exp(-p[0] * dt)]]
    if kind in (_M32, _SHO_CRIT):  # a double root f of the characteristic polynomial
        f = p[0]
        e = exp(-f * dt)
        return [[e * (1 + f * dt), e * dt], [-e * f * f * dt, e * (1 - f * dt)]]
    if kind == _M52:  # a triple root: exp(-f dt) (I + N dt + N^2 dt^2 / 2), N = F + f I
        f = p[0]
        e, x = exp(-f * dt), f * dt
        return [[e * (1 + x + x * x / 2), e * dt * (1 + x), e * dt * dt / 2],
                [-e * f * x * x / 2, e * (1 + x - x * x), e * dt * (1 - x / 2)],
                [e * f * f * x * (x / 2 - 1), e * f * x * (x - 3), e * (1 - 2 * x + x * x / 2)]]
    if kind in (_COS, _CELERITE):  # a rotation by d dt, damped by c dt
        c, d = (0 * one, p[0]) if kind == _COS else (p[0], p[1])
        e = exp(-c * dt)
        return [[e * cos(d * dt), -e * sin(d * dt)], [e * sin(d * dt), e * cos(d * dt)]]
    # SHO, F = [[0, 1], [-w^2, -w/Q]]: roots -a0 +- i b0 (under-damped) or -a0 +- b0 (over-damped), a0 = w / 2Q.
    # The table's third parameter (b0 / a0 rounded to float64) is not read: it is recomputed in this dtype.
    w, q = p[0], p[1]
    a0 = w / (2 * q)
    if kind == _SHO_UNDER:
        b0 = a0 * sqrt(4 * q * q - one)
        e = exp(-a0 * dt)
        C, S = e * cos(b0 * dt), e * sin(b0 * dt) / b0  # S = e^-a0dt sin(b0 dt) / b0
    else:
        f = sqrt(one - 4 * q * q)
        b0 = a0 * f
        if dtype is MP:  # no overflow in mpmath: the textbook form
            cosh, sinh = _fn("cosh", dtype), _fn("sinh", dtype)
            e = exp(-a0 * dt)
            C, S = e * cosh(b0 * dt), e * sinh(b0 * dt) / b0
        else:  # the two decaying modes exp(-(a0 -+ b0) dt); a0 - b0 = 2 w Q / (1 + f)
            slow, fast = exp(-(2 * w * q / (1 + f)) * dt), exp(-(a0 + b0) * dt)
            C, S = (slow + fast) / 2, -slow * _fn("expm1", dtype)(-2 * b0 * dt) / (2 * b0)
    return [[C + a0 * S, S], [-w * w * S, C - a0 * S]]


def model_transitions(ssm, dt, dtype):
    """A(dt) of the whole model, shape ``dt.shape + (J, J)``, in ``dtype``: entry (r, c) is the product over the
    leaves of the term that both states belong to (Sum: block-diagonal; Product: Kronecker), zero otherwise."""
    dt = cast(dt, dtype)
    J = ssm.J
    leaves = [_leaf(int(row[0]), row[1:], dt, dtype) for row in ssm.leaves]
    out = np.zeros(dt.shape + (J, J), dtype=dtype)
    if dtype is MP:
        out = cast(out, MP)
    for r in range(J):
        for c in range(J):
            a, b = ssm.state_map[r], ssm.state_map[c]
            if np.any((a < 0) != (b < 0)):
                continue
            v = cast(np.ones(dt.shape), dtype)
            for l in np.nonzero(a >= 0)[0]:
                v = v * leaves[l][a[l]][b[l]]
            out[..., r, c] = v
    return out


def transitions(kernel, t, dtype=np.float64):
    t = np.asarray(t, dtype=np.float64)
    dt = np.diff(t, prepend=t[:1])  # in float64, as the device forms it
    if dtype is np.float64:
        return kernel._phi(dt)
    return model_transitions(kernel._ssm(), dt, dtype)


def _sqrt(x):
    return x.sqrt() if hasattr(x, "sqrt") and not isinstance(x, np.generic) else np.sqrt(x)


def _dtype_of(F):
    return MP if F[2].dtype == object else F[2].dtype.type


def factor(kernel, t, noise, dtype=np.float64):
    s = kernel._ssm()
    A = transitions(kernel, t, dtype)
    h, Pinf, noise = cast(s.h, dtype), cast(s.Pinf, dtype), cast(noise, dtype)
    n, J = len(t), s.J
    c = np.empty(n, dtype=dtype)
    w = np.empty((n, J), dtype=dtype)
    Pf = None
    for i in range(n):
        Pm = A[i] @ (Pf - Pinf) @ A[i].T + Pinf if i else Pinf  # P_0 = 0 before the first point
        g = Pm @ h
        c[i] = h @ g + noise[i]
        w[i] = g / _sqrt(c[i])
        Pf = Pm - np.multiply.outer(g, g) / c[i]
    return A, h, c, w


def solve_lower(F, y, dtype=None):
    """L^-1 y for y (N,) or (N, R)."""
    A, h, c, w = F
    dtype = _dtype_of(F) if dtype is None else dtype
    y = cast(y, dtype)
    z = np.empty_like(y)
    g = cast(np.zeros((len(h),) + y.shape[1:]), dtype)
    for i in range(len(c)):
        f = A[i] @ g
        z[i] = (y[i] - h @ f) / _sqrt(c[i])
        g = f + np.multiply.outer(w[i], z[i])
    return z


def solve_upper(F, z, dtype=None):
    """L^-T z."""
    A, h, c, w = F
    dtype = _dtype_of(F) if dtype is None else dtype
    z = cast(z, dtype)
    x = np.empty_like(z)
    b = cast(np.zeros((len(h),) + z.shape[1:]), dtype)
    for i in range(len(c) - 1, -1, -1):
        x[i] = (z[i] - w[i] @ b) / _sqrt(c[i])
        b = A[i].T @ (b + np.multiply.outer(h, x[i]))
    return x


def dot_lower(F, z, dtype=None):
    """L @ z."""
    A, h, c, w = F
    dtype = _dtype_of(F) if dtype is None else dtype
    z = cast(z, dtype)
    y = np.empty_like(z)
    g = cast(np.zeros((len(h),) + z.shape[1:]), dtype)
    for i in range(len(c)):
        f = A[i] @ g
        y[i] = _sqrt(c[i]) * z[i] + h @ f
        g = f + np.multiply.outer(w[i], z[i])
    return y


def dense_factor(F):
    """L as a dense (N, N) matrix (small N only)."""
    n = len(F[2])
    return np.stack([dot_lower(F, e) for e in np.eye(n)], axis=1)


def log_probability(kernel, t, noise, r, dtype=np.float64, F=None):
    F = factor(kernel, t, noise, dtype) if F is None else F
    z = solve_lower(F, r, dtype)
    two_pi = 2 * _mp().pi if dtype is MP else 8 * np.arctan(dtype(1))
    return -(np.sum(z * z) + np.sum(_fn("log", dtype)(F[2])) + len(t) * _fn("log", dtype)(two_pi)) / 2
