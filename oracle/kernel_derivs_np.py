"""TEST INFRASTRUCTURE: closed-form parameter derivatives of the stationary kernels in NumPy.

The reference has no derivative code of its own (its users differentiate with JAX autodiff, docs/tutorials/
quickstart.ipynb cell 4); the device evaluates d k / d theta in closed form (tinygp_amd/csrc/kmat.hip, leaf_deriv).  This
file states those closed forms a second time, independently, from the kernels' definitions
(/root/reference/src/tinygp/kernels/stationary.py:76-235, restated in oracle/tinygp_np.py), and tests/test_oracle.py holds
them against central differences of the oracle's own kernel matrices -- so that the gradient oracle (oracle/grad_np.py:
the trace identity with dK/dtheta by central differences) and the device's formulas are pinned by something other than
each other.  With r the kernel's distance, l its scale:

  Exp                k = exp(-r / l)                          dk/dl = k r / l^2
  ExpSquared         k = exp(-r^2 / (2 l^2))                  dk/dl = k r^2 / l^3
  Matern32           a = sqrt(3) r / l, k = (1 + a) e^-a      dk/dl = a^2 e^-a / l
  Matern52           a = sqrt(5) r / l, k = (1+a+a^2/3) e^-a  dk/dl = (a^2 / 3)(1 + a) e^-a / l
  Cosine             u = 2 pi r / l, k = cos u                dk/dl = u sin(u) / l
  ExpSineSquared     u = pi r / l, k = exp(-g sin^2 u)        dk/dl = k g 2 sin(u) cos(u) u / l,  dk/dg = -sin^2(u) k
  RationalQuadratic  q = r^2 / (2 a l^2), k = (1 + q)^-a      dk/dl = k / (1 + q) r^2 / l^3,  dk/da = k (q / (1 + q) - ln(1 + q))

The derivative with respect to the LOG of a per-dimension input scale (x_q -> s_q x_q for every point, what
``transforms.Linear`` / ``Cholesky`` with a vector do) is stated here through dk/dr, not through dk/dl: a stationary
leaf is a function of its distance r alone, so  dk/dlog s_q = (dk/dr)(dr/dlog s_q)  with, for the scaled difference
d_q = s_q (x1_q - x2_q),

  L1  r = sum_q |d_q|          dr/dlog s_q = |d_q|
  L2  r = sqrt(sum_q d_q^2)    dr/dlog s_q = d_q^2 / r   (0 at r = 0: |d_q| <= r, so the quotient is at most r)

and dk/dr from the definitions above (``dleaf_dr``):

  Exp  -k / l       ExpSquared  -k r / l^2       Matern32  -(sqrt(3) / l) a e^-a       Matern52  -(sqrt(5) / l)(a / 3)(1 + a) e^-a
  Cosine  -(2 pi / l) sin u       ExpSineSquared  -k g sin(2 u) pi / l       RationalQuadratic  -(r / l^2)(1 + q)^(-a - 1)

The dot-product leaf (reference kernels/base.py:212-256: DotProduct is l = 1, sigma = 0; Polynomial raises it to a
power, which the callers compose by the power rule  d u^P = P u^(P - 1) du [+ u^P ln u dP]):

  u = x1 . x2 / l^2 + sigma^2      du/dl = -2 x1 . x2 / l^3      du/dsigma = 2 sigma      du/dlog s_q = 2 x1_q x2_q / l^2
                                                                                          (x the scaled coordinates)
Every function keeps the dtype of its points (the two-point probe of tests/_kernel_derivs.py runs them in long double).
"""
import numpy as np

from oracle import tinygp_np as o


def _r(kernel, X1, X2, squared=False):
    d = np.asarray(X1)[:, None, :] - np.asarray(X2)[None, :, :]
    return kernel.distance.squared_distance(d) if squared else kernel.distance.distance(d)


def dleaf(kernel, X1, X2, param="scale"):
    """d k(X1, X2) / d param for a stationary leaf of oracle/tinygp_np.py; X (n, d)."""
    l = float(kernel.scale)
    if isinstance(kernel, o.Exp):
        assert param == "scale"
        r = _r(kernel, X1, X2)
        return np.exp(-r / l) * r / l**2
    if isinstance(kernel, o.ExpSquared):
        assert param == "scale"
        r2 = _r(kernel, X1, X2, squared=True)
        return np.exp(-0.5 * r2 / l**2) * r2 / l**3
    if isinstance(kernel, o.Matern32):
        assert param == "scale"
        a = np.sqrt(3) * _r(kernel, X1, X2) / l
        return a * a * np.exp(-a) / l
    if isinstance(kernel, o.Matern52):
        assert param == "scale"
        a = np.sqrt(5) * _r(kernel, X1, X2) / l
        return (a * a / 3) * (1 + a) * np.exp(-a) / l
    if isinstance(kernel, o.Cosine):
        assert param == "scale"
        u = 2 * np.pi * _r(kernel, X1, X2) / l
        return u * np.sin(u) / l
    if isinstance(kernel, o.ExpSineSquared):
        u = np.pi * _r(kernel, X1, X2) / l
        g = float(kernel.gamma)
        k = np.exp(-g * np.sin(u) ** 2)
        if param == "scale":
            return k * g * 2 * np.sin(u) * np.cos(u) * u / l
        assert param == "gamma"
        return -np.sin(u) ** 2 * k
    if isinstance(kernel, o.RationalQuadratic):
        a = float(kernel.alpha)
        r2 = _r(kernel, X1, X2, squared=True)
        q = 0.5 * r2 / (a * l**2)
        k = (1 + q) ** -a
        if param == "scale":
            return k / (1 + q) * r2 / l**3
        assert param == "alpha"
        return k * (q / (1 + q) - np.log1p(q))
    raise TypeError(f"no closed form for {type(kernel).__name__}")


def dleaf_dr(kernel, X1, X2):
    """d k / d r at the leaf's own distance r (L1 or L2), from the definitions; X (n, d)."""
    l = float(kernel.scale)
    r = _r(kernel, X1, X2)
    if isinstance(kernel, o.Exp):
        return -np.exp(-r / l) / l
    if isinstance(kernel, o.ExpSquared):
        return -np.exp(-0.5 * (r / l) ** 2) * r / l**2
    if isinstance(kernel, o.Matern32):
        a = np.sqrt(3) * r / l
        return -(np.sqrt(3) / l) * a * np.exp(-a)
    if isinstance(kernel, o.Matern52):
        a = np.sqrt(5) * r / l
        return -(np.sqrt(5) / l) * (a / 3) * (1 + a) * np.exp(-a)
    if isinstance(kernel, o.Cosine):
        return -(2 * np.pi / l) * np.sin(2 * np.pi * r / l)
    if isinstance(kernel, o.ExpSineSquared):
        u = np.pi * r / l
        g = float(kernel.gamma)
        return -np.exp(-g * np.sin(u) ** 2) * g * np.sin(2 * u) * np.pi / l
    if isinstance(kernel, o.RationalQuadratic):
        a = float(kernel.alpha)
        q = 0.5 * (r / l) ** 2 / a
        return -(r / l**2) * (1 + q) ** (-a - 1)
    raise TypeError(f"no closed form for {type(kernel).__name__}")


def ddistance_dlogscale(kernel, X1, X2):
    """d r / d log s_q for every input dimension q, at points that already carry the scales: (d, n1, n2)."""
    d = np.asarray(X1)[:, None, :] - np.asarray(X2)[None, :, :]
    if isinstance(kernel.distance, o.L1Distance):
        return np.moveaxis(np.abs(d), -1, 0)
    assert isinstance(kernel.distance, o.L2Distance)
    r = np.sqrt(np.sum(d * d, axis=-1))
    safe = np.where(r > 0, r, np.ones_like(r))
    return np.moveaxis(np.where((r > 0)[..., None], d * d / safe[..., None], np.zeros_like(d)), -1, 0)


def dleaf_dlogscale(kernel, X1, X2):
    """d k / d log s_q of a stationary leaf for every input dimension q: (d, n1, n2)."""
    return dleaf_dr(kernel, X1, X2)[None] * ddistance_dlogscale(kernel, X1, X2)


def dot_value(X1, X2, scale=1.0, sigma=0.0):
    """u = (x1 / l) . (x2 / l) + sigma^2 (DotProduct: l = 1, sigma = 0): (n1, n2)."""
    X1, X2 = np.asarray(X1), np.asarray(X2)
    return (X1 / scale) @ (X2 / scale).T + sigma * sigma * np.ones((len(X1), len(X2)), dtype=X1.dtype)


def ddot(X1, X2, scale, sigma, param):
    """d u / d scale or d u / d sigma."""
    X1, X2 = np.asarray(X1), np.asarray(X2)
    if param == "scale":
        return -2 * (X1 @ X2.T) / scale**3
    assert param == "sigma"
    return 2 * sigma * np.ones((len(X1), len(X2)), dtype=X1.dtype)


def ddot_dlogscale(X1, X2, scale):
    """d u / d log s_q for every input dimension q, at points that already carry the scales: (d, n1, n2)."""
    X1, X2 = np.asarray(X1), np.asarray(X2)
    return 2 * np.moveaxis(X1[:, None, :] * X2[None, :, :], -1, 0) / scale**2
