"""Inputs and high-precision references for the dense solver's shape tests (``test_gpu_1_solver_shapes.py``).

The points live in a box whose size does not depend on N, so every 128 x 128 tile of the kernel matrix, of the cross
covariance and of the Cholesky factor carries weight: a tile that a kernel drops, or a k-loop that stops one tile
early, moves the result by far more than rounding.  The three conditions that make this true are asserted here, on
the float64 reference alone (``check_factor`` / ``check_cross``); ``test_dense_shapes_cpu.py`` runs them at every
shape the GPU file uses.

References are SciPy LAPACK in float64 on the oracle's kernel matrix (``oracle.tinygp_np``); the matrix products
against the device's own factor are ``np.longdouble``.  Everything returned from a cache is read-only.
"""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla

from oracle import tinygp_np as o

TILE = 128
NS = (100, 128, 129, 257, 300, 1100)
WIDTHS = (1, 2, 7, 8, 9, 63, 64, 65, 128, 129, 200, 300)  # R (right-hand sides) and M (test points)
WMAX = max(WIDTHS)
FP32_NS = (129, 300)

# the conditional-covariance cases: (d, n, m, xt_given, test_noise, other_kernel, dtype)
_F64, _F32 = "float64", "float32"
COND_CASES = (
    # 1-D, test points given, test-point noise: every N with every M (M > N with ragged N included: 100 x 129 ... 300)
    [(1, n, m, True, True, False, _F64) for n in NS for m in WIDTHS]
    # 3-D without test-point noise: each N with the M that change a branch (one point, 64-block edge, tile edge, 3 tiles)
    + [(3, n, m, True, False, False, _F64) for n in NS for m in (1, 64, 65, 129, 300)]
    # X_test = None (m = N)
    + [(d, n, n, False, nz, False, _F64) for d in (1, 3) for n in (129, 300) for nz in (True, False)]
    # a kernel other than the solver's
    + [(d, n, m, True, True, True, _F64) for d in (1, 3) for n in (129, 300, 1100) for m in (65, 200)]
    + [(1, 300, 300, False, True, True, _F64)]
    # fp32
    + [(d, n, m, True, True, False, _F32) for d in (1, 3) for n in FP32_NS for m in (1, 64, 129, 300)]
    + [(1, n, n, False, True, False, _F32) for n in FP32_NS]
)


def kernel(mod, d):
    """The solver's kernel, from ``tinygp_amd.kernels`` or the oracle."""
    if d == 1:
        return 1.3 * mod.ExpSquared(1.5)
    return mod.Matern32(1.5, distance=mod.L2Distance())


def other_kernel(mod, d):
    """A second kernel for ``condition(kernel=...)`` and ``refactor``; as broad as the first (see ``check_cross``)."""
    if d == 1:
        return 0.8 * mod.Matern52(2.0)
    return 0.9 * mod.ExpSquared(2.5)


def _frozen(a):
    a.setflags(write=False)
    return a


def _points(n, d, seed, dtype):
    rng = np.random.default_rng([seed, n, d])
    X = np.sort(rng.uniform(0.0, 4.0, n)) if d == 1 else rng.uniform(0.0, 3.0, (n, 3))
    return X.astype(dtype)


@functools.lru_cache(maxsize=None)
def train(n, d, dtype=_F64):
    """``(X, noise diagonal)`` in ``dtype``: sorted U[0, 4] in 1-D, U[0, 3]^3 in 3-D, noise U[0.05, 0.15]."""
    diag = np.random.default_rng([2, n, d]).uniform(0.05, 0.15, n).astype(dtype)
    return _frozen(_points(n, d, 1, dtype)), _frozen(diag)


@functools.lru_cache(maxsize=None)
def query_points(m, d, dtype=_F64):
    """``(X_test, test-point noise)`` from the same box."""
    nz = np.random.default_rng([4, m, d]).uniform(0.01, 0.05, m).astype(dtype)
    return _frozen(_points(m, d, 3, dtype)), _frozen(nz)


def tile_norms(L):
    """Frobenius norms of the 128 x 128 tiles of ``|L|`` on or below the diagonal (ragged edge tiles as they are)."""
    nt = -(-L.shape[0] // TILE)
    return np.array([np.linalg.norm(L[i * TILE:(i + 1) * TILE, j * TILE:(j + 1) * TILE])
                     for i in range(nt) for j in range(i + 1)])


def check_factor(K, L):
    """Every tile of the factor matters and the problem is well posed."""
    norms = tile_norms(L)
    assert norms.min() >= 1e-6 * norms.max(), (norms.min(), norms.max())
    cond = np.linalg.cond(K)
    assert cond <= 1e6, cond


def check_cross(Ks):
    """No entry of the cross covariance is negligible beside the largest."""
    a = np.abs(Ks)
    assert a.min() >= 1e-3 * a.max(), (a.min(), a.max())


@functools.lru_cache(maxsize=None)
def reference(n, d, dtype=_F64):
    """float64 LAPACK reference of the factorisation at the (dtype-rounded) inputs; conditions asserted."""
    X, diag = train(n, d, dtype)
    X64, diag64 = X.astype(np.float64), diag.astype(np.float64)
    K = kernel(o, d)(X64, X64) + np.diag(diag64)
    L = np.tril(sla.cholesky(K, lower=True))
    check_factor(K, L)
    return SimpleNamespace(n=n, d=d, X=_frozen(X64), diag=_frozen(diag64), K=_frozen(K), L=_frozen(L))


@functools.lru_cache(maxsize=None)
def conditional(d, n, m, xt_given, test_noise, other, dtype=_F64):
    """``(C, var)``: ``Kss + diag(nz) - A^T A`` and ``diag(Kss) - colsum(A * A)`` with ``A = L^-1 Ks`` (direct.py:75-95)."""
    ref = reference(n, d, dtype)
    kern = (other_kernel if other else kernel)(o, d)
    if xt_given:
        Xt = query_points(m, d, dtype)[0].astype(np.float64)
        Ks, Kss = kern(ref.X, Xt), kern(Xt, Xt)
    else:
        assert m == n
        Ks = Kss = kern(ref.X, ref.X)
    check_cross(Ks)
    A = sla.solve_triangular(ref.L, Ks, lower=True, check_finite=False)
    C = Kss - A.T @ A
    var = np.diag(Kss) - np.sum(A * A, axis=0)
    if test_noise:
        C = C + np.diag(query_points(m, d, dtype)[1].astype(np.float64))
    return _frozen(C), _frozen(var)


@functools.lru_cache(maxsize=None)
def rhs(n, dtype=_F64):
    """Standard-normal (n, 300) block in ``dtype``; the tests use its leading R columns."""
    return _frozen(np.random.default_rng([5, n]).standard_normal((n, WMAX)).astype(dtype))


def dot_reference(L, Z):
    """``(L Z, |L| |Z|)``: the product in long double and the magnitude sum behind the componentwise bound
    ``|fl(L Z) - L Z| <= gamma_N |L| |Z|`` (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5: any
    order of summation)."""
    want = np.tril(L).astype(np.longdouble) @ Z.astype(np.longdouble)
    mag = np.abs(np.tril(L)).astype(np.float64) @ np.abs(Z).astype(np.float64)
    return want, mag


def dot_bar(n, dtype, mag):
    """``2 N eps |L| |Z|``: gamma_N, doubled for the conversions to and from the device's dtype."""
    return 2.0 * n * float(np.finfo(dtype).eps) * mag


def solve_reference(L, Y, transpose):
    return sla.solve_triangular(np.tril(L).astype(np.float64), Y.astype(np.float64), lower=True,
                                trans=1 if transpose else 0, check_finite=False)


def solve_bar(dtype, want):
    """(rtol, atol): 1e-10 and 1e-10 max|want| in fp64 (test_trsv_vs_lapack, test_trsm_right_lt_vs_lapack);
    2e-3 max|want| in fp32 (test_streaming_solves_match_lapack_and_the_stepwise_path)."""
    scale = float(np.max(np.abs(want)))
    if np.dtype(dtype) == np.float64:
        return 1e-10, 1e-10 * scale
    return 0.0, 2e-3 * scale


def posterior_bar(dtype):
    """The project's posterior bar (``TOL`` of test_gpu_1_gp.py; 5e-4 in fp32, test_default_jitter_and_fp32)."""
    t = 5e-7 if np.dtype(dtype) == np.float64 else 5e-4
    return dict(rtol=t, atol=t)


def failing_noise(n=300, at=200):
    """Noise diagonal with one negative entry in the second tile: the leading ``at`` x ``at`` minor is positive
    definite and pivot ``at + 1`` (1-based) is not."""
    diag = np.array(train(n, 1)[1])
    diag[at] = -2.0
    return diag
