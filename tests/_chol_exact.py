"""Cholesky inputs whose factor is known in advance, and the check that names the first wrong tile, in NumPy alone.

K = L0 L0^T with an integer lower-triangular L0: K is exact in floating point (every partial sum of every product is an
integer below 2^53 in fp64, 2^24 in fp32: bounds()), the exact factor is L0 itself, and no reference computation is needed.

  family X  diagonal p, strictly-lower entries iid integers in {-a..a} outside the 128 x 128 diagonal blocks, which are p I.
            p is a power of two: every pivot stays p^2, every reciprocal and reciprocal square root is 2^-k exactly, every
            scaled entry is (p l) / p = l, every Schur complement an integer sum.  A correct factorisation returns L0 bit for
            bit, whatever its schedule.  fp64: p = 4096, a = 2.  fp32: p = 64, a = 1.
  family D  the same with dense diagonal blocks (fp64 only): the in-block eliminations, the inverses of the diagonal blocks
            and the in-panel solves see real work.  The inverse of p I + N does not terminate, so a device that multiplies
            by inverses is held to an absolute bar (BAR_D) and not to bits; LAPACK, which divides, still returns L0 exactly.

Unlike a kernel matrix of sorted 1-D points, whose factor decays to nothing a dozen tiles from the diagonal, every
off-diagonal tile of L0 weighs the same: one wrong, missing or doubled product l_ik l_jk moves an entry of L by at least
1 / p = 2^-12 (fp64), 256 times BAR_D.

No GPU and no library here: tests/test_chol_exact_cpu.py proves the properties and that the checks have teeth,
tests/test_gpu_0_chol_exact.py and tests/test_gpu_5_distributed.py run the device against them.
"""
import math
import zlib

import numpy as np

TILE = 128
PARAMS = {"f64": (4096, 2), "f32": (64, 1)}  # (p, a)
LIMIT = {"f64": 2 ** 53, "f32": 2 ** 24}
BAR_D = 2.0 ** -20  # family D on the device: 256 times below one wrong product (2^-12), ~1e5 above N eps at cond ~ 1


def _name(dtype):
    return {"float64": "f64", "float32": "f32"}[np.dtype(dtype).name]


class Factor(np.ndarray):
    """L0 with the key of its construction, (n, family, dtype name, seed): matrix() caches on it."""
    key = None

    def __array_finalize__(self, obj):
        self.key = None  # (slices and results of arithmetic are not the factor)


_factor_cache = {}  # one entry, like matrix()'s: consecutive cases on the same inputs build them once


def factor(n, family, dtype=np.float64, seed=0):
    """L0 (n, n), row-major, read-only.  Ragged n: the leading n x n part of the construction, the last block cut short."""
    name = _name(dtype)
    if family not in ("X", "D") or (family == "D" and name != "f64"):
        raise ValueError(f"no family {family!r} in {name}")
    if (n, family, name, seed) in _factor_cache:
        return _factor_cache[(n, family, name, seed)]
    p, a = PARAMS[name]
    rng = np.random.default_rng(zlib.crc32(f"chol-{family}-{n}-{name}-{seed}".encode()))
    L = np.tril(rng.integers(-a, a + 1, size=(n, n), dtype=np.int8), -1).astype(dtype)
    if family == "X":
        for j0 in range(0, n, TILE):
            L[j0:j0 + TILE, j0:j0 + TILE] = 0
    L[np.diag_indices(n)] = p
    L = L.view(Factor)
    L.key = (n, family, name, seed)
    L.flags.writeable = False
    _factor_cache.clear()
    _factor_cache[L.key] = L
    return L


def bounds(n, dtype):
    """(max |K_ij|, the limit below which integers are exact): p^2 + 2 a p + a^2 n bounds every partial sum of
    sum_k l_ik l_jk in any order -- at most one term p^2 (i = j = k), two terms a p, the others a^2 -- and with it every
    entry of K and of every Schur complement (K minus such a partial sum is the sum of the remaining terms)."""
    name = _name(dtype)
    p, a = PARAMS[name]
    return p * p + 2 * a * p + a * a * n, LIMIT[name]


_matrix_cache = {}  # one entry: the largest K of the GPU tests has 660 MB


def matrix(L0):
    """K = L0 L0^T in L0's dtype by ONE BLAS product (exact: bounds()), read-only, cached on the factor's key."""
    key = getattr(L0, "key", None)
    if key is not None and key in _matrix_cache:
        return _matrix_cache[key]
    assert bounds(L0.shape[0], L0.dtype)[0] < bounds(L0.shape[0], L0.dtype)[1]
    base = np.asarray(L0)
    K = base @ base.T
    K.flags.writeable = False
    if key is not None:
        _matrix_cache.clear()
        _matrix_cache[key] = K
    return K


def rhs(L0, seed=0):
    """(w, r = L0 w) with integer w in {-3..3}: |r_i| <= 3 (p + a n), exact in L0's dtype; so L0^-1 r = w exactly for a solver
    that substitutes with the exact inverses 1 / p of family X."""
    n = L0.shape[0]
    rng = np.random.default_rng(zlib.crc32(f"chol-rhs-{n}-{seed}".encode()))
    w = rng.integers(-3, 4, size=n).astype(L0.dtype)
    r = np.asarray(L0) @ w
    return w, r


def loglik(L0, w):
    """log N(r; 0, L0 L0^T) for r = L0 w: -w.w / 2 - sum log L0_ii - n / 2 log 2 pi, in math.fsum."""
    n = L0.shape[0]
    d = np.diag(np.asarray(L0)).astype(np.float64)
    ww = np.asarray(w, dtype=np.float64)
    return -0.5 * math.fsum(ww * ww) - math.fsum(np.log(d)) - 0.5 * n * math.log(2.0 * math.pi)


def normalization(L0):
    n = L0.shape[0]
    return math.fsum(np.log(np.diag(np.asarray(L0)).astype(np.float64))) + 0.5 * n * math.log(2.0 * math.pi)


# ---- the check ---------------------------------------------------------------------------------------------------------------

def _tiles(bad):
    """(tile rows, tile columns) bool: which 128 x 128 tiles of the (n, w) block hold a bad entry (ragged edges padded)."""
    n, w = bad.shape
    tr, tc = -(-n // TILE), -(-w // TILE)
    pad = np.zeros((tr * TILE, tc * TILE), dtype=bool)
    pad[:n, :w] = bad
    return pad.reshape(tr, TILE, tc, TILE).any(axis=(1, 3))


def _report(got, want, bad, col0, why):
    """Name the first wrong 128 x 128 tile (column by column) and what its residual looks like."""
    t = _tiles(bad)
    tj, ti = np.argwhere(t.T)[0]
    sl = (slice(ti * TILE, (ti + 1) * TILE), slice(tj * TILE, (tj + 1) * TILE))
    g, r = got[sl].astype(np.float64), want[sl].astype(np.float64)
    nbad = int(bad[sl].sum())
    with np.errstate(invalid="ignore"):
        dev = np.abs(g - r)[bad[sl]]
    fin = dev[np.isfinite(dev)]
    worst = f"largest deviation {fin.max():.3e}" if fin.size else "no finite deviation"
    nan = int((~np.isfinite(g)).sum())
    return (f"{why}: first wrong 128x128 tile (i, j) = ({ti}, {tj + col0 // TILE}) with {nbad} of {g.size} entries wrong, "
            f"{worst}{f', {nan} not finite' if nan else ''}; {int(t.sum())} tile(s) wrong in all")


def _check(got, L0, col0, close):
    want = np.asarray(L0)[:, col0:col0 + got.shape[1]]
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    if np.array_equal(got, want):  # (the common case in one pass; the upper triangle of L0 is zero)
        return
    i = np.arange(got.shape[0])[:, None]
    j = col0 + np.arange(got.shape[1])[None, :]
    lower = i >= j
    with np.errstate(invalid="ignore"):
        bad = lower & ~close(got, want)
        up = ~lower & ~(got == 0)  # (NaN is not zero)
    msgs = []
    if bad.any():
        msgs.append(_report(got, want, bad, col0, "the factor differs from L0"))
    if up.any():
        msgs.append(_report(got, want, up, col0, "non-zero above the diagonal"))
    assert not msgs, "; ".join(msgs)


def check_exact(got, L0, col0=0):
    """got == L0, entry by entry (as numbers: -0 is 0).  `got` may be the column block of L starting at column `col0`, a
    multiple of 128.  Raises AssertionError naming the first wrong tile, how many of its entries are wrong and the largest
    deviation, and separately any non-zero entry above the diagonal."""
    assert col0 % TILE == 0
    _check(got, L0, col0, lambda g, w: g == w)


def check_close(got, L0, bar, col0=0):
    """|got - L0| <= bar on and below the diagonal, exact zeros above it; the same report."""
    assert col0 % TILE == 0
    _check(got, L0, col0, lambda g, w: np.abs(g.astype(np.float64) - w) <= bar)


def worst(got, L0):
    """max |got - L0| over the lower triangle (NaN if any entry is)."""
    return float(np.max(np.abs(np.tril(got).astype(np.float64) - np.asarray(L0))))
