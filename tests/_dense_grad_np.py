"""Inputs and the exact reference for the dense gradient's tile tests (``test_gpu_2_grad_tiles.py``, the two box cases
of ``test_gpu_5_distributed.py``; run without a GPU by ``test_dense_grad_cpu.py``).

The points are those of ``_dense_np.train``: a box whose size does not depend on N, so ``dK/dtheta`` does not decay
to nothing a tile away from the diagonal and EVERY 128 x 128 tile of ``K^-1`` enters the gradient with weight.  That
is a condition, asserted here on the float64 reference alone (``reference``), next to cond(K) and the agreement of two
routes to the reference; ``test_dense_grad_cpu.py`` runs the conditions at every case the GPU files use.

The reference is  g_p = 1/2 sum (alpha alpha^T - K^-1) o dK_p  in float64 with
  * K from the oracle (``oracle.tinygp_np``), L = LAPACK's Cholesky factor, K^-1 = dpotri(L) symmetrised,
    alpha = cho_solve(L, y);
  * dK_p ANALYTIC: the leaves' closed forms of ``oracle/kernel_derivs_np.py`` composed by the sum and product rules,
    written out per program below -- no differencing anywhere (``oracle/grad_np.py`` differentiates K by central
    differences, noise ~1e-8 of the largest component; the CPU file ties the two together at N = 300).
Everything returned from a cache is read-only.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import scipy.linalg as sla

import _dense_np as dn
from oracle import grad_np
from oracle import kernel_derivs_np as kd
from oracle import tinygp_np as o

TILE = dn.TILE
_F64, _F32 = "float64", "float32"

# the project's bars (tests/test_gpu_2_grad.py): rtol, and atol as the same fraction of the largest component.  (fp32:
# 2e-3 for the gradients; the older fp32 case does not look at the mean gradient alpha = K^-1 y, which carries the same
# cond(K) eps error as K^-1 and is held to the same 2e-3 here.)
BARS = {
    _F64: dict(ll=1e-8, kernel=2e-6, noise=1e-6, mean=1e-7),
    _F32: dict(ll=5e-4, kernel=2e-3, noise=2e-3, mean=2e-3),
}
WEIGHT_FACTOR = {_F64: 100.0, _F32: 10.0}  # every tile weighs at least this many bars
SECOND_PASS = 1024  # sum_partials_kernel: one workgroup of 1024 threads, a second trip of its loop from here on
EVERY_TILE_AT_33 = ("fast",)  # the programs whose every tile still weighs 100 bars at 33 tiles (the others: the tail)


# ---- programs: name -> (input dimension, theta0, build(module, theta), derivatives(theta, X (n, d))) -----------------
def _build_fast(mod, t):
    return t[0] * mod.ExpSquared(t[1])


def _dk_fast(t, X):
    leaf = o.ExpSquared(t[1])
    return [leaf(X, X), t[0] * kd.dleaf(leaf, X, X)]


def _build_m32c(mod, t):
    return mod.Matern32(t[0], distance=mod.L2Distance()) + mod.Constant(t[1])


def _dk_m32c(t, X):
    n = len(X)
    return [kd.dleaf(o.Matern32(t[0], distance=o.L2Distance()), X, X), np.ones((n, n))]  # d(k + c)/dc = 1 everywhere


def _build_ess(mod, t):
    return t[0] * mod.ExpSquared(t[1]) + t[2] * mod.ExpSineSquared(t[3], gamma=t[4])


def _dk_ess(t, X):
    sq, per = o.ExpSquared(t[1]), o.ExpSineSquared(t[3], gamma=t[4])
    return [sq(X, X), t[0] * kd.dleaf(sq, X, X), per(X, X), t[2] * kd.dleaf(per, X, X),
            t[2] * kd.dleaf(per, X, X, "gamma")]


def _build_linear(mod, t):
    if mod is o:  # (the oracle has no transforms module: grad_np.Scaled is k(s * x1, s * x2))
        return t[0] * grad_np.Scaled(t[2:5], o.ExpSquared(t[1], distance=o.L2Distance()))
    from tinygp_amd import transforms

    return t[0] * transforms.Linear(np.array(t[2:5]), mod.ExpSquared(t[1], distance=mod.L2Distance()))


def _dk_linear(t, X):
    """k = A exp(-u), u = sum_q s_q^2 dx_q^2 / (2 l^2) with dx_q = x1_q - x2_q:  dk/dA = k / A,  dk/dl = k r^2 / l^3
    with r^2 = sum_q s_q^2 dx_q^2 (the leaf's closed form on the scaled points), and, u being the only place s_q
    appears,  dk/ds_q = -k du/ds_q = -k s_q dx_q^2 / l^2."""
    amp, ell, s = t[0], t[1], np.asarray(t[2:5], dtype=np.float64)
    leaf = o.ExpSquared(ell, distance=o.L2Distance())
    Xs = X * s
    k0 = leaf(Xs, Xs)
    out = [k0, amp * kd.dleaf(leaf, Xs, Xs)]
    for q in range(3):
        dx = X[:, None, q] - X[None, :, q]
        out.append(-amp * k0 * s[q] * dx * dx / ell**2)
    return out


PROGRAMS = {
    "fast": (1, (1.3, 1.5), _build_fast, _dk_fast),                               # FastEval: two sums in one pass
    "m32c": (3, (1.5, 0.4), _build_m32c, _dk_m32c),                               # GeneralEval family 0; dK/dc = 1
    "ess": (1, (1.3, 1.5, 0.3, 1.2, 0.7), _build_ess, _dk_ess),                   # five parameters, a periodic term
    "linear": (3, (1.5, 1.2, 1.0, 2.0, 1.5), _build_linear, _dk_linear),          # which_op < 0: d / d s_q
}
N_KERNEL = {"fast": 2, "m32c": 2, "ess": 5, "linear": 2}  # len(g["kernel"]); linear's other three are g["transform"]


def sizes(tile_counts):
    """N = 128 nt - 63 and 128 nt for each tile count: a last tile of 65 rows and an exact one.  (One point into the
    last tile is not a case here: a 1 x 128 tile weighs ~1/128 of a full one and falls under the bar; that edge is
    held at N = 129 and 257 by test_gpu_2_kmat_edges.py, where one row is a visible share of the whole.)"""
    return [n for nt in tile_counts for n in (TILE * nt - 63, TILE * nt)]


EVERY_COUNT = tuple(range(1, 18))    # every (nfull, rem) pattern of the halving recursion up to a lone 17th tile
SOME_COUNTS = (1, 2, 3, 6, 11, 16, 17)
# `linear` meets the tile condition only up to three tiles.  Its points are 3-D and unordered, every far tile's sum is
# a few thousand terms of both signs for each of five parameters, and from six tiles on one of them lands under 100
# bars: with the scales (0.5, 2.0, 1.3) already at N = 321 (15 bars), and at N = 768, 1 345 or 2 048 with each of 24
# sets of amplitude 0.7 / 1.5 / 3.0 and scales between 0.5 and 4 that were tried (1.1 ... 88 bars).  The condition is
# not lowered: the program runs at 1, 2 and 3 tiles (lightest tile 5 980 bars) and at 33, where the tail counts.
LINEAR_COUNTS = (1, 2, 3)
FP32_COUNTS = (2, 3, 5)
# (program, n, dtype) of test_gpu_2_grad_tiles.py
GPU_CASES = tuple(
    [(p, n, _F64) for p in ("fast", "m32c") for n in sizes(EVERY_COUNT)]
    + [(p, n, _F64) for p, counts in (("ess", SOME_COUNTS), ("linear", LINEAR_COUNTS)) for n in sizes(counts)]
    + [(p, n, _F64) for p in PROGRAMS for n in sizes((33,))]     # 1 089 partials: sum_partials_kernel's second trip
    + [(p, n, _F32) for p in ("fast", "m32c") for n in sizes(FP32_COUNTS)]
)
# (program, n, nb, GRAD_CHUNK) of test_gpu_5_distributed.py's box cases
BLOCK_COLUMN_CASES = (("ess", 1100, 256, 384), ("ess", 2176, 512, 512))


def kernel(name, mod):
    """The program's kernel from ``tinygp_amd.kernels`` or from the oracle."""
    _, theta, build, _ = PROGRAMS[name]
    return build(mod, theta)


_frozen = dn._frozen


@functools.lru_cache(maxsize=None)
def inputs(n, d, dtype=_F64):
    """``(X, noise diagonal, y)`` in ``dtype``, a function of (n, d) alone: the box points and noise of
    ``_dense_np.train`` (sorted U[0, 4] in 1-D, U[0, 3]^3 in 3-D; noise U[0.05, 0.15]) and
    y = sin(x_0) + 0.3 N(0, 1)."""
    X, diag = dn.train(n, d, dtype)
    x0 = np.asarray(X, dtype=np.float64).reshape(n, -1)[:, 0]
    y = np.sin(x0) + 0.3 * np.random.default_rng([3, n, d]).standard_normal(n)
    return X, diag, _frozen(y.astype(dtype))


def tile_sums(C):
    """Sums of the 128 x 128 tiles of ``C`` (ragged edge tiles as they are): (nt, nt)."""
    idx = np.arange(0, C.shape[0], TILE)
    return np.add.reduceat(np.add.reduceat(C, idx, axis=0), idx, axis=1)


def tile_weights(Kinv, dKs, g, frac):
    """``|sum_{ij in tile} w_ij Kinv_ij dK_p,ij| / (frac max|g|)`` for every parameter p and tile (a, b), a >= b, of the
    lower triangle (w = 1/2 on the diagonal, 1 below it: the weights of kgrad_tile_kernel); NaN above the diagonal."""
    n = Kinv.shape[0]
    nt = -(-n // TILE)
    bar = frac * np.abs(g).max()
    W = np.tril(np.ones((n, n)))
    W[np.diag_indices(n)] = 0.5
    WK = W * Kinv
    table = np.full((len(dKs), nt, nt), np.nan)
    low = np.tril_indices(nt)
    for p, dK in enumerate(dKs):
        table[p][low] = np.abs(tile_sums(WK * dK))[low] / bar
    return table


@functools.lru_cache(maxsize=None)
def reference(name, n, dtype=_F64):
    """The float64 reference at the (dtype-rounded) inputs, conditions asserted.  Returns ``ll``, ``g`` (kernel
    parameters, then the transform's for ``linear``), ``noise`` = 1/2 diag(G), ``alpha``, and the per-tile table
    ``tiles[p, a, b]`` of condition 3 in units of the bar (``min_tile`` its smallest entry; ``tail`` the weight of the
    partials past the first 1 024, or None where there are none)."""
    d, theta, build, derivs = PROGRAMS[name]
    X, diag, y = (np.asarray(a, dtype=np.float64) for a in inputs(n, d, dtype))
    Xp = X.reshape(n, -1)
    K = build(o, theta)(X, X) + np.diag(diag)
    L = sla.cholesky(K, lower=True, check_finite=False)
    Kinv, info = sla.lapack.dpotri(L, lower=1)
    assert info == 0
    Kinv = np.tril(Kinv) + np.tril(Kinv, -1).T
    alpha = sla.cho_solve((L, True), y, check_finite=False)
    ll = -0.5 * float(y @ alpha) - float(np.sum(np.log(np.diag(L)))) - 0.5 * n * math.log(2.0 * math.pi)
    G = np.outer(alpha, alpha) - Kinv
    dKs = derivs(theta, Xp)
    g = np.array([0.5 * np.sum(G * dK) for dK in dKs])
    frac = BARS[dtype]["kernel"]
    bar = frac * np.abs(g).max()

    # 1. the problem is well posed
    ev = sla.eigvalsh(K, check_finite=False)
    cond = float(ev[-1] / ev[0])
    assert ev[0] > 0 and cond <= 1e6, cond
    # 2. a second route to the same numbers: LU instead of Cholesky
    G2 = np.linalg.inv(K)
    a2 = G2 @ y
    G2 = np.outer(a2, a2) - G2
    g2 = np.array([0.5 * np.sum(G2 * dK) for dK in dKs])
    route_gap = float(np.abs(g - g2).max() / np.abs(g).max())
    assert route_gap <= 1e-10, route_gap
    del G2
    # 3. every tile of K^-1 carries weight in every parameter's sum
    nt = -(-n // TILE)
    tiles = tile_weights(Kinv, dKs, g, frac)
    min_tile = float(np.nanmin(tiles))
    if nt * nt <= SECOND_PASS or name in EVERY_TILE_AT_33:
        assert min_tile >= WEIGHT_FACTOR[dtype], (name, n, dtype, min_tile)
    # 4. past 1 024 partials: what the second trip of sum_partials_kernel's loop adds.  A partial is the tile's whole
    # sum, w (alpha alpha^T - K^-1) dK, at index tr * nt + tc (zero above the diagonal)
    tail = None
    if nt * nt > SECOND_PASS:
        W = np.tril(np.ones((n, n)))
        W[np.diag_indices(n)] = 0.5
        late = np.arange(nt * nt).reshape(nt, nt) >= SECOND_PASS
        late &= np.tri(nt, dtype=bool)
        tail = float(min(abs(tile_sums(W * G * dK)[late].sum()) for dK in dKs) / bar)
        assert tail >= WEIGHT_FACTOR[dtype], (name, n, tail)
    return SimpleNamespace(name=name, n=n, nt=nt, dtype=dtype, theta=theta, ll=ll, g=_frozen(g),
                           noise=_frozen(0.5 * np.diag(G)), alpha=_frozen(alpha), tiles=_frozen(tiles),
                           min_tile=min_tile, tail=tail, cond=cond, route_gap=route_gap)


def in_bars(got, want, rtol, frac):
    """``max |got - want| / (rtol |want| + frac max|want|)``: the error in units of the bar that
    ``assert_allclose(got, want, rtol=rtol, atol=frac * max|want|)`` applies; at most 1 passes."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / (rtol * np.abs(want) + frac * np.abs(want).max())))


def errors(ref, ll, kernel_grad, noise_grad, mean_grad):
    """The worst error of each of the device's numbers in units of its bar (to print; ``check`` asserts)."""
    b = BARS[ref.dtype]
    return dict(ll=abs(float(ll) - ref.ll) / (b["ll"] * abs(ref.ll)),
                kernel=in_bars(kernel_grad, ref.g, b["kernel"], b["kernel"]),
                noise=in_bars(noise_grad, ref.noise, b["noise"], b["noise"]),
                mean=in_bars(mean_grad, ref.alpha, b["mean"], b["mean"]))


def check(ref, ll, kernel_grad, noise_grad, mean_grad):
    """The device's numbers against ``ref`` at the project's bars."""
    b = BARS[ref.dtype]
    np.testing.assert_allclose(ll, ref.ll, rtol=b["ll"])
    np.testing.assert_allclose(kernel_grad, ref.g, rtol=b["kernel"], atol=b["kernel"] * np.abs(ref.g).max())
    np.testing.assert_allclose(noise_grad, ref.noise, rtol=b["noise"], atol=b["noise"] * np.abs(ref.noise).max())
    np.testing.assert_allclose(mean_grad, ref.alpha, rtol=b["mean"], atol=b["mean"] * np.abs(ref.alpha).max())
