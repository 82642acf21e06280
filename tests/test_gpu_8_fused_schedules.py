"""GPU: the fused log-likelihood under every schedule of the Cholesky's panel chain.

`DirectSolver.factor_log_probability` (tgp_solver_factor_logprob) is what bench.py times and what every optimiser step
runs: the Cholesky factor, the forward solve z = L^-1 r and the two sums z.z and sum log L_ii in ONE pass -- with the
persistent chain (the default) the solve and the sums are tasks of the chain launches, each block's partial sums added up
by the launch that holds the matrix's last block.  Checked here against an fp64 LAPACK reference of the same operation
(the oracle's kernel matrix, scipy's Cholesky and triangular solve, both sums with math.fsum) under every option set of
test_gpu_0_kernels.py::test_panel_chain_variants_agree, at panels on both sides of the chain launch's limit of 64 block
columns, and across evaluations on one context that switch between such schedules.

The data are well conditioned (ExpSquared with 0.5 on the diagonal: cond(K) < 3e3), so that the fp64 reference itself is
good to ~1e-13 and the device is held to rtol 1e-11 -- far below what a raced block of z or a missing or stale block sum
costs (1e-3 and more) and much tighter than the suite's LL_RTOL = 1e-8.
"""
import contextlib
import functools
import math

import numpy as np
import pytest
import scipy.linalg as sla

from _schedules import PANEL_CHAIN_VARIANTS, option_id
from oracle import tinygp_np as o
from tinygp_amd import _ffi, kernels, noise, synthetic
from tinygp_amd.solvers import DirectSolver

pytestmark = pytest.mark.gpu

RTOL_REF = 1e-11   # fp64 device value against the fp64 LAPACK reference
RTOL_SELF = 1e-12  # fused value against the same solver's separate solve + reduction kernels
FP32_RTOL = 5e-4   # the suite's fp32 tolerance (reference src/tinygp/test_utils.py:15)
DIAG = 0.5
KERNELS = {"k1": (1.5**2, 2.5), "k2": (1.2**2, 1.8)}  # amplitude^2, scale of ExpSquared


def _kernel(mod, which):
    amp, scale = KERNELS[which]
    return amp * mod.ExpSquared(scale)


def _inputs(n, which, dtype=np.float64):
    """Sorted 1-D inputs and residual r1 (sin(x) + noise) or r2 (a different residual on the same inputs)."""
    X, y = synthetic.make_inputs(n, 1)
    if which == "r2":
        y = np.cos(0.7 * X) - 0.3 + 0.2 * np.random.default_rng(7).normal(size=n)
    return X.astype(dtype), y.astype(dtype)


@functools.lru_cache(maxsize=1)
def _reference(n, k, r, dtype=np.float64):
    """(log-likelihood, L) in fp64 on the inputs as the device sees them in `dtype`."""
    X, y = _inputs(n, r, dtype)
    X, y = X.astype(np.float64), y.astype(np.float64)
    K = _kernel(o, k)(X, X)
    K[np.diag_indices(n)] += DIAG
    L = sla.cholesky(K, lower=True, overwrite_a=True, check_finite=False)
    z = sla.solve_triangular(L, y, lower=True, check_finite=False)
    ll = -0.5 * math.fsum(z * z) - math.fsum(np.log(np.diag(L))) - 0.5 * n * math.log(2.0 * math.pi)
    return ll, L


@contextlib.contextmanager
def _options(**opts):
    """Context options on the default context for the block, restored behind it."""
    ctx = _ffi.default_ctx()
    old = {}
    try:
        for key, value in opts.items():
            old[key] = ctx.set_option(key, value)
        yield
    finally:
        for key, value in old.items():
            ctx.set_option(key, value)


def _solver(n, k, r, dtype=np.float64):
    X, y = _inputs(n, r, dtype)
    s = DirectSolver(_kernel(kernels, k), X, noise.Diagonal(np.full(n, DIAG, dtype=dtype)))
    s.set_residual(y)
    return s, y


def _check_fused(s, y, k, want, repeats, rtol=RTOL_REF, rtol_self=RTOL_SELF):
    """`repeats` fused evaluations with the resident residual: bit-identical, against the reference, and against the same
    solver's separate solve on the factor it kept (tgp_solver_logprob: streaming solve + reduction kernels)."""
    vals = [float(s.factor_log_probability(None, _kernel(kernels, k))) for _ in range(repeats)]
    assert s.info == 0
    assert all(v == vals[0] for v in vals), vals
    np.testing.assert_allclose(vals[0], want, rtol=rtol)
    np.testing.assert_allclose(float(s.log_probability(y)), vals[0], rtol=rtol_self)
    return vals[0]


@pytest.mark.parametrize("opts", PANEL_CHAIN_VARIANTS, ids=option_id)
@pytest.mark.parametrize("n", [2560, 5120])
def test_fused_value_under_every_schedule(n, opts):
    """Every option set of the panel chain's schedule (tests/_schedules.py), fp64: the fused value matches LAPACK to 1e-11
    and the solver's own separate solve to 1e-12, three times with the same bits."""
    want, _ = _reference(n, "k1", "r1")
    with _options(**opts):
        s, y = _solver(n, "k1", "r1")
        _check_fused(s, y, "k1", want, 3)


# panels on both sides of the chain launch's limit of 64 block columns (N ragged: the padding is in the last block)
BOUNDARY = [
    (9100, dict(nb_first=8320)),                            # 65 blocks block by block, then a 7-block chain
    (9100, dict(nb_first=8320, chain_merged=0)),
    (9100, dict(nb_first=8320, chain_sub_panel=512)),
    (9100, dict(nb_first=8320, lookahead=0)),
    (9100, dict(nb_first=8192)),                            # 64 blocks: every panel a chain launch
    (9100, dict(nb_first=8064)),
    (12200, dict(nb_outer=8448)),                           # 66 blocks block by block, then a 30-block chain
    (12200, dict(nb_outer=8448, lookahead=0)),
    (12200, dict(nb_outer=8448, chain_fwd_tasks=0)),
    (16800, dict(nb_outer=4224, nb_wide_rows=8000)),        # chain 33, block by block 66, chain 33
    (24526, dict(nb_outer=16384)),                          # 128 blocks block by block, then a 64-block chain
]


@pytest.mark.parametrize("n,opts", BOUNDARY, ids=[f"n{n}-{option_id(o_)}" for n, o_ in BOUNDARY])
def test_fused_value_with_panels_on_both_sides_of_the_chain_limit(n, opts):
    """A panel wider than 64 block columns runs block by block; the forward substitution and the sums of the whole
    evaluation then stay off the chain launches (one decision per evaluation, chol.hip potrf).  fp64: the fused value
    against LAPACK (1e-11) and against the separate solve (1e-12), five bit-identical repeats, and the factor it kept."""
    want, L = _reference(n, "k1", "r1")
    with _options(**opts):
        s, y = _solver(n, "k1", "r1")
        _check_fused(s, y, "k1", want, 5)
        got = s.scale_tril  # (the factor of the last fused evaluation)
    tol = 1e-11 * np.abs(np.diag(L)).max()  # (|L_ij| <= max_i sqrt(K_ii) = max |L_ii|)
    for j0 in range(0, n, 2048):  # (column blocks: one temporary of 2 048 columns, not of the whole matrix)
        err = np.abs(got[:, j0:j0 + 2048] - L[:, j0:j0 + 2048]).max()
        assert err <= tol, (j0, err, tol)


def test_partial_sums_of_an_earlier_evaluation_are_not_read():
    """One context, three evaluations: the default schedule (every panel a chain launch: each block's partial sums are
    written), then panels on both sides of the limit with another kernel and residual (no chain launch may add up the
    slots the first evaluation left), then the default schedule again.  Each value matches its own reference."""
    n = 9100
    want1, _ = _reference(n, "k1", "r1")
    want2, _ = _reference(n, "k2", "r2")
    _, r2 = _inputs(n, "r2")
    s, r1 = _solver(n, "k1", "r1")
    v1 = float(s.factor_log_probability(r1, _kernel(kernels, "k1")))
    with _options(nb_first=8320):
        v2 = float(s.factor_log_probability(r2, _kernel(kernels, "k2")))
    v3 = float(s.factor_log_probability(r1, _kernel(kernels, "k1")))
    np.testing.assert_allclose(v1, want1, rtol=RTOL_REF)
    np.testing.assert_allclose(v2, want2, rtol=RTOL_REF)
    assert v3 == v1
    with _options(nb_first=8320):  # ... and the other way round
        v4 = float(s.factor_log_probability(r1, _kernel(kernels, "k1")))
    v5 = float(s.factor_log_probability(r2, _kernel(kernels, "k2")))
    np.testing.assert_allclose(v4, want1, rtol=RTOL_REF)
    np.testing.assert_allclose(v5, want2, rtol=RTOL_REF)


@pytest.mark.parametrize("n,opts", [(5120, {}), (5120, dict(chain_kernel=0, fused_step=1)), (9100, dict(nb_first=8320))],
                         ids=["n5120-defaults", "n5120-chain_kernel0-fused_step1", "n9100-nb_first8320"])
def test_fused_value_fp32(n, opts):
    """fp32 inputs, the default chain, the launch-per-block path and panels on both sides of the limit: against the fp64
    reference of the same (fp32-rounded) inputs at the suite's fp32 tolerance."""
    want, _ = _reference(n, "k1", "r1", np.float32)
    with _options(**opts):
        s, y = _solver(n, "k1", "r1", np.float32)
        _check_fused(s, y, "k1", want, 3, rtol=FP32_RTOL, rtol_self=5e-5)
