"""GPU: where the dense Cholesky reports a failed pivot, and what the solver returns behind it.

`info` is written by the first potf2 workgroup that meets a pivot which is not > 0 (potf2_body.inc: one compare-and-swap
on `info` with pivot_base + k0 + bad), and pivot_base comes from a different host expression at every launch site of
chol.hip (launch_potf2, panel_potf2, launch_panel_step, launch_chain and the chain's own q.pivot_base + c * TILE, the
sub-panel forms, the block-column driver's pivot_off).  The factorisation then runs to its end on NaNs, through every
hand-off, the fused forward solve and the chain's partial sums.  Here a failure is planted at the first and the last
column of every 16-column step, tile, sub-panel, panel and chain launch, under every option set of tests/_schedules.py
and on both sides of the 64-block chain limit, through the unfused and the fused route, and `info` must be p + 1:
an integer that follows from the construction of the inputs (tests/_dense_failure.py, proved on the host by
tests/test_dense_failure_cpu.py), so the comparison is exact.  A failure is a result: nothing raises, no pass is
repeated (the context's `timeout_retries` does not move), and the same handle gives a fresh solver's bits afterwards.
"""
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import _dense_failure as df
import _lowlevel as ll
from _schedules import PANEL_CHAIN_VARIANTS, option_id
from test_gpu_8_fused_schedules import _options
from tinygp_amd import GaussianProcess, _ffi, kernels, noise
from tinygp_amd.solvers import DirectSolver

pytestmark = pytest.mark.gpu


# ---- 1. the raw factor ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clean(n, dtype, diag):
    K = df.spd(n, dtype, diag)
    L = sla.cholesky(K.astype(np.float64), lower=True)
    K.setflags(write=False), L.setflags(write=False)
    return K, L


@pytest.mark.parametrize("n,dtype,diag", [(128, np.float64, 0.05), (256, np.float64, 0.05), (640, np.float64, 0.05),
                                          (640, np.float32, 0.5)], ids=["n128", "n256", "n640", "n640-fp32"])
def test_raw_factor_reports_the_pivot_and_keeps_the_leading_block(n, dtype, diag):
    """tgp_potrf on a matrix with K[p, p] = -1, K[p, p] = NaN, row and column p NaN, or one NaN pair (p, q) with q in
    p's 16-column step, in an earlier step of p's tile, in the tile before: info = p + 1, L[p, p] is not finite, and
    the leading block L[:p, :p] is LAPACK's factor of K[:p, :p] (the first p columns of the factor of the clean
    matrix) to 1e-11 max|L| in fp64 and to 5e-4 in fp32.  The pair keeps to row p because every product of the
    factorisation keeps rows apart."""
    K0, Lref = _clean(n, dtype, diag)
    for p in df.raw_positions(n):
        want = Lref[:p, :p]
        for form in df.RAW_FORMS:
            K = df.plant(K0, p, form)
            if K is None:
                continue
            L, info = ll.potrf(K)
            assert info == p + 1, (p, form, info)
            lead = L[:p, :p]
            assert np.all(np.isfinite(lead)), (p, form)
            if dtype == np.float64:
                np.testing.assert_allclose(lead, want, rtol=0, atol=1e-11 * np.abs(want).max(initial=0.0),
                                           err_msg=f"{p} {form}")
            else:
                np.testing.assert_allclose(lead, want, rtol=5e-4, atol=5e-4, err_msg=f"{p} {form}")
            assert not np.isfinite(L[p, p]), (p, form, L[p, p])


# ---- the two routes of a solver ------------------------------------------------------------------------------------
def _both_routes(n, ps, want, dtype=np.float64, repeats=1):
    """A solver whose noise has the bad entries `ps`: the unfused refactor() and the fused evaluation on the resident
    residual both report `want`, `repeats` times over; the fused value is not finite, log_probability is -inf, and no
    pass was repeated behind a timeout."""
    ctx = _ffi.default_ctx()
    retries = ctx.get_option("timeout_retries")
    X, y = df.inputs(n, dtype)
    s = DirectSolver(df.kernel(kernels), X, noise.Diagonal(df.bad_noise(n, ps, dtype)))
    try:
        for _ in range(repeats):
            assert s.refactor() == want, (ps, "unfused")
            assert s.info == want
        assert s.log_probability(y) == -np.inf
        s.set_residual(y)
        for _ in range(repeats):
            v = s.factor_log_probability(None, df.kernel(kernels))
            assert s.info == want, (ps, "fused", s.info)
            assert not np.isfinite(v), (ps, v)
        assert s.log_probability(y) == -np.inf
    finally:
        s.close()
    assert ctx.get_option("timeout_retries") == retries, ps


# ---- 2. every schedule ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", PANEL_CHAIN_VARIANTS, ids=option_id)
def test_pivot_position_under_every_schedule(opts):
    """N = 2 560, fp64, every option set of the panel chain: a bad noise entry at the first and last column of every
    step, tile, sub-panel and panel width and of the one-launch tail that the option sets name, and at both ends."""
    three_times = df.SCHEDULE_POSITIONS[PANEL_CHAIN_VARIANTS.index(opts) % len(df.SCHEDULE_POSITIONS)]
    with _options(**opts):
        for p in df.SCHEDULE_POSITIONS:
            _both_routes(df.SCHEDULE_N, p, p + 1, repeats=3 if p == three_times else 1)


# ---- 3. both sides of the chain limit ------------------------------------------------------------------------------
@pytest.mark.parametrize("n,opts", df.BOUNDARY_CASES, ids=[f"n{n}-{option_id(o_)}" for n, o_ in df.BOUNDARY_CASES])
def test_pivot_position_with_panels_on_both_sides_of_the_chain_limit(n, opts):
    """A panel of more than 64 block columns runs block by block, the next one as a chain launch: the last column
    below and the first at and above the panel width, both sides of column 8 192, and the last real row in front of
    the padding (N is ragged)."""
    with _options(**opts):
        for p in df.edges(n, opts, above=True):
            _both_routes(n, p, p + 1)


# ---- 4. ragged sizes and the padded tile ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", df.RAGGED_SIZES)
def test_pivot_position_at_ragged_sizes(n):
    """The last tile is padded with an identity block: a failure in the last real row is that row, never a padding row."""
    for p in df.ragged_positions(n):
        _both_routes(n, p, p + 1)


# ---- 5. fp32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", df.FP32_SCHEDULES, ids=option_id)
def test_pivot_position_fp32(opts):
    with _options(**opts):
        for p in df.FP32_POSITIONS:
            _both_routes(df.FP32_N, p, p + 1, dtype=np.float32)


# ---- 6. the first of two -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", df.PAIR_SCHEDULES, ids=option_id)
@pytest.mark.parametrize("where", list(df.PAIRS))
def test_the_first_of_two_bad_pivots_is_reported(where, opts):
    """The compare-and-swap of the second failing workgroup must lose: two bad pivots in one 16-column step, one tile,
    two tiles of a panel, two panels, and on the two sides of a chain launch -- the smaller index, five times."""
    n, extra, p1, p2 = df.PAIRS[where]
    with _options(**extra, **opts):
        _both_routes(n, [p2, p1], p1 + 1, repeats=5)


# ---- 7. what the caller sees ---------------------------------------------------------------------------------------
def _caller_sees_a_failure(gp, y, p):
    n = len(y)
    xt = np.linspace(0.0, n / 100.0, 23)
    assert gp.log_probability(y) == -np.inf  # (the first use: the fused pass)
    assert gp.solver.info == p + 1
    assert gp.solver.refactor() == p + 1
    assert gp.log_probability(y) == -np.inf
    value, grads = gp.log_probability_and_grad(y)
    assert value == -np.inf
    assert len(grads["kernel"]) > 0 and np.all(np.isnan(grads["kernel"]))
    assert grads["noise_diag"].shape == (n,) and np.all(np.isnan(grads["noise_diag"]))
    assert grads["mean"].shape == (n,) and np.all(np.isnan(grads["mean"]))
    cond = gp.condition(y, xt)
    assert cond.log_probability == -np.inf
    assert np.all(np.isnan(cond.gp.loc)) and np.all(np.isnan(cond.gp.variance)) and np.all(np.isnan(cond.gp.covariance))
    mean, var = gp.predict(y, xt, return_var=True)
    assert mean.shape == var.shape == (23,) and np.all(np.isnan(mean)) and np.all(np.isnan(var))
    assert np.all(np.isnan(gp.predict(y)))
    assert np.all(np.isnan(gp.solver.solve_triangular(y))) and np.isnan(gp.solver.normalization())
    assert np.all(np.isnan(gp.solver.scale_tril))


@pytest.mark.parametrize("how", ["noise", "nan_coordinate", "covariance_nan_row"])
def test_what_the_caller_sees(how):
    """GaussianProcess at N = 640 with the failure in the third tile -- a bad noise entry, X[p] = NaN through the
    device's own assembly (row and column p of K are NaN), covariance= with row and column p NaN: -inf, NaN gradients,
    NaN predictions, nothing raises (reference gp.py:316)."""
    n, p = df.CALLER_N, df.CALLER_P
    X, y = df.inputs(n)
    k = df.kernel(kernels)
    if how == "noise":
        gp = GaussianProcess(k, X, noise=noise.Diagonal(df.bad_noise(n, p)))
    elif how == "nan_coordinate":
        X = X.copy()
        X[p] = np.nan
        gp = GaussianProcess(k, X, diag=df.DIAG)
    else:
        gp = GaussianProcess(k, X, diag=df.DIAG, covariance_value=df.plant(df.noise_matrix(n, []), p, "nan_row"))
    retries = _ffi.default_ctx().get_option("timeout_retries")
    _caller_sees_a_failure(gp, y, p)
    assert _ffi.default_ctx().get_option("timeout_retries") == retries
    gp.solver.close()


# ---- 8. the handle after a failure ---------------------------------------------------------------------------------
def _everything(s, y, Y, xt):
    return [np.asarray(s.log_probability(y)), s.solve_triangular(Y), s.solve_triangular(Y, transpose=True),
            s.solve_triangular(y), s.condition_variance(df.kernel(kernels), xt),
            np.asarray(s.factor_log_probability(y)), np.asarray(s.info), np.asarray(s.log_probability(y))]


@pytest.mark.parametrize("opts", df.HANDLE_SCHEDULES, ids=option_id)
@pytest.mark.parametrize("how", ["covariance", "kernel", "fused"])
@pytest.mark.parametrize("n,p", df.HANDLE_CASES)
def test_one_handle_good_failed_good(n, p, how, opts):
    """One DirectSolver: a good factorisation, a failed one -- refactor(covariance=) with a bad pivot at p (and the
    fused pass on that resident matrix), refactor(kernel=) with a negative amplitude (info = 1), the fused call with
    that kernel -- and the good one again: log_probability, factor_log_probability, both triangular solves and the
    conditional variance then have the bits of a solver that never failed, and info is 0."""
    X, y = df.inputs(n)
    Y = np.random.default_rng(n).normal(size=(n, 3))
    xt = np.linspace(X[0], X[-1], 37)
    good, negative = df.kernel(kernels), -1.0 * df.kernel(kernels)
    clean = noise.Diagonal(np.full(n, df.DIAG))
    ctx = _ffi.default_ctx()
    retries = ctx.get_option("timeout_retries")
    with _options(**opts):
        fresh = DirectSolver(good, X, clean)
        assert fresh.refactor() == 0
        want = _everything(fresh, y, Y, xt)
        fresh.close()
        assert all(np.all(np.isfinite(w)) for w in want)

        s = DirectSolver(good, X, clean)
        assert s.refactor() == 0
        if how == "covariance":
            assert s.refactor(covariance=df.noise_matrix(n, p)) == p + 1
            assert not np.isfinite(s.factor_log_probability(y)) and s.info == p + 1
        elif how == "kernel":
            assert s.refactor(kernel=negative) == 1
        else:
            assert not np.isfinite(s.factor_log_probability(y, negative)) and s.info == 1
        assert s.log_probability(y) == -np.inf
        assert np.all(np.isnan(s.solve_triangular(Y))) and np.all(np.isnan(s.solve_triangular(Y, transpose=True)))
        assert np.all(np.isnan(s.condition_variance(good, xt)))
        assert s.refactor(kernel=good) == 0
        got = _everything(s, y, Y, xt)
        s.close()
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert ctx.get_option("timeout_retries") == retries
