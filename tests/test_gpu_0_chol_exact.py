"""GPU: the Cholesky (chol.hip) and what rides on it, held to a factor known in advance with every tile weighted.

The inputs are tests/_chol_exact.py's: K = L0 L0^T from an integer L0.  Family X (128 x 128 diagonal blocks p I, p a power
of two) must come back as L0 bit for bit under EVERY schedule, in fp64 and fp32: every pivot is p^2, fast_rsqrt / fast_rcp
of a power of two are exact (the FMA residual is zero at the exact value and the refinement lands on it), every scaled entry
is (p l) 2^-k = l and every Schur complement an integer sum, exact in any order, split along k or not.  Family D (dense
diagonal blocks) exercises potf2's eliminations, the 16 x 16 inverses and the in-panel solves and is held to 2^-20 -- 256
times below the effect of one wrong product.  Unlike the kernel-matrix inputs of test_gpu_0_kernels.py and
test_gpu_8_fused_schedules.py, whose factor decays below those tests' bars a dozen tiles from the diagonal, a dropped,
doubled or mis-fed tile update anywhere in these matrices fails the case and is named by its tile
(tests/test_chol_exact_cpu.py shows both).

The fused value, the factor it keeps and the solves go through DirectSolver(..., covariance=K): the kernel is not evaluated.
"""
import numpy as np
import pytest

import _chol_exact as cx
import _lowlevel as ll
from _schedules import PANEL_CHAIN_VARIANTS, option_id
from test_gpu_8_fused_schedules import BOUNDARY, RTOL_REF, _options
from tinygp_amd import kernels, noise
from tinygp_amd.solvers import DirectSolver

pytestmark = pytest.mark.gpu

SCHEDULES = [{}] + PANEL_CHAIN_VARIANTS
SPLIT_TAIL = [dict(split_tail=1, chain_reserve=0), dict(chain_kernel=0, split_tail=1, sub_panel=512), dict(chain_full_rows=0),
              dict(chain_kernel=0)]  # test_split_tail_and_two_level_at_n6144_deterministic
DENSE = [{}, dict(chain_kernel=0), dict(chain_kernel=0, fused_step=1), dict(chain_full_rows=0)]
FP32 = [(1536, dict(chain_kernel=0, fused_step=1)), (1536, dict(chain_kernel=1)), (1536, dict(chain_kernel=1, chain_full_rows=0)),
        (1024, {})]  # test_panel_step_fp32_and_bad_pivot, test_potrf_fp32
FUSED = [{}, dict(chain_kernel=0, fused_step=1), dict(lookahead=0), dict(chain_fwd_tasks=0),
         dict(chain_batch=4, chain_batch_minrows=0)]
CHAIN_LIMIT = [o for n, o in BOUNDARY if n == 9100]


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _exact_twice(n, dtype, opts):
    L0 = cx.factor(n, "X", dtype)
    K = cx.matrix(L0)
    L, info = ll.potrf(K, **opts)
    assert info == 0
    cx.check_exact(L, L0)
    L2, info2 = ll.potrf(K, **opts)
    assert info2 == 0 and np.array_equal(_bits(L), _bits(L2)), opts


@pytest.mark.parametrize("opts", SCHEDULES, ids=option_id)
@pytest.mark.parametrize("n", [1152, 2560, 5120])
def test_family_x_is_exact_under_every_schedule(n, opts):
    """tgp_potrf on family X, fp64, under the defaults and every option set of the panel chain: L0 to the bit, twice."""
    _exact_twice(n, np.float64, opts)


@pytest.mark.parametrize("opts", SPLIT_TAIL, ids=option_id)
def test_family_x_is_exact_with_the_last_round_cut_along_k(opts):
    """N = 6 144: the trailing updates have several rounds of tiles and the split tail cuts the last one along k."""
    _exact_twice(6144, np.float64, opts)


@pytest.mark.parametrize("opts", DENSE, ids=option_id)
@pytest.mark.parametrize("n", [1152, 2560, 5120])
def test_family_d_within_two_to_the_minus_twenty(n, opts):
    """Dense diagonal blocks: |L - L0| <= 2^-20 (tests/_chol_exact.py BAR_D: from the construction), and every variant agrees
    with the default schedule's factor at the bar of test_panel_chain_variants_agree."""
    L0 = cx.factor(n, "D")
    K = cx.matrix(L0)
    L, info = ll.potrf(K, **opts)
    assert info == 0
    print(f"\n[family D n={n} {option_id(opts)}] max |L - L0| = {cx.worst(L, L0):.3e}")
    cx.check_close(L, L0, cx.BAR_D)
    if opts:
        Ldef, info0 = ll.potrf(K)
        assert info0 == 0
        np.testing.assert_allclose(L, Ldef, rtol=0, atol=1e-12 * np.abs(Ldef).max())


@pytest.mark.parametrize("n,opts", FP32, ids=[f"n{n}-{option_id(o)}" for n, o in FP32])
def test_family_x_is_exact_in_fp32(n, opts):
    _exact_twice(n, np.float32, opts)


@pytest.mark.parametrize("nb_outer", [128, 256, 512, 1024])
def test_family_x_is_exact_at_every_block_size(nb_outer):
    _exact_twice(1536, np.float64, dict(nb_outer=nb_outer))


def _solver(n):
    """(solver on K through the covariance channel, L0, w, r = L0 w).  The kernel only has to lower: it is not evaluated."""
    L0 = cx.factor(n, "X")
    w, r = cx.rhs(L0)
    s = DirectSolver(kernels.ExpSquared(1.0), np.arange(n, dtype=np.float64), noise.Diagonal(np.zeros(n)),
                     covariance=cx.matrix(L0))
    return s, L0, w, r


def _check_value(s, L0, w, r):
    """The fused value: three repeats with the same bits, against -w.w / 2 - N log p - N / 2 log 2 pi (only the order of the
    N equal log p terms is inexact; a lost 128-block of z costs ~3e-3)."""
    vals = [float(s.factor_log_probability(r)) for _ in range(3)]
    assert s.info == 0
    assert all(v == vals[0] for v in vals), vals
    np.testing.assert_allclose(vals[0], cx.loglik(L0, w), rtol=RTOL_REF)
    np.testing.assert_allclose(float(s.normalization()), cx.normalization(L0), rtol=RTOL_REF)


@pytest.mark.parametrize("opts", FUSED, ids=option_id)
@pytest.mark.parametrize("n", [1100, 2561, 5120])
def test_fused_value_factor_and_solves_are_exact(n, opts):
    """factor_log_probability, the factor it keeps and both triangular solves on family X, ragged N included: scale_tril is
    L0, L0^-1 (L0 w) and L0^-T (L0^T w) are w, entry for entry (integer sums times the exact inverse 1 / p)."""
    with _options(**opts):
        s, L0, w, r = _solver(n)
        try:
            _check_value(s, L0, w, r)
            cx.check_exact(s.scale_tril, L0)
            rt = np.asarray(L0).T @ w  # (integers up to 3 (p + a N): exact)
            for mode in (1, 0):
                with _options(stream_trsv=mode):
                    z = s.solve_triangular(r)
                    zt = s.solve_triangular(rt, transpose=True)
                assert np.array_equal(z, w), (mode, int((z != w).sum()), int(np.argmax(z != w)))
                assert np.array_equal(zt, w), (mode, int((zt != w).sum()), int(np.argmax(zt != w)))
        finally:
            s.close()


@pytest.mark.parametrize("opts", CHAIN_LIMIT, ids=option_id)
def test_family_x_with_panels_on_both_sides_of_the_chain_limit(opts):
    """N = 9 100 under the N = 9 100 option sets of test_gpu_8_fused_schedules.py::BOUNDARY (panels of 65, 64 and 63 block
    columns in front of a chain): the factor exactly, in column blocks of 2 048, and the fused value."""
    n = 9100
    with _options(**opts):
        s, L0, w, r = _solver(n)
        try:
            _check_value(s, L0, w, r)
            got = s.scale_tril
            for j0 in range(0, n, 2048):
                cx.check_exact(got[:, j0:j0 + 2048], L0, col0=j0)
        finally:
            s.close()
