"""tests/_chol_exact.py on the CPU: the families are exact by construction (K is the int64 product, LAPACK returns L0 with
error 0, every tile of L0 carries weight), the checks reject a single dropped, doubled or mis-fed tile update wherever it
sits -- and the kernel-matrix inputs of the older factor tests let the same mutation through."""
import numpy as np
import pytest
import scipy.linalg as sla

import _cases
import _chol_exact as cx
from oracle import tinygp_np as o

B = cx.TILE
FAMILIES = [("X", np.float64), ("D", np.float64), ("X", np.float32)]
SIZES_CPU = (640, 2560, 5120)
# every N of test_gpu_0_chol_exact.py and of the block-column test in test_gpu_5_distributed.py
SIZES_GPU = {
    ("X", np.float64): (1100, 1152, 1536, 1900, 2000, 2560, 2561, 5120, 6144, 9100),
    ("D", np.float64): (1152, 2560, 5120),
    ("X", np.float32): (1024, 1536),
}
KINDS = ("dropped", "doubled", "neighbour")


def blocked_cholesky(K, mutation=None):
    """Right-looking Cholesky over 128-tiles in NumPy / LAPACK.  mutation = (kind, (i, j, k)) spoils ONE tile update
    A_ij -= L_ik L_jk^T (i >= j > k): "dropped", "doubled", or "neighbour" (fed L_(i-1)k in place of L_ik)."""
    n = K.shape[0]
    assert n % B == 0
    T = n // B
    A = np.array(K, dtype=K.dtype, order="C")
    kind, (mi, mj, mk) = mutation if mutation else (None, (-1, -1, -1))
    assert mutation is None or (kind in KINDS and T > mi >= mj > mk >= 0)

    def t(i):
        return slice(i * B, (i + 1) * B)

    for k in range(T):
        Lkk = sla.cholesky(A[t(k), t(k)], lower=True, check_finite=False)
        A[t(k), t(k)] = Lkk
        if k + 1 < T:
            A[(k + 1) * B:, t(k)] = sla.solve_triangular(Lkk, A[(k + 1) * B:, t(k)].T, lower=True, check_finite=False).T
        if k != mk:  # (one product for the whole trailing matrix; the upper half is scratch)
            A[(k + 1) * B:, (k + 1) * B:] -= A[(k + 1) * B:, t(k)] @ A[(k + 1) * B:, t(k)].T
            continue
        for j in range(k + 1, T):
            if j != mj:
                A[j * B:, t(j)] -= A[j * B:, t(k)] @ A[t(j), t(k)].T
                continue
            for i in range(j, T):
                rows = t(i)
                if i == mi:
                    if kind == "dropped":
                        continue
                    if kind == "neighbour":
                        rows = t(i - 1)
                A[t(i), t(j)] -= A[rows, t(k)] @ A[t(j), t(k)].T
                if i == mi and kind == "doubled":
                    A[t(i), t(j)] -= A[rows, t(k)] @ A[t(j), t(k)].T
    return np.tril(A)


def triples(T):
    """The far corner and one mid-matrix update."""
    return [(T - 1, T - 2, 0), (T // 2 + 1, T // 2 - 1, T // 4)]


@pytest.mark.parametrize("family,dtype", FAMILIES, ids=["X-f64", "D-f64", "X-f32"])
def test_magnitudes_keep_every_sum_exact(family, dtype):
    """p^2 + 2 a p + a^2 N < 2^53 / 2^24 for every N the GPU tests use, and the entries of K and r respect it."""
    name = cx._name(dtype)
    p, a = cx.PARAMS[name]
    assert p & (p - 1) == 0
    for n in SIZES_CPU + SIZES_GPU[(family, dtype)]:
        bound, limit = cx.bounds(n, dtype)
        assert bound == p * p + 2 * a * p + a * a * n and bound < limit, (n, bound, limit)
        assert 3 * (p + a * n) < limit  # (the right-hand side r = L0 w)
    for n in (640, 1100, 2560):
        L0 = cx.factor(n, family, dtype)
        K = cx.matrix(L0)
        assert K.dtype == dtype and L0.dtype == dtype
        assert np.abs(K).max() <= cx.bounds(n, dtype)[0]
        assert np.array_equal(np.diag(L0), np.full(n, p)) and np.abs(np.tril(L0, -1)).max() == a
        assert np.all(np.triu(L0, 1) == 0)
        if family == "X":
            for j0 in range(0, n, B):
                blk = np.asarray(L0[j0:j0 + B, j0:j0 + B])
                assert np.array_equal(blk, p * np.eye(blk.shape[0]))
        w, r = cx.rhs(L0)
        assert np.abs(w).max() == 3 and r.dtype == dtype
        assert np.array_equal(r.astype(np.int64), np.asarray(L0).astype(np.int64) @ w.astype(np.int64))


@pytest.mark.parametrize("family,dtype", FAMILIES, ids=["X-f64", "D-f64", "X-f32"])
@pytest.mark.parametrize("n", SIZES_CPU)
def test_matrix_is_the_int64_product_and_lapack_returns_the_factor(n, family, dtype):
    """One BLAS product gives K = L0 L0^T exactly; LAPACK potrf returns L0 with error exactly 0; cond(L0) ~ 1; every
    off-diagonal tile of L0 weighs in."""
    L0 = cx.factor(n, family, dtype)
    K = cx.matrix(L0)
    assert cx.matrix(L0) is K  # (cached)
    Li = np.asarray(L0).astype(np.int64)
    if n == 640:
        assert np.array_equal(K.astype(np.int64), Li @ Li.T)
    else:  # (int64 matmul has no BLAS: column samples at the larger sizes)
        cols = np.random.default_rng(n).choice(n, size=16, replace=False)
        assert np.array_equal(K[:, cols].astype(np.int64), Li @ Li[cols].T)
    assert np.array_equal(K, K.T)
    L = sla.cholesky(K, lower=True, check_finite=False)
    assert L.dtype == dtype
    cx.check_exact(L, L0)
    assert cx.worst(L, L0) == 0.0
    if n == 640:
        cond = np.linalg.cond(np.asarray(L0).astype(np.float64))
        assert cond < (1.1 if dtype == np.float64 else 2.0), cond  # (p = 4096: 1.03; p = 64: 1.8)
    T = n // B
    sums = np.abs(np.asarray(L0)).reshape(T, B, T, B).sum(axis=(1, 3))
    low = sums[np.tril_indices(T, -1)]
    a = cx.PARAMS[cx._name(dtype)][1]
    assert low.min() > (19000 if a == 2 else 10000), low.min()  # (E = 19 661 with a = 2, 10 923 with a = 1)


def test_ragged_sizes_and_the_cache():
    L0 = cx.factor(1100, "X")
    assert L0.shape == (1100, 1100) and not L0.flags.writeable
    assert np.array_equal(cx.factor(1100, "X"), L0) and not np.array_equal(cx.factor(1100, "X", seed=1), L0)
    K = cx.matrix(L0)
    cx.check_exact(sla.cholesky(K, lower=True), L0)
    assert cx.matrix(cx.factor(1100, "X")) is K          # the same key
    K2 = cx.matrix(cx.factor(640, "X"))
    assert cx.matrix(cx.factor(1100, "X")) is not K and K2.shape == (640, 640)  # one entry
    with pytest.raises(ValueError):
        cx.factor(256, "D", np.float32)
    w, _ = cx.rhs(L0)
    want = -0.5 * float(w @ w) - 1100 * np.log(4096.0) - 550 * np.log(2 * np.pi)
    np.testing.assert_allclose(cx.loglik(L0, w), want, rtol=1e-14)
    np.testing.assert_allclose(cx.normalization(L0), 1100 * np.log(4096.0) + 550 * np.log(2 * np.pi), rtol=1e-14)


def test_the_report_names_tile_count_deviation_and_upper_entries():
    L0 = cx.factor(1100, "X")
    got = np.array(L0)
    cx.check_exact(got, L0)
    cx.check_exact(got[:, 256:512], L0, col0=256)
    got[700, 300] += 0.25
    got[701, 301] += 0.5
    got[1099, 1050] = np.nan
    got[3, 900] = 1e-300
    with pytest.raises(AssertionError) as e:
        cx.check_exact(got, L0)
    msg = str(e.value)
    assert "first wrong 128x128 tile (i, j) = (5, 2) with 2 of 16384 entries wrong, largest deviation 5.000e-01" in msg
    assert "2 tile(s) wrong in all" in msg
    assert "non-zero above the diagonal: first wrong 128x128 tile (i, j) = (0, 7) with 1 of" in msg
    with pytest.raises(AssertionError, match=r"tile \(i, j\) = \(5, 2\) with 2 of"):
        cx.check_exact(got[:, 256:512], L0, col0=256)
    with pytest.raises(AssertionError, match=r"tile \(i, j\) = \(8, 8\) with 1 of 5776 entries wrong, no finite deviation, 1 not"):
        cx.check_close(got[:, 1024:], L0, 1.0, col0=1024)
    ok = np.array(L0)
    ok[700, 300] += cx.BAR_D
    cx.check_close(ok, L0, cx.BAR_D)
    ok[700, 300] += cx.BAR_D
    with pytest.raises(AssertionError, match=r"\(5, 2\) with 1 of"):
        cx.check_close(ok, L0, cx.BAR_D)
    neg = np.array(L0)
    neg[0, 5] = -0.0  # a signed zero is a zero
    cx.check_exact(neg, L0)


@pytest.mark.parametrize("family,dtype", FAMILIES, ids=["X-f64", "D-f64", "X-f32"])
def test_every_mutation_of_one_tile_update_is_caught(family, dtype):
    """The blocked factorisation run correctly returns L0 bit for bit; with one update (i, j, k) dropped, doubled or fed
    the k-tile of the neighbouring row -- at the far corner and mid-matrix -- it fails check_exact, and check_close at 2^-20,
    with (i, j) named as the first wrong tile."""
    n = 1536
    L0 = cx.factor(n, family, dtype)
    K = cx.matrix(L0)
    cx.check_exact(blocked_cholesky(K), L0)
    p = cx.PARAMS[cx._name(dtype)][0]
    for trip in triples(n // B):
        for kind in KINDS:
            L = blocked_cholesky(K, (kind, trip))
            where = rf"first wrong 128x128 tile \(i, j\) = \({trip[0]}, {trip[1]}\)"
            with pytest.raises(AssertionError, match=where):
                cx.check_exact(L, L0)
            with pytest.raises(AssertionError, match=where):
                cx.check_close(L, L0, cx.BAR_D)
            tile = (L - np.asarray(L0))[trip[0] * B:(trip[0] + 1) * B, trip[1] * B:(trip[1] + 1) * B]
            assert np.abs(tile).max() >= 1.0 / p  # (one wrong product moves an entry by at least 1 / p)


def _spd(n, seed, cond_diag):
    """The inputs of test_gpu_0_kernels.py::_spd."""
    X, _ = _cases.synthetic.make_inputs(n, 1, seed=_cases.synthetic.SEED + seed)
    return (1.5**2 * o.ExpSquared(2.5))(X, X) + cond_diag * np.eye(n)


def test_the_kernel_matrix_inputs_miss_the_same_mutations():
    """Why the families exist.  On the sorted 1-D ExpSquared(2.5) inputs of test_panel_chain_variants_agree (N = 2 560,
    seed 3, diagonal 0.05) and at its bar of 1e-11 max |L|, the far-corner update can be dropped, doubled or fed the wrong
    k-tile and the factor still passes; the figures of every mutation are printed."""
    n = 2560
    K = _spd(n, 3, 0.05)
    Lref = sla.cholesky(K, lower=True)
    bar = 1e-11 * np.abs(Lref).max()
    assert np.abs(blocked_cholesky(K) - Lref).max() <= bar
    far, mid = triples(n // B)
    for trip in (far, mid):
        for kind in KINDS:
            try:
                err = np.abs(blocked_cholesky(K, (kind, trip)) - Lref).max()
            except sla.LinAlgError:  # (a mid-matrix mutation may cost positive definiteness: caught, loudly)
                err = np.inf
            print(f"[spd n={n}] {kind} {trip}: max |L - Lref| = {err:.3e} (bar {bar:.3e})")
            if trip == far:
                assert err <= bar, (kind, trip, err, bar)
