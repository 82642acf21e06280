"""The posterior half of the dense ``DirectSolver`` past one 128 x 128 tile: multi-RHS ``dot_triangular`` (the
per-column trmv route and the MFMA TRMM route), multi-RHS ``solve_triangular`` in both directions and both
``stream_trsv`` modes, the full M x M conditional covariance (SYRK-shaped product + mirror pass) beside
``condition_variance``, one handle across calls of every kind, and a failed factorisation.

Inputs, references and bars come from ``_dense_np.py`` (its input conditions are asserted when a reference is built;
``test_dense_shapes_cpu.py`` runs them without a GPU).  The products and solves are compared on the device's OWN
factor, which isolates them from the factorisation; the conditional covariance against float64 LAPACK end to end.

Largest errors seen on an MI355X at these shapes, as a fraction of each bar, are recorded in DESIGN.md ("Parity of
the dense posterior path past one tile"); every test prints its own figure before it asserts.
"""
import ctypes as C

import numpy as np
import pytest
from scipy.linalg import lapack

import _dense_np as dn
import _lowlevel as ll
from oracle import tinygp_np as o
from tinygp_amd import GaussianProcess, _ffi, kernels, noise
from tinygp_amd.solvers import DirectSolver

pytestmark = pytest.mark.gpu

F64, F32 = "float64", "float32"
N_DTYPE = [(n, F64) for n in dn.NS] + [(n, F32) for n in dn.FP32_NS]


def _new_solver(n, d, dtype=F64, kernel=None):
    X, diag = dn.train(n, d, dtype)
    return DirectSolver(dn.kernel(kernels, d) if kernel is None else kernel, X, noise.Diagonal(diag))


@pytest.fixture(scope="module")
def solvers():
    """One factored solver per (n, d, dtype) for the whole file -- the handles see calls of every kind and width in
    turn, as a user's would."""
    cache = {}

    def get(n, d, dtype=F64):
        key = (n, d, dtype)
        if key not in cache:
            s = _new_solver(n, d, dtype)
            assert s.info == 0 and s.dtype == np.dtype(dtype)
            cache[key] = s
        return cache[key]

    yield get
    for s in cache.values():
        s.close()


@pytest.fixture(scope="module")
def dot_refs(solvers):
    """(L Z, |L| |Z|) for the 300-column block, once per (n, dtype), on the device's own factor."""
    cache = {}

    def get(n, dtype):
        if (n, dtype) not in cache:
            cache[n, dtype] = dn.dot_reference(solvers(n, 1, dtype).scale_tril, dn.rhs(n, dtype))
        return cache[n, dtype]

    return get


@pytest.fixture(scope="module")
def solve_refs(solvers):
    cache = {}

    def get(n, dtype, transpose):
        key = (n, dtype, transpose)
        if key not in cache:
            cache[key] = dn.solve_reference(solvers(n, 1, dtype).scale_tril, dn.rhs(n, dtype), transpose)
        return cache[key]

    return get


def _within(got, want, bar, what):
    """Componentwise |got - want| <= bar; prints the largest fraction of the bar first."""
    err = np.abs(got.astype(np.longdouble) - want)
    frac = float(np.max(err / bar))
    print(f"{what}: max |err| / bar = {frac:.3g}, max |err| = {float(err.max()):.3g}")
    assert frac <= 1.0, (what, frac)


def _close(got, want, rtol, atol, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    frac = float(np.max(err / (atol + rtol * np.abs(want))))
    print(f"{what}: max |err| / bar = {frac:.3g}, max |err| = {float(err.max()):.3g}")
    assert np.all(np.isfinite(got)) and frac <= 1.0, (what, frac)


# ---- 1. L Z ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", dn.WIDTHS)
@pytest.mark.parametrize("n,dtype", N_DTYPE)
def test_dot_triangular_matches_long_double_product(n, dtype, r, solvers, dot_refs):
    s = solvers(n, 1, dtype)
    Z = np.ascontiguousarray(dn.rhs(n, dtype)[:, :r])
    want, mag = dot_refs(n, dtype)
    want, bar = want[:, :r], dn.dot_bar(n, dtype, mag[:, :r])
    got = s.dot_triangular(Z)
    assert got.shape == (n, r) and got.dtype == np.dtype(dtype)
    _within(got, want, bar, f"L Z {dtype} n={n} r={r}")
    got3 = s.dot_triangular(Z.reshape(n, r, 1))
    assert got3.shape == (n, r, 1)
    np.testing.assert_array_equal(got3[..., 0], got)


@pytest.mark.parametrize("n,dtype", N_DTYPE)
def test_dot_triangular_routes_agree_across_the_eight_column_switch(n, dtype, solvers, dot_refs):
    """R = 7 runs one trmv launch per column, R = 8 and 9 one TRMM-mode MFMA product: the shared columns agree.  Each
    route is an N-term dot product of the same inputs, so each is within gamma_N |L| |Z| of the exact product and
    they are within 2 N eps |L| |Z| of each other."""
    s = solvers(n, 1, dtype)
    Z = dn.rhs(n, dtype)
    want, mag = dot_refs(n, dtype)
    out = {r: s.dot_triangular(np.ascontiguousarray(Z[:, :r])) for r in (7, 8, 9)}
    for r in (7, 8, 9):
        _within(out[r], want[:, :r], dn.dot_bar(n, dtype, mag[:, :r]), f"L Z route r={r} n={n} {dtype}")
    for a, b in ((7, 8), (7, 9), (8, 9)):
        _within(out[a], out[b][:, :a].astype(np.longdouble), dn.dot_bar(n, dtype, mag[:, :a]),
                f"L Z r={a} against r={b} n={n} {dtype}")


def test_sample_is_loc_plus_l_times_the_regenerated_normals():
    """``sample`` draws ``default_rng(key).standard_normal((N,) + shape)`` (gp.py ``sample``) and returns
    ``loc + (L z)`` with the sample axis first."""
    n, key = 300, 20240
    X, diag = dn.train(n, 1)
    gp = GaussianProcess(dn.kernel(kernels, 1), X, diag=diag, mean=0.7)
    got = gp.sample(key, shape=(9,))
    assert got.shape == (9, n)
    z = np.random.default_rng(key).standard_normal((n, 9))
    want, mag = dn.dot_reference(gp.solver.scale_tril, z)
    eps = np.finfo(np.float64).eps
    # the product's bar plus one rounding of the sum loc + L z
    _within(got.T, gp.loc[:, None] + want, dn.dot_bar(n, np.float64, mag) + eps * np.abs(gp.loc[:, None] + want),
            "sample n=300 shape=(9,)")
    again = gp.sample(np.random.default_rng(key), shape=(9,))
    np.testing.assert_array_equal(again, got)


# ---- 2. L^-1 Y and L^-T Y -------------------------------------------------------------------------------------------
def _columns(r):
    return range(r) if r <= 9 else (0, r // 2, r - 1)


@pytest.mark.parametrize("r", dn.WIDTHS)
@pytest.mark.parametrize("n,dtype", N_DTYPE)
def test_solve_triangular_many_columns_both_directions_both_modes(n, dtype, r, solvers, solve_refs):
    s = solvers(n, 1, dtype)
    Y = np.ascontiguousarray(dn.rhs(n, dtype)[:, :r])
    ctx = _ffi.default_ctx()
    for transpose in (False, True):
        want = solve_refs(n, dtype, transpose)[:, :r]
        rtol, atol = dn.solve_bar(dtype, want)
        for mode in (1, 0):
            old = ctx.set_option("stream_trsv", mode)
            try:
                got = s.solve_triangular(Y, transpose=transpose)
                single = {c: s.solve_triangular(np.ascontiguousarray(Y[:, c]), transpose=transpose) for c in _columns(r)}
            finally:
                ctx.set_option("stream_trsv", old)
            what = f"L^-{'T' if transpose else '1'} Y {dtype} n={n} r={r} stream_trsv={mode}"
            assert got.shape == (n, r) and got.dtype == np.dtype(dtype)
            _close(got, want, rtol, atol, what)
            for c, x in single.items():
                if transpose and r > 1:  # the same launches on the same data
                    np.testing.assert_array_equal(got[:, c], x, err_msg=f"{what} column {c}")
                else:
                    _close(got[:, c], x.astype(np.float64), rtol, atol, f"{what} column {c} against the one-vector call")


@pytest.mark.parametrize("transpose", [False, True])
def test_solve_triangular_takes_a_strided_right_hand_side(transpose, solvers, solve_refs):
    n, r = 300, 9
    s = solvers(n, 1)
    wide = np.repeat(dn.rhs(n)[:, :r], 2, axis=1) * np.array([1.0, -3.0] * r)
    Y = wide[:, ::2]
    assert not Y.flags.c_contiguous and np.array_equal(Y, dn.rhs(n)[:, :r])
    got = s.solve_triangular(Y, transpose=transpose)
    want = solve_refs(n, F64, transpose)[:, :r]
    _close(got, want, *dn.solve_bar(F64, want), f"strided Y transpose={transpose}")
    np.testing.assert_array_equal(got, s.solve_triangular(np.ascontiguousarray(Y), transpose=transpose))
    got_dot = s.dot_triangular(Y)
    np.testing.assert_array_equal(got_dot, s.dot_triangular(np.ascontiguousarray(Y)))


# ---- 3. the device-pointer trsm ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [128, 640])
def test_trsm_right_lt_row_counts(n):
    """``tgp_trsm_right_lt`` takes m in multiples of 128 (``tgp_hip.h``): 64 and 192 rows are a bad argument and leave B
    untouched; 128 and 256 rows are solved to the bar of test_trsm_right_lt_vs_lapack."""
    import scipy.linalg as sla

    rng = np.random.default_rng(n)
    A = rng.normal(size=(n, n))
    L = sla.cholesky(A @ A.T / n + np.eye(n), lower=True)
    ctx = _ffi.default_ctx()
    for m in (64, 192):
        B = rng.normal(size=(m, n))
        with pytest.raises(ValueError, match="multiples of 128"):
            ll.trsm_right_lt(L, B)
        dL = ctx.upload(np.asfortranarray(L).ravel(order="K"))
        dB = ctx.upload(np.asfortranarray(B).ravel(order="K"))
        try:
            status = _ffi.lib().tgp_trsm_right_lt(ctx.handle, _ffi.dtype_code(np.float64), m, n, C.c_void_p(dL), n,
                                                  C.c_void_p(dB), m)
            assert status == _ffi.E_ARG
            np.testing.assert_array_equal(ctx.download(dB, (n, m), np.float64).T, B)
        finally:
            ctx.free(dL), ctx.free(dB)
    for m in (128, 256):
        B = rng.normal(size=(m, n))
        want = sla.solve_triangular(L, B.T, lower=True).T
        _close(ll.trsm_right_lt(L, B), want, 1e-10, 1e-10 * np.abs(want).max(), f"trsm_right_lt m={m} n={n}")


# ---- 4. conditional covariance and variance ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", dn.COND_CASES, ids=lambda c: "-".join(map(str, c)))
def test_conditional_covariance_and_variance(case, solvers):
    d, n, m, xt_given, test_noise, other, dtype = case
    s = solvers(n, d, dtype)
    kern = (dn.other_kernel if other else dn.kernel)(kernels, d)
    Xt, nz = dn.query_points(m, d, dtype)
    nzd = nz if test_noise else np.zeros(m, dtype=dtype)
    want, want_var = dn.conditional(*case)
    got = s.condition(kern, Xt if xt_given else None, noise.Diagonal(nzd))
    var = s.condition_variance(kern, Xt if xt_given else None)
    assert got.shape == (m, m) and var.shape == (m,) and got.dtype == var.dtype == np.dtype(dtype)
    tol = dn.posterior_bar(dtype)
    what = "cov " + "-".join(map(str, case))
    _close(got, want, tol["rtol"], tol["atol"], what)
    _close(var, want_var, tol["rtol"], tol["atol"], what.replace("cov", "var"))
    _close(np.diag(got).astype(np.float64) - nzd, var.astype(np.float64), tol["rtol"], tol["atol"], what + " diag - nz against var")
    # symmetric bit for bit: every entry above the diagonal is a copy of its mirror (the 64-block mirror pass)
    np.testing.assert_array_equal(got, got.T)


@pytest.mark.parametrize("n", dn.NS)
def test_public_condition_and_predict_covariance_match_the_oracle(n):
    m = 200
    X, diag = dn.train(n, 1)
    Xt, _ = dn.query_points(m, 1)
    y = np.sin(2.0 * X) + 0.3 * X
    gp = GaussianProcess(dn.kernel(kernels, 1), X, diag=diag)
    ref = o.GaussianProcess(dn.kernel(o, 1), X, diag=diag)
    a, b = gp.condition(y, Xt), ref.condition(y, Xt)
    tol = dn.posterior_bar(F64)
    _close(a.gp.loc, b.gp.loc, tol["rtol"], tol["atol"], f"condition loc n={n}")
    _close(a.gp.covariance, b.gp.covariance, tol["rtol"], tol["atol"], f"condition covariance n={n}")
    loc, cov = gp.predict(y, Xt, return_cov=True)
    rloc, rcov = ref.predict(y, Xt, return_cov=True)
    _close(loc, rloc, tol["rtol"], tol["atol"], f"predict loc n={n}")
    _close(cov, rcov, tol["rtol"], tol["atol"], f"predict covariance n={n}")


# ---- 5. one handle, many calls ----------------------------------------------------------------------------------------
def test_one_handle_gives_the_bits_of_fresh_handles_whatever_came_before():
    """The solver's scratch only grows and every entry point lays it out differently: after a larger call of another
    kind (stale Ks rows, stale padding columns) each result is still, bit for bit, what a new handle returns."""
    n, d = 300, 1
    Z, Y = dn.rhs(n), dn.rhs(n)[:, ::-1]

    def calls(kern):
        q = lambda m: dn.query_points(m, d)  # noqa: E731
        return [
            ("condition M=300", lambda s: s.condition(kern, q(300)[0], noise.Diagonal(q(300)[1]))),
            ("condition M=1", lambda s: s.condition(kern, q(1)[0], noise.Diagonal(q(1)[1]))),
            ("dot_triangular R=129", lambda s: s.dot_triangular(np.ascontiguousarray(Z[:, :129]))),
            ("solve_triangular R=2", lambda s: s.solve_triangular(np.ascontiguousarray(Y[:, :2]))),
            ("condition_variance M=65", lambda s: s.condition_variance(kern, q(65)[0])),
            ("dot_triangular R=8", lambda s: s.dot_triangular(np.ascontiguousarray(Z[:, :8]))),
        ]

    k1, k2 = dn.kernel(kernels, d), dn.other_kernel(kernels, d)
    one = _new_solver(n, d)
    try:
        for kern in (k1, k2):
            if kern is k2:
                assert one.refactor(k2) == 0
            for name, call in calls(kern):
                fresh = _new_solver(n, d, kernel=kern)
                try:
                    want = call(fresh)
                finally:
                    fresh.close()
                got = call(one)
                assert np.all(np.isfinite(want)), name
                np.testing.assert_array_equal(got, want, err_msg=f"{name} after the calls before it "
                                              f"({'refactored' if kern is k2 else 'first'} kernel)")
    finally:
        one.close()


# ---- 6. failure -------------------------------------------------------------------------------------------------------
def test_failed_factorisation_in_the_second_tile_poisons_every_posterior_result():
    n = 300
    X, _ = dn.train(n, 1)
    diag = dn.failing_noise(n)
    _, info = lapack.dpotrf(dn.kernel(o, 1)(X, X) + np.diag(diag), lower=1)
    assert dn.TILE < info <= 2 * dn.TILE
    s = DirectSolver(dn.kernel(kernels, 1), X, noise.Diagonal(diag))
    try:
        assert s.info == info
        Y = np.ascontiguousarray(dn.rhs(n)[:, :9])
        for transpose in (False, True):
            out = s.solve_triangular(Y, transpose=transpose)
            assert out.shape == (n, 9) and np.all(np.isnan(out))
        for r in (7, 9):
            out = s.dot_triangular(np.ascontiguousarray(Y[:, :r]))
            assert out.shape == (n, r) and np.all(np.isnan(out))
        Xt, nz = dn.query_points(129, 1)
        for xt, m in ((Xt, 129), (None, n)):
            out = s.condition(dn.kernel(kernels, 1), xt, noise.Diagonal(np.full(m, 0.02)))
            assert out.shape == (m, m) and np.all(np.isnan(out))
            out = s.condition_variance(dn.kernel(kernels, 1), xt)
            assert out.shape == (m,) and np.all(np.isnan(out))
    finally:
        s.close()
