"""Posterior samples of a quasiseparable GP on the device (``tgp_qsep_sample``, ``QuasisepSolver.sample_conditional``,
``GaussianProcess.sample_conditional``) and the conditional mean of many columns (``tgp_qsep_predict_mean``).

The sampler is a linear map of the standard normals it is given, so its distribution is checked exactly: fed every unit
vector as a column it returns S with S S^T the conditional covariance, and at zero normals the conditional mean, both
against dense LAPACK at 1e-9 (the covariance is linear in Q, so the cancellation in Q is not square-rooted; the same
construction reaches a few 1e-15 in NumPy, ``test_quasisep_sample_cpu.py``).  Value for value it is held to the
sequential statement ``_quasisep_sample_np`` at the project's posterior bar rtol = atol = 5e-7, at the edges of both
scans: the merged grid's (G points) and the data's (N points), chunks of 16 and groups of 64 chunks.  Every test prints
the figures it asserts; the coordinates keep distinct neighbours 0.02 apart (``_quasisep_sample_np.lattice`` says why).
"""
import numpy as np
import pytest

from tinygp_amd import GaussianProcess, kernels
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.noise import Diagonal
from tinygp_amd.solvers import DirectSolver, QuasisepSolver

import _quasisep_sample_np as so
from _quasisep_cases import CASES

pytestmark = pytest.mark.gpu

BAR = dict(rtol=5e-7, atol=5e-7)


@pytest.fixture
def solver():
    """``solver(kernel, t, noise)``: a ``QuasisepSolver`` that is closed when the test ends, passed or failed."""
    made = []

    def make(kernel, t, noise):
        made.append(QuasisepSolver(kernel, t, Diagonal(noise)))
        return made[-1]
    yield make
    for s in made:
        s.close()


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


# ---- 1. the exact distribution ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(1, 1), (5, 3), (17, 9), (70, 40)])
@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_distribution(solver, name, n, m):
    """R = (N + M) J + N unit vectors (up to 950 columns: many passes of 64): S S^T and the value at zero normals
    against the dense joint conditional covariance and mean of data and test points, every entry within 1e-9."""
    k = CASES[name](q)
    t, noise, r, xt = so.problem(n, m)
    J = k._ssm().J
    xi, eps = so.unit_normals(n, m, J)
    s = solver(k, t, noise)
    S = np.vstack(s.sample_conditional(np.zeros(n), xt, xi=xi, eps=eps, return_data=True))
    assert s.info == 0 and S.shape == (n + m, (n + m) * J + n) and s.sample_passes == -(-S.shape[1] // 64)
    mean = np.concatenate(s.sample_conditional(r, xt, xi=np.zeros((n + m, J)), eps=np.zeros(n), return_data=True))
    wmean, wcov = so.dense(k, t, noise, r, np.concatenate([t, xt]))
    ecov, emean = np.abs(S @ S.T - wcov).max(), np.abs(mean - wmean).max()
    print(f"sample distribution {name} n={n} m={m} R={S.shape[1]}: max |S S^T - cov| = {ecov:.2e} (data block "
          f"{np.abs(S[:n] @ S[:n].T - wcov[:n, :n]).max():.2e}), max |mean - dense| = {emean:.2e}")
    assert ecov <= 1e-9 and emean <= 1e-9


# ---- 2. value for value at the scans' edges ---------------------------------------------------------------------------------
def _edge_problem(n, m, kind):
    """Data and test points on one lattice.  ``kind``: "spread" -- test points anywhere, two below the first and two
    above the last data point (M >= 4); "interval" -- all of them inside one interval of the data; ties t[16] = t[15]
    (across the data's first chunk boundary) and t[N - 1] = t[N - 2], and test points on both (M >= 4)."""
    rng = np.random.default_rng(100 * n + m)
    coords = so.lattice(rng, n + m)
    is_test = np.zeros(n + m, dtype=bool)
    if kind == "interval":
        lo = n // 2
        is_test[lo:lo + m] = True
    elif m:
        pick = rng.permutation(np.arange(2, n + m - 2))[:max(m - 4, 0)] if m >= 4 else rng.permutation(n + m)[:m]
        is_test[pick] = True
        if m >= 4:
            is_test[[0, 1, n + m - 2, n + m - 1]] = True
    t, xt = coords[~is_test], coords[is_test]
    if n > 16:
        t[16], t[n - 1] = t[15], t[n - 2]
    xt = xt[rng.permutation(m)]
    if m >= 8 and kind == "spread":  # on the tied data points; the extremes are kept
        inner = np.argsort(xt)[2:-2]
        xt[inner[0]], xt[inner[1]] = t[15], t[n - 1]
    return t, rng.uniform(0.05, 0.2, n), rng.standard_normal(n), xt


# (N, M or None, kind): G = N + M in {16, 17, 1024, 1025, 1041}: one chunk, a last chunk of one point, 64 chunks, 65
# chunks (the second scan level); N in {16, 17, 1024, 1025} the same on the data's side
EDGES = [(16, None, "none"), (16, 1, "spread"), (17, 0, "spread"), (1024, None, "none"), (1024, 1, "spread"),
         (1024, 17, "spread"), (1025, 16, "spread"), (768, 257, "interval")]


@pytest.mark.parametrize("n,m,kind", EDGES)
@pytest.mark.parametrize("name", ["matern32", "m32cos_plus_sho"])
def test_draws_match_the_oracle(solver, name, n, m, kind):
    """R = 9 random columns (two column groups, the second with one live column), J = 2 and J = 6, data and test side,
    rtol = atol = 5e-7."""
    k = CASES[name](q)
    t, noise, r, xt = _edge_problem(n, m or 0, kind)
    rng = np.random.default_rng(7)
    J, G = k._ssm().J, n + (m or 0)
    xi, eps = rng.standard_normal((G, J, 9)), rng.standard_normal((n, 9))
    s = solver(k, t, noise)
    wdata, wtest = so.sample(k, t, noise, r, xt, xi, eps)
    if m is None:
        data, test = s.sample_conditional(r, None, xi=xi, eps=eps), np.zeros((0, 9))
    else:
        data, test = s.sample_conditional(r, xt, xi=xi, eps=eps, return_data=True)
    assert s.info == 0 and data.shape == (n, 9) and test.shape == (m or 0, 9) and s.sample_passes == 1
    if m is not None:  # the test side alone (M = 0: nothing to do, no pass)
        assert _same(test, s.sample_conditional(r, xt, xi=xi, eps=eps)) and s.sample_passes == (1 if m else 0)
    print(f"sample edge {name} n={n} m={m} {kind}: max |data - oracle| = {np.abs(data - wdata).max():.3e}, max |test - "
          f"oracle| = {np.abs(test - wtest).max() if test.size else 0.0:.3e}")
    np.testing.assert_allclose(data, wdata, **BAR)
    np.testing.assert_allclose(test, wtest, **BAR)
    if n > 16:  # a tie gets one prior value exactly; f + v - noise alpha rounds v - noise alpha (both O(1), alpha to
        # about cond(K) 2^-52 ~ 1e-13) on each of the two points: 1e-11
        np.testing.assert_allclose(data[15], data[16], rtol=0, atol=1e-11)
        np.testing.assert_allclose(data[n - 2], data[n - 1], rtol=0, atol=1e-11)


# ---- 3. columns are independent; calls are deterministic -----------------------------------------------------------------------
def test_columns_are_independent_and_calls_deterministic(solver):
    """Column c of an R = 65 call (two passes: 64 + 1) equals a call with that column alone, bit for bit, whatever its
    column group and lane; two identical calls agree bit for bit."""
    k = CASES["m32cos_plus_sho"](q)
    n, m = 70, 40
    t, noise, r, xt = so.problem(n, m)
    rng = np.random.default_rng(8)
    xi, eps = rng.standard_normal((n + m, 6, 65)), rng.standard_normal((n, 65))
    s = solver(k, t, noise)
    data, test = s.sample_conditional(r, xt, xi=xi, eps=eps, return_data=True)
    assert s.sample_passes == 2
    again = s.sample_conditional(r, xt, xi=xi, eps=eps, return_data=True)
    assert _same(data, again[0]) and _same(test, again[1])
    for c in (0, 7, 8, 31, 63, 64):
        d1, t1 = s.sample_conditional(r, xt, xi=xi[:, :, c], eps=eps[:, c], return_data=True)
        assert s.sample_passes == 1 and d1.shape == (n,) and t1.shape == (m,)
        assert _same(d1, data[:, c]) and _same(t1, test[:, c]), c
    d9, t9 = s.sample_conditional(r, xt, xi=xi[:, :, 56:65], eps=eps[:, 56:65], return_data=True)
    assert _same(d9, data[:, 56:65]) and _same(t9, test[:, 56:65])


# ---- 4. the conditional mean of many columns -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 17, 1024, 1025])
def test_predict_mean_of_a_block_of_residuals(solver, n):
    """``predict_mean_var`` with an (N, R) residual, R in {1, 8, 9}, against R single calls at rtol = atol = 5e-7; the
    1-D call keeps its bits: it equals ``conditional_mean``'s 1-D route, which this change does not touch."""
    k = CASES["m32cos_plus_sho"](q)
    t, noise, r, xt = _edge_problem(n, 24, "spread")
    Y = np.random.default_rng(9).standard_normal((n, 9))
    s = solver(k, t, noise)
    single = np.stack([s.predict_mean_var(Y[:, c], xt, return_var=False) for c in range(9)], axis=1)
    for R in (1, 8, 9):
        got = s.predict_mean_var(Y[:, :R], xt, return_var=False)
        assert got.shape == (len(xt), R)
        print(f"predict block n={n} R={R}: max |block - single| = {np.abs(got - single[:, :R]).max():.3e}")
        np.testing.assert_allclose(got, single[:, :R], **BAR)
        alpha = np.stack([s.alpha(Y[:, c])[0] for c in range(R)], axis=1)
        assert _same(s.conditional_mean(k, xt, alpha), got)
    assert _same(s.conditional_mean(k, xt, s.alpha(Y[:, 0])[0]), single[:, 0])
    assert s.predict_mean_var(Y[:, :0], xt, return_var=False).shape == (len(xt), 0)
    assert s.predict_mean_var(Y, xt[:0], return_var=False).shape == (0, 9)
    with pytest.raises(ValueError):
        s.predict_mean_var(Y, xt)


# ---- 5. the front end ---------------------------------------------------------------------------------------------------------------
def test_gaussian_process_sample_conditional():
    k = CASES["sum_sho_m32"](q)
    n, m = 70, 40
    t, noise, r, xt = so.problem(n, m)
    mean = lambda x: 0.5 * x - 1.0  # noqa: E731
    gp = GaussianProcess(k, t, diag=noise, mean=mean)
    y = r + mean(t)
    one = gp.sample_conditional(y, xt, key=3)
    many = gp.sample_conditional(y, xt, key=3, shape=(2, 5))
    at_data = gp.sample_conditional(y, key=3, shape=(4,))
    assert one.shape == (m,) and many.shape == (2, 5, m) and at_data.shape == (4, n) and one.dtype == np.float64
    assert _same(many, gp.sample_conditional(y, xt, key=np.random.default_rng(3), shape=(2, 5)))
    assert not _same(many, gp.sample_conditional(y, xt, key=4, shape=(2, 5)))
    bare = gp.sample_conditional(y, xt, key=3, shape=(2, 5), include_mean=False)
    np.testing.assert_allclose(many - bare, np.broadcast_to(mean(xt), many.shape), rtol=0, atol=1e-12)
    # the draw is the solver's, from xi, then eps, of the generator
    rng = np.random.default_rng(3)
    xi, eps = rng.standard_normal((n + m, 4, 10)), rng.standard_normal((n, 10))
    want = gp.solver.sample_conditional(r, xt, xi=xi, eps=eps)
    np.testing.assert_allclose(bare.reshape(10, m).T, want, rtol=0, atol=1e-12)
    # the sample mean over many draws approaches the conditional mean: 4000 draws, 6 sigma of the largest variance
    draws = gp.sample_conditional(y, xt, key=5, shape=(4000,), include_mean=False)
    pm, pv = gp.solver.predict_mean_var(r, xt)
    print(f"sample front end: max |mean of 4000 draws - conditional mean| = {np.abs(draws.mean(axis=0) - pm).max():.3e} "
          f"(6 sigma: {6 * np.sqrt(pv.max() / 4000):.3e})")
    assert np.abs(draws.mean(axis=0) - pm).max() <= 6 * np.sqrt(pv.max() / 4000)
    # fp32 in, fp32 out, computed in fp64
    t32, n32, y32, x32 = (a.astype(np.float32) for a in (t, noise, y, xt))
    gp32 = GaussianProcess(k, t32, diag=n32, mean=mean)
    gp64 = GaussianProcess(k, t32.astype(np.float64), diag=n32.astype(np.float64), mean=mean)
    s32 = gp32.sample_conditional(y32, x32, key=3, shape=(3,))
    s64 = gp64.sample_conditional(y32.astype(np.float64), x32.astype(np.float64), key=3, shape=(3,))
    print(f"sample front end: max |fp32 - fp64| = {np.abs(s32 - s64).max():.3e}")
    assert s32.dtype == np.float32 and s32.shape == (3, m)
    np.testing.assert_allclose(s32, s64, rtol=5e-4, atol=5e-4)
    for g in (gp, gp32, gp64):
        g.solver.close()


def test_direct_solver_raises_and_a_failed_factor_gives_nan():
    t, noise, r, xt = so.problem(30, 10)
    dense_gp = GaussianProcess(kernels.ExpSquared(scale=1.5), t, diag=noise, solver=DirectSolver)
    with pytest.raises(TypeError, match="QuasisepSolver"):
        dense_gp.sample_conditional(r, xt, key=0)
    bad = noise.copy()
    bad[11] = -50.0
    gp = GaussianProcess(CASES["matern32"](q), t, diag=bad)
    out = gp.sample_conditional(r, xt, key=0, shape=(3,))
    at_data = gp.sample_conditional(r, key=0)
    assert gp.solver.info != 0
    assert out.shape == (3, 10) and np.isnan(out).all() and at_data.shape == (30,) and np.isnan(at_data).all()
    assert np.isnan(gp.solver.predict_mean_var(np.stack([r, r], axis=1), xt, return_var=False)).all()
    gp.solver.close()
