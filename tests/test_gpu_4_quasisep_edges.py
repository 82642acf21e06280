"""The gradient and the prediction of ``QuasisepSolver`` at every edge of the chunked scan (``_quasisep_edges``:
N = 15 ... 4097, one and two levels, last chunks and last groups of one element) and at ragged direction batches,
against the sequential oracles and dense LAPACK.  These are the routes of ``csrc/qsep.hip`` that the structure sweep
(``test_gpu_4_quasisep_structure.py``: solves and factor) does not walk: the factor and solve tangents (``ScanCong`` /
``ScanAffine`` of width ndir), the noise gradient (``ScanPred`` backwards, ``qs_invdiag_emit``), ``qs_pred_emit``'s
gathers at chunk ends and ``qs_pred_identity``.

Bars: the gradient's of ``test_gpu_4_quasisep_grad.py`` (value 1e-8 relative; kernel 2e-6, noise 1e-6, mean 1e-7, each
with atol = bar x the largest reference entry) and the project's posterior bar rtol = atol = 5e-7.  Every test prints
the figures it asserts; every reference is computed once per module and never written to."""
import numpy as np
import pytest

from tinygp_amd.kernels import quasisep as q
from tinygp_amd.noise import Diagonal
from tinygp_amd.solvers import QuasisepSolver

import _quasisep_grad_np as og
import _quasisep_predict_np as po
import _quasisep_terms_np as tn
from _quasisep_cases import CASES
from _quasisep_edges import (EDGE_N, KERNELS, SHAPES, combine_tangents, direction_matrix, edge_test_points,
                             eight_exp_terms, grad_figures, series, shape)

pytestmark = pytest.mark.gpu

BAR = dict(rtol=5e-7, atol=5e-7)
DENSE_UP_TO = 1040  # dense LAPACK up to here, the sequential oracle above

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _frozen(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def _grad_oracle(name, n):
    t, noise, r = series(n)
    return _once(("grad", name, n), lambda: _frozen(og.value_and_grad(CASES[name](q), t, noise, r)))


def _predict_reference(name, n):
    """``(xt, mean, var)`` at the edge sweep's test points."""
    def make():
        t, noise, r = series(n)
        xt = edge_test_points(t)
        ref = po.dense if n <= DENSE_UP_TO else po.predict
        return _frozen((xt,) + tuple(ref(CASES[name](q), t, noise, r, xt)))
    return _once(("predict", name, n), make)


def _data_reference(name, n):
    """``(mean, var)`` at the data points themselves."""
    def make():
        t, noise, r = series(n)
        ref = po.dense if n <= DENSE_UP_TO else po.predict
        return _frozen(tuple(ref(CASES[name](q), t, noise, r, t)))
    return _once(("data", name, n), make)


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


def test_sizes_reach_the_shapes_they_name():
    """The size list against the table of shapes it names (host arithmetic; no device)."""
    assert sorted(SHAPES) == EDGE_N
    assert {n: shape(n) for n in EDGE_N} == SHAPES


# ---- 1. the gradient at every edge ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_N)
@pytest.mark.parametrize("name", KERNELS)
def test_gradient_matches_the_oracle(solver, name, n):
    """value 1e-8 relative, kernel 2e-6, noise 1e-6, mean 1e-7 (atol = bar x the largest reference entry).  The noise
    gradient and alpha are compared over all N entries: the backward scan's first chunk is the short last one."""
    t, noise, r = series(n)
    s = solver(CASES[name](q), t, noise)
    ll, g = s.value_and_grad(r)
    assert s.info == 0
    wll, wg, wgn, walpha = _grad_oracle(name, n)
    v, ke, ne, me = grad_figures((ll, g), (wll, wg, wgn, walpha))
    ends = np.r_[0:min(17, n), max(0, n - 17):n]
    print(f"edge grad {name} n={n}: value rel {v:.2e}; kernel {ke:.2e} of max; noise {ne:.2e} of max (first / last 17: "
          f"{np.abs(g['noise_diag'] - wgn)[ends].max() / np.abs(wgn).max():.2e}); mean {me:.2e} of max")
    gk = np.asarray(g["kernel"])
    assert np.isfinite(ll) and gk.shape == wg.shape and g["transform"] is None
    assert g["noise_diag"].shape == g["mean"].shape == (n,)
    assert ll == pytest.approx(wll, rel=1e-8)
    np.testing.assert_allclose(gk, wg, rtol=2e-6, atol=2e-6 * np.abs(wg).max())
    np.testing.assert_allclose(g["noise_diag"], wgn, rtol=1e-6, atol=1e-6 * np.abs(wgn).max())
    np.testing.assert_allclose(g["mean"], walpha, rtol=1e-7, atol=1e-7 * np.abs(walpha).max())


# ---- 2. direction counts ----------------------------------------------------------------------------------------------
DIR_KERNEL = "m32cos_plus_sho"
NDIRS = [1, 2, 7, 8, 9, 17]


@pytest.fixture(scope="module")
def direction_problem():
    """``direction_problem(n)``: one solver per N, shared by the direction counts and closed after the module:
    ``(solver, r, tangents, value_and_grad's result)``."""
    held = {}

    def get(n):
        if n not in held:
            k = CASES[DIR_KERNEL](q)
            t, noise, r = series(n)
            s = QuasisepSolver(k, t, Diagonal(noise))
            held[n] = (s, r, k._ssm_tangents(), s.value_and_grad(r))
            assert len(held[n][2]) == 7
        return held[n]
    yield get
    for s, *_ in held.values():
        s.close()


@pytest.mark.parametrize("ndir", NDIRS)
@pytest.mark.parametrize("n", [1025, 4097])
def test_direction_counts(direction_problem, n, ndir):
    """A batch holds 8 directions: 9 and 17 leave a ragged last batch of one, 1 ... 8 change the scans' width.  Forward
    mode is linear in the direction, so the derivatives along C @ tangents are C @ (oracle gradient): bar 2e-6 with
    atol = 2e-6 x max_i sum_j |C_ij g_j|.  The value, the noise gradient and alpha do not depend on the directions
    (bit for bit); a direction that runs alone in the ragged batch equals its single-direction call bit for bit."""
    s, r, tang, (ll, g) = direction_problem(n)
    C = direction_matrix(ndir, 7)
    dleaves, dh, dP = combine_tangents(C, tang)
    v, kg, gn, alpha = s._grad_call(r, dleaves, dh, dP, vectors=True)
    assert s.info == 0 and kg.shape == (ndir,)
    wg = _grad_oracle(DIR_KERNEL, n)[1]
    want, scale = C @ wg, (np.abs(C) * np.abs(wg)).sum(axis=1).max()
    print(f"edge dirs n={n} ndir={ndir}: max |d - C g| = {np.abs(kg - want).max() / scale:.2e} of max_i sum_j |C_ij g_j|")
    np.testing.assert_allclose(kg, want, rtol=2e-6, atol=2e-6 * scale)
    assert v == ll and _same(gn, g["noise_diag"]) and _same(alpha, g["mean"])
    for i in range(min(ndir, 3)):  # the unit rows: value_and_grad's own derivatives
        assert kg[i] == g["kernel"][i], (i, kg[i], g["kernel"][i])
    for row in (8, 16):  # ndir = 9: row 8 alone in the second batch; ndir = 17: row 8 leads a full batch, row 16 is alone
        if row < ndir:
            one = s._grad_call(r, dleaves[row:row + 1], dh[row:row + 1], dP[row:row + 1], vectors=False)
            assert one[2] is None and one[3] is None
            assert one[0] == ll and one[1][0] == kg[row], (row, one[1][0], kg[row])


# ---- 3. prediction at every edge ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_N)
@pytest.mark.parametrize("name", KERNELS)
def test_prediction_matches_the_reference(solver, name, n):
    """Test points outside the range, on both sides of every kind of chunk end, on the tied data points and (up to
    N = 1040) on every data point; dense LAPACK up to N = 1040, the sequential oracle at 4097; rtol = atol = 5e-7."""
    k = CASES[name](q)
    t, noise, r = series(n)
    xt, wmean, wvar = _predict_reference(name, n)
    s = solver(k, t, noise)
    mean, var = s.predict_mean_var(r, xt)
    assert s.info == 0 and mean.shape == var.shape == xt.shape
    print(f"edge predict {name} n={n} m={len(xt)}: max |mean - ref| = {np.abs(mean - wmean).max():.3e}, "
          f"max |var - ref| = {np.abs(var - wvar).max():.3e}")
    np.testing.assert_allclose(mean, wmean, **BAR)
    np.testing.assert_allclose(var, wvar, **BAR)
    if name == DIR_KERNEL:  # the phases skipped: the mean alone, the variance alone through the hook
        assert _same(s.predict_mean_var(r, xt, return_var=False), mean)
        assert _same(s.condition_variance(k, xt), var)


# ---- 4. the data as test points ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1009, 1025, 4097])
@pytest.mark.parametrize("name", KERNELS)
def test_prediction_at_the_data(solver, name, n):
    """``predict_terms(r, None)`` with the model as its own single term (``qs_pred_identity``: nothing uploaded or
    sorted) against the reference at xt = t (5e-7), and bit for bit against ``predict_mean_var(r, t.copy())``: the two
    paths are meant to share bits ("results equal those of the same points passed explicitly").
    The tied points (6, 7 and 15, 16) are data points like the others."""
    k = CASES[name](q)
    t, noise, r = series(n)
    wmean, wvar = _data_reference(name, n)
    s = solver(k, t, noise)
    means, vars_ = s.predict_terms(r, None, [k])
    assert means.shape == vars_.shape == (1, n)
    print(f"edge data {name} n={n}: max |mean - ref| = {np.abs(means[0] - wmean).max():.3e}, "
          f"max |var - ref| = {np.abs(vars_[0] - wvar).max():.3e}")
    np.testing.assert_allclose(means[0], wmean, **BAR)
    np.testing.assert_allclose(vars_[0], wvar, **BAR)
    mean, var = s.predict_mean_var(r, t.copy())
    assert _same(means[0], mean) and _same(vars_[0], var)


# ---- 5. eight terms across a group boundary ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1025, 4097])
def test_eight_terms(solver, n):
    """J = 8 as eight ``Exp`` terms, all in one call: dense LAPACK per term at N = 1025, the sequential oracle with the
    eight test-side vectors at 4097; the term means add up to the model's mean.  All at rtol = atol = 5e-7."""
    k, terms = eight_exp_terms(q)
    assert k._ssm().J == 8 and k._addends() == terms
    t, noise, r = series(n)
    xt = edge_test_points(t)
    s = solver(k, t, noise)
    means, vars_ = s.predict_terms(r, xt)
    assert s.info == 0 and means.shape == vars_.shape == (8, len(xt))
    if n <= DENSE_UP_TO:
        want = [tn.dense_term(k, term, t, noise, r, xt) for term in terms]
        wmeans, wvars = np.stack([m for m, _ in want]), np.stack([v for _, v in want])
    else:
        wmeans, wvars = tn.predict_g(k, t, noise, r, xt, np.stack([k._term_vector(term) for term in terms]))
    mean = s.predict_mean_var(r, xt, return_var=False)
    print(f"edge terms n={n}: max |mean - ref| = {np.abs(means - wmeans).max():.3e}, max |var - ref| = "
          f"{np.abs(vars_ - wvars).max():.3e}, |sum of term means - mean| = {np.abs(means.sum(axis=0) - mean).max():.3e}")
    np.testing.assert_allclose(means, wmeans, **BAR)
    np.testing.assert_allclose(vars_, wvars, **BAR)
    np.testing.assert_allclose(means.sum(axis=0), mean, **BAR)


# ---- 6. one handle across routes at an edge size ------------------------------------------------------------------------------
def test_one_handle_across_routes(solver):
    """N = 1025 (65 chunks): gradient, prediction, a solve with R = 9 and the gradient again on one handle.  Every
    route regrows and rewrites ``work`` under another policy and width; nothing may leak from one into the next."""
    n = 1025
    k = CASES[DIR_KERNEL](q)
    t, noise, r = series(n)
    xt = _predict_reference(DIR_KERNEL, n)[0]
    s = solver(k, t, noise)
    ll, g = s.value_and_grad(r)
    mean, var = s.predict_mean_var(r, xt)
    Y = np.random.default_rng(6).standard_normal((n, 9))
    Z = s.solve_triangular(Y)
    ll2, g2 = s.value_and_grad(r)
    assert ll == ll2 and g["kernel"] == g2["kernel"]
    assert _same(g["noise_diag"], g2["noise_diag"]) and _same(g["mean"], g2["mean"])
    fresh = solver(k, t, noise)
    fmean, fvar = fresh.predict_mean_var(r, xt)
    assert _same(mean, fmean) and _same(var, fvar)
    assert _same(Z, fresh.solve_triangular(Y))
    wll, wg, wgn, walpha = _grad_oracle(DIR_KERNEL, n)
    v, ke, ne, me = grad_figures((ll2, g2), (wll, wg, wgn, walpha))
    print(f"edge handle n={n}: second gradient: value rel {v:.2e}; kernel {ke:.2e}; noise {ne:.2e}; mean {me:.2e}")
    assert v <= 1e-8 and ke <= 2e-6 and ne <= 1e-6 and me <= 1e-7
