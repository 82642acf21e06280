"""The inputs and references of ``test_gpu_4_quasisep_edges.py`` checked without a device, so that a failure there
can only mean the device: the sizes reach the shapes they name, the sequential oracles agree with dense LAPACK at the
edge sizes, the oracle's gradient is linear along a combined direction, and the test points land where the gathers of
``qs_pred_emit`` change."""
import numpy as np
import pytest

from tinygp_amd.kernels import quasisep as q

import _quasisep_grad_np as og
import _quasisep_np as o
import _quasisep_predict_np as po
from _quasisep_cases import CASES
from _quasisep_edges import (EDGE_N, GROUP, KERNELS, LC, SHAPES, _levels, _test_points, combine_tangents,
                             direction_matrix, edge_test_points, series, shape, tied_points)


def test_sizes_reach_the_shapes_they_name():
    assert sorted(SHAPES) == EDGE_N
    for n in EDGE_N:
        chunks, levels, last_steps, groups, last_group = SHAPES[n]
        assert _levels(n) == (LC, levels)
        assert shape(n) == SHAPES[n]
        # the table against the arithmetic written out: full chunks and full groups but for the last of each
        assert (chunks - 1) * LC + last_steps == n and 1 <= last_steps <= LC
        assert (groups - 1) * GROUP + last_group == chunks and 1 <= last_group <= GROUP
        assert levels == (1 if chunks <= GROUP else 2) and groups <= GROUP


def test_series_has_both_ties():
    for n in EDGE_N:
        t, noise, r = series(n)
        assert t.shape == noise.shape == r.shape == (n,) and np.all(np.diff(t) >= 0)
        assert t[7] == t[6] and (n <= LC or t[LC] == t[LC - 1])
        assert len(tied_points(t)) == (4 if n > LC else 2)
        assert np.sum(np.diff(t) == 0) == (2 if n > LC else 1)
        assert np.array_equal(series(n)[0], t)  # a function of n alone


@pytest.mark.parametrize("name", ["matern32", "m32cos_plus_sho"])
def test_gradient_oracle_matches_dense_lapack_at_65_chunks(name):
    """N = 1025.  The kernel part at the dense reference's own floor (its central differences), 1e-6 of the largest
    component as in ``test_quasisep_grad_cpu.py``; the noise part at 1e-6 and the mean at 1e-7 of the largest entry."""
    n = 1025
    k = CASES[name](q)
    t, noise, r = series(n)
    lp, g, gn, alpha = og.value_and_grad(k, t, noise, r)
    wlp, wg, wgn, walpha, _ = og.dense_value_and_grad(k, t, noise, r)
    print(f"{name} n={n}: kernel {np.abs(g - wg).max() / np.abs(wg).max():.2e} of max, noise "
          f"{np.abs(gn - wgn).max() / np.abs(wgn).max():.2e} of max, mean {np.abs(alpha - walpha).max() / np.abs(walpha).max():.2e} "
          f"of max")
    assert lp == pytest.approx(wlp, rel=1e-10)
    np.testing.assert_allclose(g, wg, rtol=0, atol=1e-6 * np.abs(wg).max())
    np.testing.assert_allclose(gn, wgn, rtol=1e-6, atol=1e-6 * np.abs(wgn).max())
    np.testing.assert_allclose(alpha, walpha, rtol=1e-7, atol=1e-7 * np.abs(walpha).max())


@pytest.mark.parametrize("name", KERNELS)
def test_prediction_oracle_matches_dense_lapack_at_65_chunks(name):
    """N = 1040 at the edge sweep's own test points (every data point among them): 1e-10."""
    n = 1040
    k = CASES[name](q)
    t, noise, r = series(n)
    xt = edge_test_points(t)
    mean, var = po.predict(k, t, noise, r, xt)
    wmean, wvar = po.dense(k, t, noise, r, xt)
    print(f"{name} n={n}: max |mean - dense| = {np.abs(mean - wmean).max():.2e}, max |var - dense| = "
          f"{np.abs(var - wvar).max():.2e}")
    np.testing.assert_allclose(mean, wmean, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(var, wvar, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("ndir, row", [(9, 8), (17, 16)])  # the rows that run alone in a ragged last batch
def test_gradient_is_linear_along_a_combined_direction(ndir, row):
    """The GPU test takes C @ (oracle gradient) as the derivative along C @ tangents.  The oracle exposes no
    directional derivative, so a combined row of C is held to a central difference of the oracle's log-probability
    along that direction in parameter space: steps h and 2h combined as (4 D(h) - D(2h)) / 3, h = 1e-4.  The truncation
    left is O(h^4); the rounding is about 1e-13 |log p| / h = 1e-6 absolute for |log p| ~ 1e3, against derivatives of
    order 10: 1e-7 relative.  Bar: 1e-6 of sum_j |C_j g_j|, the floor the dense reference is held at."""
    n = 1025
    k = CASES["m32cos_plus_sho"](q)
    t, noise, r = series(n)
    g = og.value_and_grad(k, t, noise, r)[1]
    C = direction_matrix(ndir, 7)
    assert np.array_equal(C[:3], np.eye(7)[:3]) and np.abs(C).max() <= 1.0 and np.all(C[3:] != 0.0)
    d = C[row]
    theta, h = og.get_parameters(k), 1e-4
    try:
        def diff(step):
            vals = []
            for sgn in (1.0, -1.0):
                og.set_parameters(k, theta + sgn * step * d)
                vals.append(o.log_probability(k, t, noise, r))
            return (vals[0] - vals[1]) / (2 * step)
        fd = (4.0 * diff(h) - diff(2 * h)) / 3.0
    finally:
        og.set_parameters(k, theta)
    scale = np.abs(d * g).sum()
    print(f"row {row} of {ndir}: d . g = {d @ g:.10e}, central difference {fd:.10e}, difference {abs(d @ g - fd) / scale:.2e} of sum |d_j g_j|")
    assert abs(d @ g - fd) <= 1e-6 * scale


def test_combined_tangents_are_the_linear_combination():
    k = CASES["m32cos_plus_sho"](q)
    tang = k._ssm_tangents()
    C = direction_matrix(17, len(tang))
    dleaves, dh, dP = combine_tangents(C, tang)
    J, L = k._ssm().J, len(k._ssm().leaves)
    assert dleaves.shape == (17, L, 4) and dh.shape == (17, J) and dP.shape == (17, J, J)
    for i in range(3):  # a unit row is the tangent itself, bit for bit
        assert np.array_equal(dleaves[i], tang[i].dleaves) and np.array_equal(dh[i], tang[i].dh)
        assert np.array_equal(dP[i], tang[i].dPinf)
    np.testing.assert_allclose(dP, np.tensordot(C, np.stack([x.dPinf for x in tang]), axes=1), rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(dleaves, np.tensordot(C, np.stack([x.dleaves for x in tang]), axes=1), rtol=1e-14,
                               atol=1e-14)
    np.testing.assert_allclose(dh, C @ np.stack([x.dh for x in tang]), rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize("n", EDGE_N)
def test_test_points_reach_the_ends(n):
    """Before the first point, past the last, on the last point, inside the first chunk and in the last chunk (whose
    intervals start at its first step), and on the data points either side of the last chunk boundary."""
    t = series(n)[0]
    chunks, _, last_steps, _, _ = SHAPES[n]
    first_of_last = (chunks - 1) * LC
    for xt in (_test_points(t, 200, seed=n), edge_test_points(t)):
        idx = po.intervals(t, xt)
        assert len(xt) >= 200 or n <= LC
        assert np.any(idx == -1) and np.any(xt > t[-1]) and np.any(xt == t[-1])
        assert np.any((xt > t[0]) & (idx < min(LC, n) - 1) & (idx >= 0))
        assert np.any(idx >= first_of_last)
        if last_steps > 8:
            assert np.any((idx >= first_of_last) & (xt > t[first_of_last]) & (xt < t[-1]))
    idx = po.intervals(t, edge_test_points(t))
    if chunks > 1:  # the gathers' lower bounds: the intervals that end one chunk and start the next
        assert np.any(idx == first_of_last)
        assert np.any(idx == first_of_last - 1) or t[first_of_last - 1] == t[first_of_last]  # N = 17: the tie's, empty
    assert all(np.any(idx == i) for i in ((7, LC) if n > LC else (7,)))  # a tie's interval is its last point's
