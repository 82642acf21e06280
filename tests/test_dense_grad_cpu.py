"""The inputs and the reference of ``test_gpu_2_grad_tiles.py`` and of the block-column box cases, checked without a
GPU: ``_dense_grad_np.reference`` asserts its own conditions (cond(K), two routes to the same numbers, every tile of
K^-1 weighted, the partials past the first 1 024 weighted) at every case the GPU files use; the composed analytic
derivatives are tied to the pinned oracle; and the inputs of the older tile-count test are shown to leave the far
tiles of K^-1 without weight -- the gap the new cases close."""
import numpy as np
import pytest

import _dense_grad_np as dg
from oracle import grad_np
from oracle import tinygp_np as o

_CASES = sorted(set(dg.GPU_CASES) | {(p, n, "float64") for p, n, _, _ in dg.BLOCK_COLUMN_CASES},
                key=lambda c: (c[2], c[0], c[1]))


def test_the_case_list_is_the_one_the_tile_counts_call_for():
    cases = set(dg.GPU_CASES)
    both = lambda nt: (128 * nt - 63, 128 * nt)  # noqa: E731
    for p in ("fast", "m32c"):
        assert {(p, n, "float64") for nt in range(1, 18) for n in both(nt)} <= cases
        assert {(p, n, "float32") for nt in (2, 3, 5) for n in both(nt)} <= cases
    assert {("ess", n, "float64") for nt in (1, 2, 3, 6, 11, 16, 17) for n in both(nt)} <= cases
    assert {("linear", n, "float64") for nt in (1, 2, 3) for n in both(nt)} <= cases  # (_dense_grad_np.LINEAR_COUNTS)
    for p in dg.PROGRAMS:
        assert {(p, 4161, "float64"), (p, 4224, "float64")} <= cases
    assert len(cases) == len(dg.GPU_CASES) == 2 * 34 + 14 + 6 + 4 * 2 + 2 * 6


@pytest.mark.parametrize("case", _CASES, ids=lambda c: "-".join(map(str, c)))
def test_reference_conditions_hold_at_every_gpu_case(case):
    name, n, dtype = case
    d = dg.PROGRAMS[name][0]
    X, diag, y = dg.inputs(n, d, dtype)
    assert X.dtype == diag.dtype == y.dtype == np.dtype(dtype) and X.shape == ((n,) if d == 1 else (n, 3))
    assert X.min() >= 0.0 and X.max() <= (4.0 if d == 1 else 3.0)  # the box does not grow with N
    assert not (X.flags.writeable or diag.flags.writeable or y.flags.writeable)
    ref = dg.reference(name, n, dtype)  # asserts conditions 1-4
    nt = -(-n // dg.TILE)
    npar = len(dg.PROGRAMS[name][1])
    assert ref.g.shape == (npar,) and ref.tiles.shape == (npar, nt, nt)
    assert ref.noise.shape == ref.alpha.shape == (n,) and np.isfinite(ref.ll)
    assert np.all(np.isfinite(ref.tiles[:, np.tril_indices(nt)[0], np.tril_indices(nt)[1]]))
    assert (ref.tail is None) == (nt * nt <= dg.SECOND_PASS)
    assert not (ref.g.flags.writeable or ref.tiles.flags.writeable)
    print(f"{name} N={n} {dtype}: cond {ref.cond:.3g}, routes agree to {ref.route_gap:.1e}, lightest tile "
          f"{ref.min_tile:.4g} bars, tail {ref.tail}")


@pytest.mark.parametrize("name", sorted(dg.PROGRAMS))
def test_analytic_derivatives_against_the_pinned_oracle_at_n300(name):
    """The composed closed forms through the trace identity against ``oracle.grad_np`` (the same identity with dK by
    central differences of the oracle's kernel matrix) at the bar test_oracle.py holds the closed forms to, 2e-7; the
    value against the oracle's own ``log_probability``, which is pinned to the reference."""
    d, theta, build, _ = dg.PROGRAMS[name]
    X, diag, y = dg.inputs(300, d)
    ref = dg.reference(name, 300)
    want_ll, want_g, want_noise, want_alpha = grad_np.log_probability_and_grad(lambda t: build(o, t), theta, X, diag, y)
    scale = np.abs(want_g).max()
    np.testing.assert_allclose(ref.g, want_g, rtol=2e-7, atol=2e-7 * scale)
    np.testing.assert_allclose(ref.ll, want_ll, rtol=1e-12)
    np.testing.assert_allclose(ref.noise, want_noise, rtol=1e-9, atol=1e-9 * np.abs(want_noise).max())
    np.testing.assert_allclose(ref.alpha, want_alpha, rtol=1e-9, atol=1e-9 * np.abs(want_alpha).max())


def test_tile_table_sees_a_wrong_tile():
    """The table is what it says: zeroing one far tile of K^-1 moves the gradient by that tile's entry, in bars."""
    name, n = "fast", 705
    d, theta, build, derivs = dg.PROGRAMS[name]
    X, diag, y = (np.asarray(a) for a in dg.inputs(n, d))
    ref = dg.reference(name, n)
    K = build(o, theta)(X, X) + np.diag(diag)
    Kinv = np.linalg.inv(K)
    bad = Kinv.copy()
    a, b = 5, 0
    bad[a * 128:(a + 1) * 128, b * 128:(b + 1) * 128] = 0.0
    bad[b * 128:(b + 1) * 128, a * 128:(a + 1) * 128] = 0.0
    alpha = Kinv @ y
    dKs = derivs(theta, X.reshape(n, -1))
    g_bad = np.array([0.5 * np.sum((np.outer(alpha, alpha) - bad) * dK) for dK in dKs])
    moved = np.abs(g_bad - ref.g) / (2e-6 * np.abs(ref.g).max())
    np.testing.assert_allclose(moved, ref.tiles[:, a, b], rtol=1e-6)
    assert moved.min() >= 100.0


def test_the_older_tile_count_inputs_leave_the_far_tiles_without_weight():
    """A record of the gap: with the inputs of test_gpu_2_grad.py::test_grad_block_structures_of_the_inverse at
    N = 1 400 (X on [0, N / 40], ExpSquared of scale 0.9) every tile three or more off the diagonal -- 36 of the 66 --
    weighs less than 1e-5 of the bar, so whatever spd_inverse_lower writes there passes that test.  (Two off the
    diagonal the tiles weigh 0.12 ... 221 bars, some of them nothing either; on and next to the diagonal 6e4 and more.
    The same at N = 640 and 3 000: at most 3e-8 and 5e-6 of the bar from three tiles off.)"""
    n = 1400
    rng = np.random.default_rng(n)
    X = np.sort(rng.uniform(0, n / 40.0, n))
    y = np.sin(X) + 0.1 * rng.normal(size=n)
    diag = rng.uniform(0.05, 0.15, n)
    theta = (1.7, 0.9)
    K = dg.PROGRAMS["fast"][2](o, theta)(X, X) + np.diag(diag)
    Kinv = np.linalg.inv(K)
    alpha = Kinv @ y
    dKs = dg.PROGRAMS["fast"][3](theta, X.reshape(n, 1))
    g = np.array([0.5 * np.sum((np.outer(alpha, alpha) - Kinv) * dK) for dK in dKs])
    tiles = dg.tile_weights(Kinv, dKs, g, 2e-6)
    nt = tiles.shape[1]
    off = np.subtract.outer(np.arange(nt), np.arange(nt))
    assert nt == 11 and (off >= 3).sum() == 36
    assert np.max(tiles[:, off >= 3]) < 1e-5
    assert np.min(tiles[:, off == 2]) < 1.0 and np.max(tiles[:, off == 2]) < 300.0
    assert np.min(tiles[:, (off == 0) | (off == 1)]) > 6e4
