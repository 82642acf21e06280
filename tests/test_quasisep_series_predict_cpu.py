"""Prediction for sets of series, host side: the mirrored split rule with its worked examples, the packing of the test
points and of the means with their error messages, the value-sort-then-locate order and the entry point's declaration."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tinygp_amd import _ffi
from tinygp_amd.solvers.quasisep import pack_series_tests, series_added_means

import _quasisep_predict_np as op
import _quasisep_series as qs
import _quasisep_series_predict as qp

ROOT = Path(__file__).resolve().parent.parent
M = 1 << 20


# -- the mirrored rule -----------------------------------------------------------------------------------------------------------
def test_need_of_a_short_and_a_long_series():
    # 40 points, 7 test points, J = 2: 3 chunks, S4 = 3 + 3
    assert qp.need(40, 7, 2) == 40 * 6 + 384 * 6 + 9 + 6 + 40 + 7 * 15 == 2704
    assert qp.need(40, 7, 2, want_mean=False) == 2704 - 40 - 7
    assert qp.need(40, 7, 2, want_var=False) == 2704 - 7
    assert qp.need(40, 7, 2, False, False) == 40 * 6 + 384 * 6 + 9 + 6 + 7 * 13 == 2650
    # 2^20 points predicted at themselves, J = 2: 4096 chunks, S4 = 4096 + 64 + 2
    assert qp.need(M, M, 2) == 22 * M + 384 * 4162 + 12288 + 6 == 24_679_174
    assert qp.need(M, 0, 2) == 7 * M + 384 * 4162 + 12288 + 6 == 8_950_534
    assert qp.BUDGET == (1 << 27) - 64 * 141 == 134_208_704


def test_the_value_s_need_is_inside():
    """What prediction adds to the value's need: 128 S4 of work space, the table entry, alpha and the test points."""
    for n, J in ((1, 1), (40, 2), (1025, 6), (65_537, 8), (M + 1, 2)):
        e = qs.extent(n)
        s4 = sum(e.levels) + qs.MAX_LEVELS - len(e.levels)
        assert qp.need(n, 0, J, False, False) == qs.need(n, J) + 128 * s4 + 3
        assert qp.need(n, 5, J, True, False) == qs.need(n, J) + 128 * s4 + 3 + n + 5 * 14


def test_split_worked_examples():
    # the member limit cuts
    assert qp.series_predict_split([40] * 65, [7] * 65, 2) == [64, 1]
    assert qp.series_predict_split([1] * 200, [0] * 200, 8) == [64, 64, 64, 8]
    # the cap cuts: five members of 24.7 M doubles fill 123.4 of the 134.2 M, the sixth does not fit
    assert qp.series_predict_split([M] * 12, [M] * 12, 2) == [5, 5, 2]
    assert qp.series_predict_split([M] * 6, [M] * 6, 2) == [5, 1]
    # without test points fourteen fit (125.3 M), the fifteenth (134.26 M) does not
    assert qp.series_predict_split([M] * 15, [0] * 15, 2) == [14, 1]
    # the test points alone cut: 40 data points, 4 M test points each (15 doubles a point: 62.9 M)
    assert qp.series_predict_split([40] * 3, [4 * M] * 3, 2) == [2, 1]
    assert qp.series_predict_split([40] * 3, [4 * M] * 3, 2, want_var=False) == [2, 1]
    assert qp.series_predict_split([40] * 3, [4 * M] * 3, 2, False, False) == [2, 1]
    assert qp.series_predict_split([40] * 3, [3 * M] * 3, 2, True, False) == [3]      # 14 x 3 M x 3 = 132.1 M
    assert qp.series_predict_split([40] * 3, [3 * M] * 3, 2, True, True) == [2, 1]    # 15 x 3 M x 3 = 141.6 M
    # one series alone, J = 8, at its own data: 28 n and the rest
    assert qp.series_predict_split([4_000_000], [4_000_000], 8) == [1]
    assert qp.series_predict_split([5_000_000], [5_000_000], 8) is None
    assert qp.series_predict_split([40, 5_000_000], [7, 5_000_000], 8) is None  # a short neighbour does not help
    assert qp.series_predict_split([5_000_000], [0], 8) == [1]                   # its test points were the excess


def test_adding_a_series_never_merges_chains():
    rng = np.random.default_rng(0)
    for trial in range(40):
        J = int(rng.choice([1, 2, 8]))
        nb = int(rng.integers(1, 40))
        lengths = [int(n) for n in rng.choice([1, 40, 1025, 65_537, M], size=nb)]
        counts = [int(m) for m in rng.choice([0, 1, 300, M, 3 * M], size=nb)]
        before = qp.series_predict_split(lengths, counts, J)
        after = qp.series_predict_split(lengths + [M], counts + [int(rng.choice([0, M]))], J)
        assert before is not None and after is not None
        assert after[:len(before) - 1] == before[:-1] and after[len(before) - 1] >= before[-1]
        assert sum(after) == nb + 1 and all(c <= 64 for c in after)


# -- the test points ---------------------------------------------------------------------------------------------------------------
def test_test_points_are_concatenated_in_the_caller_s_order():
    x0, x2 = np.array([3.0, -1.0, 3.0]), np.array([[0.5], [np.nan]])
    offsets, xtest, at_data = pack_series_tests([4, 2, 5, 1], [x0, None, x2, np.empty(0)])
    assert offsets.dtype == np.int64 and list(offsets) == [0, 3, 5, 7, 7]
    assert at_data.dtype == np.int32 and list(at_data) == [0, 1, 0, 0]
    assert xtest.dtype == np.float64 and xtest.flags.c_contiguous and xtest.shape == (7,)
    assert np.array_equal(xtest[:3], x0) and np.array_equal(xtest[5:], x2[:, 0], equal_nan=True)
    assert not xtest[3:5].any()  # the member at its own data brings nothing
    offsets, xtest, at_data = pack_series_tests([4], [np.array([1, 2], dtype=np.float32)])
    assert list(offsets) == [0, 2] and xtest.dtype == np.float64 and not at_data.any()
    offsets, xtest, at_data = pack_series_tests([4, 2], [None, None])
    assert list(offsets) == [0, 4, 6] and at_data.all() and xtest.shape == (6,)


def test_wrong_test_points_name_the_series():
    with pytest.raises(ValueError, match=r"X_tests must hold one entry per series \(2\); got 3"):
        pack_series_tests([3, 2], [None, None, None])
    with pytest.raises(ValueError, match=r"X_tests\[1\] of series 1: .*shape \(N,\) or \(N, 1\); got \(2, 2\)"):
        pack_series_tests([3, 2], [np.zeros(3), np.zeros((2, 2))])


def test_means_follow_the_convention_of_predict_datasets():
    offsets = np.array([0, 3, 5, 5, 9])
    vec = np.arange(7.0)
    added = series_added_means([0.5, vec, None, vec], offsets, [None, 2.0, None, np.arange(4.0)], True)
    assert [a.shape for a in added] == [(3,), (2,), (0,), (4,)] and all(a.dtype == np.float64 for a in added)
    assert np.array_equal(added[0], [0.5] * 3) and np.array_equal(added[1], [2.0, 2.0])
    assert np.array_equal(added[3], np.arange(4.0))
    assert all(not a.any() for a in series_added_means(None, offsets, None, True))
    # a vector mean without its test values: an error with include_mean, nothing to add without
    with pytest.raises(ValueError, match=r"means\[1\] of series 1 is a vector: .*test_means\[1\] \(a scalar or \(2,\)\)"):
        series_added_means([0.5, vec, None, 1.0], offsets, None, True)
    assert not series_added_means([0.5, vec, None, 1.0], offsets, None, False)[1].any()
    with pytest.raises(ValueError, match=r"test_means\[0\] is given, but means\[0\] of series 0 is not a vector"):
        series_added_means([0.5, vec, None, 1.0], offsets, [1.0, None, None, None], True)
    with pytest.raises(ValueError, match=r"test_means\[3\] must have shape \(4,\) or be a scalar for series 3; got \(3,\)"):
        series_added_means([0.5, 0.0, None, vec], offsets, [None, None, None, np.zeros(3)], True)
    with pytest.raises(ValueError, match=r"test_means must hold one entry per series \(4\); got 2"):
        series_added_means(None, offsets, [None, None], True)
    with pytest.raises(ValueError, match=r"means must hold one entry per series \(4\); got 1"):
        series_added_means([1.0], offsets, None, True)


# -- sort by value, then locate ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, m", [(1, 7), (17, 1), (17, 300), (1025, 300), (40, 0)])
def test_sorting_by_value_then_locating_gives_sorted_intervals(n, m):
    t = qs.series(n)[0]
    x = np.array(qp.test_points(n, m))
    if m > 3:
        x[3] = np.nan
    if m > 5:
        x[5], x[4] = np.inf, -np.inf
    order, sidx = qp.sort_then_locate(t, x)
    want = np.searchsorted(t, x, side="right") - 1
    want[np.isnan(x)] = -1  # NaN compares false with every t_n: interval -1, and it sorts first
    assert sorted(order) == list(range(m)) and np.array_equal(sidx, want[order])
    assert np.all(np.diff(sidx) >= 0), "the emit pass walks sidx in step with the data"
    assert np.array_equal(np.sort(want, kind="stable"), sidx)
    if m > 3:
        assert order[0] == 3 and sidx[0] == -1
    finite = ~np.isnan(x)
    assert np.array_equal(want[finite], op.intervals(t, x[finite]))
    # ties keep the caller's order
    keys = np.where(np.isnan(x), -np.inf, x)[order]
    assert all(order[j] < order[j + 1] for j in range(m - 1) if keys[j] == keys[j + 1])


def test_the_planted_placements_are_there():
    n, m = 1025, 300
    t, x = qs.series(n)[0], qp.test_points(n, m)
    idx = op.intervals(t, x)
    e = qs.extent(n)
    edge = (e.nchunks - 1) * e.lc
    assert (e.lc, e.nchunks, edge) == (16, 65, 1024)
    assert (idx == -1).any() and (idx == n - 1).sum() >= 2 and np.isin(x, t).sum() >= 5
    assert len(np.unique(x)) < m and (idx == edge).any() and (idx == edge - 1).sum() >= 2
    assert np.any(np.diff(x) < 0)


# -- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tgp_hip.h").read_text(), flags=re.S)
    m = re.search(r"int\s+tgp_qsep_series_predict\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "include/tgp_hip.h does not declare tgp_qsep_series_predict"
    params = [p.strip() for p in m.group(1).split(",")]
    sig = _ffi.SIGNATURES["tgp_qsep_series_predict"]
    assert len(params) == len(sig) == 17
    scalars = {i for i, p in enumerate(params) if "*" not in p}
    assert scalars == {2, 4} and all(params[i].startswith("int32_t ") and sig[i] is C.c_int32 for i in scalars)
    assert hasattr(_ffi.load_library(), "tgp_qsep_series_predict")
    assert _ffi.ABI_VERSION == 6 and "#define TGP_ABI_VERSION 6" in (ROOT / "include" / "tgp_hip.h").read_text()


def test_the_public_names():
    import tinygp_amd
    from tinygp_amd.solvers import QuasisepSeriesSet, QuasisepSolver

    assert callable(tinygp_amd.predict_series) and hasattr(QuasisepSeriesSet, "predict")
    assert tinygp_amd.predict_series is tinygp_amd.solvers.quasisep.predict_series
    assert not hasattr(QuasisepSolver, "predict_batch")
