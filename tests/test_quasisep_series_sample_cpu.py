"""Posterior draws for sets of series, host side: the mirrored need and split rule with hand-computed cases, the packing of
the test points and the normals with their error messages, the front end's draw order against ``GaussianProcess``'s, a
closed set and the entry point's declaration."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import tinygp_amd
from tinygp_amd import _ffi
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.solvers import QuasisepSeriesSet
from tinygp_amd.solvers import quasisep as solver_module
from tinygp_amd.solvers.quasisep import pack_series_normals, pack_series_sample_tests

import _quasisep_series as qs
import _quasisep_series_sample as ss
from _quasisep_series_sample import Chain

ROOT = Path(__file__).resolve().parent.parent
M = 1 << 20


# -- the mirrored rule -----------------------------------------------------------------------------------------------------------
def test_need_of_a_short_and_a_long_series():
    # 40 points and 5 test points, J = 2: 3 chunks of the data and of the 45 grid points, S4 = 3 + 3 either
    assert qs.need(40, 2) == 40 * 6 + 256 * 6 + 9 + 3 == 1788
    assert ss.fixed(40, 5, 2) == 1788 + 13 + 3 * 5 + 2 * 45 == 1906
    assert ss.per_cols(40, 5, 2, 1) == 45 * 2 + 2 * 40 + 5 + 192 * 6 == 1327
    assert ss.per_cols(40, 5, 2, 9) == 9 * 175 + 2 * 192 * 6 == 3879        # two column groups
    assert ss.per_cols(40, 5, 2, 9, want_test=False) == 9 * 170 + 2 * 192 * 6
    assert ss.per_cols(40, 5, 1, 1) == ss.per_cols(40, 5, 2, 1)             # J counts as at least 2: z and alpha fit
    assert ss.per_cols(40, 5, 8, 1) == 45 * 8 + 2 * 40 + 5 + 192 * 6
    # 2^20 points, no test points, J = 2: 4096 chunks of 256, S4 = 4096 + 64 + 1 + 1
    assert ss.fixed(M, 0, 2) == 6 * M + 256 * 4162 + 3 * 4096 + 3 + 13 + 2 * M == 9_466_384
    assert ss.per_cols(M, 0, 2, 1) == 4 * M + 192 * 4162 == 4_993_408
    assert ss.BUDGET == (1 << 27) - 64 * 141 == 134_208_704


def test_the_larger_pyramid_sets_the_work_space():
    """65 536 points are 4096 chunks of 16 (S4 = 4096 + 64 + 2); one test point more and the grid has 2049 chunks of 32
    (S4 = 2049 + 33 + 2): the data's pyramid is the larger.  1000 points with 25 test points: 63 chunks against 65."""
    assert qs.extent(65_536) == (16, 4096, (4096, 64)) and qs.extent(65_537) == (32, 2049, (2049, 33))
    assert ss.per_cols(65_536, 1, 2, 8) == 8 * (65_537 * 2 + 2 * 65_536 + 1) + 192 * 4162
    assert qs.extent(1000).levels == (63,) and qs.extent(1025).levels == (65, 2)
    assert ss.per_cols(1000, 25, 2, 8) == 8 * (1025 * 2 + 2000 + 25) + 192 * (65 + 2 + 2)


def test_split_hand_computed_cases():
    # the member limit cuts; 9 columns fit in one pass
    assert ss.series_sample_split([40] * 64, [5] * 64, 2, 9) == [Chain(64, 9, 1)]
    assert ss.series_sample_split([40] * 65, [5] * 65, 2, 9) == [Chain(64, 9, 1), Chain(1, 9, 1)]
    assert ss.series_sample_split([40] * 65, [5] * 65, 2, 65) == [Chain(64, 64, 2), Chain(1, 64, 2)]
    # a member ends a chain by the cap: with one column a series of 2^20 points takes 9 466 384 + 4 993 408 = 14 459 792
    # doubles; nine are 130.1 M of the 134.2 M, the tenth does not fit
    assert ss.series_sample_split([M] * 10, [0] * 10, 2, 64) == [Chain(9, 1, 64), Chain(1, 24, 3)]
    # columns cut to a multiple of 8.  One member: 124 742 320 doubles are left after its fixed part; 24 columns take
    # 24 x 4 M + 3 x 799 104 = 103 060 608, 32 columns 136.6 M.  Two members: 115 275 936 are left; 8 columns take
    # 2 (8 x 4 M + 799 104) = 68 707 072, 16 columns 137.4 M
    assert ss.series_sample_split([M], [0], 2, 64) == [Chain(1, 24, 3)]
    assert ss.series_sample_split([M], [0], 2, 25) == [Chain(1, 25, 1)]   # 25 x 4 M + 4 x 799 104 = 108.1 M fit
    assert ss.series_sample_split([M], [0], 2, 30) == [Chain(1, 24, 2)]   # 30 x 4 M alone do not: down to 24
    assert ss.series_sample_split([M] * 2, [0] * 2, 2, 64) == [Chain(2, 8, 8)]
    # and to fewer than 8, by ones.  Four members: 96 343 168 are left; 6 columns take 4 (6 x 4 M + 799 104) = 103.9 M,
    # 5 columns 87 082 496
    assert ss.series_sample_split([M] * 4, [0] * 4, 2, 64) == [Chain(4, 5, 13)]
    assert ss.series_sample_split([M] * 4, [0] * 4, 2, 5) == [Chain(4, 5, 1)]
    assert ss.series_sample_split([M] * 4, [0] * 4, 2, 3) == [Chain(4, 3, 1)]
    # a member refused alone: 8 x 2^20 points at J = 8 take 126.1 M + 90.3 M with one column; a short neighbour does not help
    assert ss.series_sample_split([8 * M], [0], 8, 3) is None
    assert ss.series_sample_split([40, 8 * M], [5, 0], 8, 3) is None
    assert ss.series_sample_split([8 * M], [0], 2, 3) == [Chain(1, 1, 3)]  # 75.7 M + 39.9 M per column: one fits, two do not


def test_the_split_is_a_function_of_its_arguments_alone():
    rng = np.random.default_rng(0)
    for trial in range(30):
        J, nrhs = int(rng.choice([1, 2, 8])), int(rng.choice([1, 8, 9, 65]))
        nb = int(rng.integers(1, 40))
        lengths = [int(n) for n in rng.choice([1, 40, 1025, 65_537, M], size=nb)]
        counts = [int(m) for m in rng.choice([0, 1, 300, M], size=nb)]
        chains = ss.series_sample_split(lengths, counts, J, nrhs)
        assert chains is not None and sum(c.members for c in chains) == nb
        b0 = 0
        for c in chains:
            assert 1 <= c.members <= 64 and 1 <= c.cols <= min(nrhs, 64) and c.passes == -(-nrhs // c.cols)
            assert c.cols == min(nrhs, 64) or c.cols % 8 == 0 or c.cols < 8
            part = range(b0, b0 + c.members)
            total = lambda k: sum(ss.fixed(lengths[b], counts[b], J) + ss.per_cols(lengths[b], counts[b], J, k)
                                  for b in part)  # noqa: E731
            assert total(c.cols) <= ss.BUDGET
            b0 += c.members
        # dropping the test side never needs more
        lean = ss.series_sample_split(lengths, counts, J, nrhs, want_test=False)
        assert len(lean) <= len(chains)


# -- packing ---------------------------------------------------------------------------------------------------------------------
def test_a_member_at_its_own_points_brings_no_test_points():
    x0, x2 = np.array([3.0, -1.0, 3.0]), np.array([[0.5], [0.25]])
    offsets, xtest, at_data = pack_series_sample_tests([4, 2, 5, 1], [x0, None, x2, np.empty(0)])
    assert offsets.dtype == np.int64 and list(offsets) == [0, 3, 3, 5, 5]
    assert at_data.dtype == np.int32 and list(at_data) == [0, 1, 0, 0]
    assert xtest.dtype == np.float64 and xtest.flags.c_contiguous and np.array_equal(xtest, [3.0, -1.0, 3.0, 0.5, 0.25])


def test_wrong_test_points_name_the_series():
    with pytest.raises(ValueError, match=r"X_tests must hold one entry per series \(2\); got 3"):
        pack_series_sample_tests([3, 2], [None, None, None])
    with pytest.raises(ValueError, match=r"X_tests\[1\] of series 1: .*shape \(N,\) or \(N, 1\); got \(2, 2\)"):
        pack_series_sample_tests([3, 2], [np.zeros(3), np.zeros((2, 2))])
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match=r"X_tests\[2\] of series 2 must be finite"):
            pack_series_sample_tests([3, 2, 4], [np.zeros(3), None, np.array([0.0, bad, 1.0])])


def test_normals_are_concatenated_member_after_member():
    rng = np.random.default_rng(1)
    lengths, counts, J, R = [4, 2, 5], [3, 0, 1], 2, 3
    xi = [rng.standard_normal((n + m, J, R)) for n, m in zip(lengths, counts)]
    eps = [rng.standard_normal((n, R)) for n in lengths]
    xi_c, eps_c, got_R, one = pack_series_normals(lengths, counts, J, xi, eps)
    assert (got_R, one) == (R, False) and xi_c.shape == (15 * J, R) and eps_c.shape == (11, R)
    assert xi_c.flags.c_contiguous and eps_c.flags.c_contiguous and xi_c.dtype == eps_c.dtype == np.float64
    assert np.array_equal(xi_c[:14], xi[0].reshape(14, R)) and np.array_equal(xi_c[18:], xi[2].reshape(12, R))
    assert np.array_equal(xi_c[14 + 1 * J + 1], xi[1][1, 1])  # row (point 1, state 1) of member 1
    assert np.array_equal(eps_c[4:6], eps[1])
    # all one-dimensional: R = 1
    xi_c, eps_c, got_R, one = pack_series_normals(lengths, counts, J, [a[:, :, 0] for a in xi], [e[:, 0] for e in eps])
    assert (got_R, one) == (1, True) and xi_c.shape == (30, 1) and np.array_equal(eps_c[:, 0], np.concatenate(eps)[:, 0])


def test_wrong_normals_name_the_member():
    lengths, counts, J = [4, 2], [3, 0], 2
    xi, eps = [np.zeros((7, 2, 3)), np.zeros((2, 2, 3))], [np.zeros((4, 3)), np.zeros((2, 3))]
    with pytest.raises(ValueError, match=r"xi and eps must hold one entry per series \(2\); got 1 and 2"):
        pack_series_normals(lengths, counts, J, xi[:1], eps)
    with pytest.raises(ValueError, match=r"xi\[1\] must have shape \(2, 2, 3\) for series 1.*; got \(3, 2, 3\)"):
        pack_series_normals(lengths, counts, J, [xi[0], np.zeros((3, 2, 3))], eps)
    with pytest.raises(ValueError, match=r"xi\[1\] must have shape \(2, 2, 3\) for series 1.*; got \(2, 2, 4\)"):
        pack_series_normals(lengths, counts, J, [xi[0], np.zeros((2, 2, 4))], eps)
    with pytest.raises(ValueError, match=r"xi\[0\] must have shape \(7, 2, 3\) for series 0; got \(7, 3, 3\)"):
        pack_series_normals(lengths, counts, J, [np.zeros((7, 3, 3)), xi[1]], eps)
    with pytest.raises(ValueError, match=r"eps\[1\] must have shape \(2, 3\) for series 1 .*; got \(2,\)"):
        pack_series_normals(lengths, counts, J, xi, [eps[0], np.zeros(2)])
    with pytest.raises(ValueError, match=r"xi\[1\] must have shape \(2, 2\) for series 1 \(as xi\[0\] has 2 dimensions\)"):
        pack_series_normals(lengths, counts, J, [np.zeros((7, 2)), xi[1]], [np.zeros(4), np.zeros(2)])
    with pytest.raises(ValueError, match=r"R >= 1; got \(7, 2, 0\)"):
        pack_series_normals(lengths, counts, J, [np.zeros((7, 2, 0)), np.zeros((2, 2, 0))],
                            [np.zeros((4, 0)), np.zeros((2, 0))])


# -- the front end's draw order ----------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for the set: keeps what ``sample_conditional_series`` hands over and answers with zeros."""
    calls = []

    def __init__(self, Xs):
        self.lengths = np.array([len(x) for x in Xs], dtype=np.int64)
        self.closed = False

    def __len__(self):
        return len(self.lengths)

    def sample_conditional(self, kernels, ys, diags, X_tests, *, xi, eps, means=None):
        _Recorder.calls.append((self, xi, eps))
        counts = [n if X is None else len(X) for n, X in zip(self.lengths, X_tests)]
        return np.zeros(len(self)), [np.zeros((m, xi[0].shape[2])) for m in counts]

    def close(self):
        self.closed = True


def test_the_normals_are_drawn_in_gaussian_process_s_order(monkeypatch):
    """Per member, in member order: xi (N + M, J, R), then eps (N, R) -- member 0 gets exactly what
    ``GaussianProcess.sample_conditional`` draws from a fresh generator with the same seed."""
    monkeypatch.setattr(solver_module, "QuasisepSeriesSet", _Recorder)
    _Recorder.calls.clear()
    k = q.Matern32(scale=0.8) + q.Celerite(1.0, 0.2, 0.5, 1.5)  # J = 4
    Xs = [np.arange(5.0), np.arange(3.0), np.arange(4.0)]
    X_tests = [np.array([0.5, 7.0]), None, np.empty(0)]
    values, samples = tinygp_amd.sample_conditional_series(k, Xs, [np.zeros(len(x)) for x in Xs], X_tests,
                                                           diags=[0.1] * 3, key=3, shape=(2, 3), means=[1.5, 0.0, 0.0])
    (fake, xi, eps), = _Recorder.calls
    assert fake.closed
    rng = np.random.default_rng(3)
    for b, (n, m) in enumerate([(5, 2), (3, 0), (4, 0)]):
        assert np.array_equal(xi[b], rng.standard_normal((n + m, 4, 6)))
        assert np.array_equal(eps[b], rng.standard_normal((n, 6)))
    assert [s.shape for s in samples] == [(2, 3, 2), (2, 3, 3), (2, 3, 0)]
    assert np.all(samples[0] == 1.5) and not samples[1].any()   # the scalar mean is added, to its own member only
    # a generator is taken as it is, and normals= replaces the draw
    _Recorder.calls.clear()
    given = [(np.ones((7, 4, 1)), np.ones((5, 1))), (np.ones((3, 4, 1)), np.ones((3, 1))), (np.ones((4, 4, 1)),) * 2]
    tinygp_amd.sample_conditional_series(k, Xs, Xs, X_tests, diags=[0.1] * 3, key=None, normals=given)
    assert _Recorder.calls[0][1][0] is given[0][0] and _Recorder.calls[0][2][1] is given[1][1]
    with pytest.raises(ValueError, match=r"normals must hold one \(xi, eps\) pair per series \(3\); got 2"):
        tinygp_amd.sample_conditional_series(k, Xs, Xs, X_tests, diags=[0.1] * 3, key=None, normals=given[:2])
    with pytest.raises(ValueError, match=r"X_tests must hold one entry per series \(3\); got 1"):
        tinygp_amd.sample_conditional_series(k, Xs, Xs, [None], diags=[0.1] * 3, key=0)
    with pytest.raises(ValueError, match=r"means\[1\] of series 1 is a vector: .*test_means\[1\] \(a scalar or \(3,\)\)"):
        tinygp_amd.sample_conditional_series(k, Xs, Xs, X_tests, diags=[0.1] * 3, key=0, means=[0.0, np.zeros(3), 0.0])
    assert all(f.closed for f, _, _ in _Recorder.calls)


# -- a closed set ------------------------------------------------------------------------------------------------------------------
def test_a_closed_set_refuses():
    s = QuasisepSeriesSet.__new__(QuasisepSeriesSet)  # what close() leaves behind, without a device
    s._handle = None
    with pytest.raises(ValueError, match="this QuasisepSeriesSet has been closed"):
        s.sample_conditional(q.Matern32(scale=1.0), [np.zeros(3)], [0.1], [None], xi=[np.zeros((3, 2))],
                             eps=[np.zeros(3)])


# -- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_entry_point():
    header = (ROOT / "include" / "tgp_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int\s+tgp_qsep_series_sample\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "include/tgp_hip.h does not declare tgp_qsep_series_sample"
    params = [p.strip() for p in m.group(1).split(",")]
    sig = _ffi.SIGNATURES["tgp_qsep_series_sample"]
    assert len(params) == len(sig) == 21
    scalars = {i: p for i, p in enumerate(params) if "*" not in p}
    assert set(scalars) == {2, 4, 12}
    assert all(scalars[i].startswith("int32_t ") and sig[i] is C.c_int32 for i in (2, 4))
    assert scalars[12].startswith("int64_t ") and sig[12] is C.c_int64
    assert hasattr(_ffi.load_library(), "tgp_qsep_series_sample")
    assert _ffi.ABI_VERSION == 6 and "#define TGP_ABI_VERSION 6" in header


def test_the_public_names():
    assert tinygp_amd.sample_conditional_series is solver_module.sample_conditional_series
    assert hasattr(QuasisepSeriesSet, "sample_conditional")
