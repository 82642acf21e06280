"""Sets of series, each on coordinates of its own (``QuasisepSeriesSet`` / ``tgp_qsep_series_logprob``): every member
against the sequential oracle and, to the bit, against the device's single call on a fresh ``QuasisepSolver``, whatever
the set's size, the member's position, the other members' lengths and the split into launch chains."""
import ctypes as C
import functools

import numpy as np
import pytest

import tinygp_amd
from tinygp_amd import GaussianProcess, _ffi
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.noise import Diagonal
from tinygp_amd.solvers import QuasisepSeriesSet, QuasisepSolver
from tinygp_amd.solvers.quasisep import pack_series

import _quasisep_np as o
import _quasisep_series as qs
from _quasisep_cases import CASES
from _quasisep_grad_batch import member, member_noise

pytestmark = pytest.mark.gpu


def _member(name, b):
    return member(CASES, q, name, b)


def _single_call(k, t, noise, r):
    """The device's single call on a fresh solver."""
    s = QuasisepSolver(k, t, Diagonal(noise), assume_sorted=True)
    try:
        return float(s.log_probability(r))
    finally:
        s.close()


@functools.lru_cache(maxsize=None)
def _single(name, n, b):
    """Member b of case ``name`` on the series of length n, alone; computed once for every set that holds it."""
    t, noise, r = qs.series(n)
    return _single_call(_member(name, b), t, member_noise(noise, b), r)


@functools.lru_cache(maxsize=None)
def _oracle(name, n, b):
    t, noise, r = qs.series(n)
    return float(o.log_probability(_member(name, b), t, member_noise(noise, b), r))


def _inputs(name, lengths, bs):
    """Member i: the series of length lengths[i] under kernel and noise number bs[i]."""
    data = [qs.series(n) for n in lengths]
    return ([_member(name, b) for b in bs], [d[0] for d in data],
            [member_noise(d[1], b) for d, b in zip(data, bs)], [d[2] for d in data])


def _evaluate(name, lengths, bs):
    ks, ts, nz, rs = _inputs(name, lengths, bs)
    s = QuasisepSeriesSet(ts)
    try:
        got, info = s.log_probability(ks, rs, nz, return_info=True)
    finally:
        s.close()
    assert got.shape == (len(lengths),) and got.dtype == np.float64 and not info.any()
    return got


def _raw(s, kernels, ys, diags):
    """The low-level call: ``(out, info, nchains)``."""
    leaves, smap, h, P, noise, resid = pack_series(s.lengths, kernels, ys, diags)
    nb = len(s)
    info, out, nchains = np.zeros(nb, dtype=np.int32), np.empty(nb), C.c_int32(-1)
    _ffi.check(_ffi.lib().tgp_qsep_series_logprob(
        s._handle, _ffi.ptr(leaves), leaves.shape[1], _ffi.ptr(smap), h.shape[1], _ffi.ptr(h), _ffi.ptr(P),
        _ffi.ptr(noise), _ffi.ptr(resid), _ffi.ptr(info), _ffi.ptr(out), C.byref(nchains)), "tgp_qsep_series_logprob")
    return out, info, nchains.value


# -- 1. every scan edge in one set ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", qs.EDGE_CASES)
def test_every_scan_edge_in_one_set(name, reverse):
    """One- and two-level scans, 64 and 65 chunks and last chunks of one step side by side; a length keeps its kernel
    and noise when the order is reversed, so both orders are held to the same references."""
    order = list(range(len(qs.EDGE_LENGTHS)))[::-1 if reverse else 1]
    lengths = [qs.EDGE_LENGTHS[b] for b in order]
    got = _evaluate(name, lengths, order)
    for v, n, b in zip(got, lengths, order):
        oracle, single = _oracle(name, n, b), _single(name, n, b)
        print(f"{name} n={n} member {b}: set {v!r} single {single!r} oracle {oracle!r}")
        assert v == pytest.approx(oracle, rel=1e-8)
        assert v == single


# -- 2. mixed chunk lengths and scan depths ------------------------------------------------------------------------------------
def test_the_mixed_lengths_cut_as_stated():
    """Lengths [65 537, 40, 262 145, 1]: chunks of 32, 16, 128 and 16 steps, scans of two, one, two and one level.
    (The chunk rule doubles lc while 4096 lc < n, so 262 145 points get 2 049 chunks of 128, not 4 097 of 64: a scan of
    three levels needs more than 4 096 chunks of 256, which DEEP_LENGTHS adds with 2^20 + 1 points: 4 097 -> 65 -> 2.)"""
    assert [qs.extent(n).lc for n in qs.MIXED_LENGTHS] == [32, 16, 128, 16]
    assert [len(qs.extent(n).levels) for n in qs.MIXED_LENGTHS] == [2, 1, 2, 1]
    assert qs.extent(qs.DEEP_LENGTHS[0]) == qs.Extent(256, 4097, (4097, 65, 2))
    assert [len(qs.extent(n).levels) for n in qs.DEEP_LENGTHS] == [3, 1, 2, 1]


@pytest.mark.parametrize("name", qs.MIXED_CASES)
def test_mixed_chunk_lengths_and_depths(name):
    got = _evaluate(name, qs.MIXED_LENGTHS, range(4))
    for b, n in enumerate(qs.MIXED_LENGTHS):
        assert got[b] == _single(name, n, b), (n, got[b])
    for b, n in enumerate(qs.MIXED_LENGTHS[:2]):
        assert got[b] == pytest.approx(_oracle(name, n, b), rel=1e-8)


@pytest.mark.parametrize("name", qs.MIXED_CASES)
def test_one_two_and_three_scan_levels_in_one_chain(name):
    got = _evaluate(name, qs.DEEP_LENGTHS, range(4))
    for b, n in enumerate(qs.DEEP_LENGTHS):
        assert got[b] == _single(name, n, b), (n, got[b])


# -- 3. position and company do not matter ------------------------------------------------------------------------------------
def test_position_and_company_do_not_matter():
    name, n = qs.PROBE_CASE, qs.PROBE_LENGTH
    want = _single(name, n, 7)
    for nb in (2, 5, 65):
        for pos in sorted({0, nb // 2, nb - 1}):
            lengths = [qs.COMPANY_LENGTHS[b % 4] for b in range(nb)]
            bs = [b % 11 for b in range(nb)]
            lengths[pos], bs[pos] = n, 7
            got = _evaluate(name, lengths, bs)
            assert got[pos] == want, (nb, pos, got[pos], want)


# -- 4. chains ----------------------------------------------------------------------------------------------------------------------
def test_sixty_five_series_run_as_two_chains():
    name, n, nb = "matern32", 40, 65
    bs = [b % 13 for b in range(nb)]
    ks, ts, nz, rs = _inputs(name, [n] * nb, bs)
    assert qs.series_split([n] * nb, 2) == [64, 1]
    s = QuasisepSeriesSet(ts)
    out, info, nchains = _raw(s, ks, rs, nz)
    s.close()
    assert nchains == 2 and not info.any() and np.all(np.isfinite(out))
    for b in (62, 63, 64):
        assert out[b] == _single(name, n, bs[b]), b


def test_the_cap_cuts_the_chain():
    """Ten series of 2^20 points with J = 8: about 13.7 M doubles each, nine of which fit 2^27."""
    name, n, nb = "celerite4", 1 << 20, 10
    chains = qs.series_split([n] * nb, 8)
    assert chains == [9, 1]
    ks, ts, nz, rs = _inputs(name, [n] * nb, range(nb))
    s = QuasisepSeriesSet(ts, assume_sorted=True)
    out, info, nchains = _raw(s, ks, rs, nz)
    s.close()
    assert nchains == len(chains) and not info.any() and np.all(np.isfinite(out))
    for b in (0, nb - 1):
        assert out[b] == _single(name, n, b), b


# -- 5. failure stays in its member ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 1, 2])
def test_failure_stays_in_its_member(pos):
    """noise = -10 at local step 5 of one series: h^T P^- h <= k(0) = 1.44 (1 + 0.04 b)^2, so that pivot is negative."""
    name, lengths = "matern32", [300, 1025, 64]
    lengths = lengths[-pos:] + lengths[:-pos]  # the series of 1025 points fails: in the middle, last, first
    bad = lengths.index(1025)
    ks, ts, nz, rs = _inputs(name, lengths, range(3))
    nz[bad] = nz[bad].copy()
    nz[bad][5] = -10.0
    s = QuasisepSeriesSet(ts)
    got, info = s.log_probability(ks, rs, nz, return_info=True)
    raw, _, _ = _raw(s, ks, rs, nz)
    s.close()
    assert list(info) == [6 if b == bad else 0 for b in range(3)]
    assert got[bad] == -np.inf and np.isnan(raw[bad])
    for b in range(3):
        if b != bad:
            assert got[b] == raw[b] == _single(name, lengths[b], b), b


# -- 6. kernels ------------------------------------------------------------------------------------------------------------------
def test_one_shared_kernel_equals_equal_copies():
    name, lengths = "m32cos_plus_sho", [17, 1025, 300]
    _, ts, nz, rs = _inputs(name, lengths, range(3))
    s = QuasisepSeriesSet(ts)
    shared = s.log_probability(_member(name, 2), rs, nz)
    copies = s.log_probability([_member(name, 2) for _ in lengths], rs, nz)
    s.close()
    assert np.all(np.isfinite(shared)) and np.array_equal(shared, copies)
    t, _, r = qs.series(1025)
    assert shared[1] == _single_call(_member(name, 2), t, nz[1], r)


def test_damping_regimes_share_one_set():
    ks = [q.SHO(omega=1.5, quality=quality) for quality in (3.0, 0.5, 0.3)]
    assert len({int(k._lower_ssm().leaves[0, 0]) for k in ks}) == 3
    lengths = [1025, 40, 300]
    data = [qs.series(n) for n in lengths]
    s = QuasisepSeriesSet([d[0] for d in data])
    got, info = s.log_probability(ks, [d[2] for d in data], [d[1] for d in data], return_info=True)
    s.close()
    assert not info.any()
    for v, k, (t, noise, r) in zip(got, ks, data):
        assert v == pytest.approx(float(o.log_probability(k, t, noise, r)), rel=1e-8)
        assert v == _single_call(k, t, noise, r)


# -- 7. the handle ---------------------------------------------------------------------------------------------------------------
def test_the_handle_serves_call_after_call():
    lengths = [1025, 17, 300]
    _, ts, nz, rs = _inputs("matern32", lengths, range(3))
    first = [_member("matern32", b) for b in range(3)]        # J = 2
    second = [_member("celerite4", b) for b in range(3)]      # J = 8: the table is cut again

    def fresh(ks):
        s = QuasisepSeriesSet(ts)
        try:
            return s.log_probability(ks, rs, nz)
        finally:
            s.close()

    t, noise, r = qs.series(4097)
    solver = QuasisepSolver(_member("m32cos_plus_sho", 0), t, Diagonal(noise))
    before = solver.log_probability(r)
    s = QuasisepSeriesSet(ts)
    a = s.log_probability(first, rs, nz)
    between = solver.log_probability(r)
    b = s.log_probability(second, rs, nz)
    again = s.log_probability(first, rs, nz)
    s.close()
    after = solver.log_probability(r)
    solver.close()
    assert np.array_equal(a, fresh(first)) and np.array_equal(b, fresh(second)) and np.array_equal(again, a)
    assert before == between == after == _single("m32cos_plus_sho", 4097, 0)
    with pytest.raises(ValueError, match="closed"):
        s.log_probability(first, rs, nz)


# -- 8. the public function -------------------------------------------------------------------------------------------------------
def test_public_function_equals_separate_gps():
    name, lengths = "m32cos_plus_sho", [1000, 33, 257, 1]
    ks, ts, _, ys = _inputs(name, lengths, range(4))
    diags = [0.1, 0.15, qs.series(257)[1], 0.05]
    for means in ([0.0, 0.3, -0.2, 1.5], [0.1 * np.cos(t) for t in ts], None):
        got = tinygp_amd.log_probability_series(ks, ts, ys, diags=diags, means=means)
        assert got.shape == (4,) and got.dtype == np.float64
        for b in range(4):
            mean = {} if means is None else {"mean": means[b]} if np.ndim(means[b]) == 0 else {"mean_value": means[b]}
            want = GaussianProcess(ks[b], ts[b], diag=diags[b], **mean).log_probability(ys[b])
            assert got[b] == want, b


# -- 9. argument errors of the C entry points ---------------------------------------------------------------------------------
def _create(offsets, t):
    h = C.c_void_p()
    offsets = None if offsets is None else np.asarray(offsets, dtype=np.int64)
    _ffi.check(_ffi.lib().tgp_qsep_series_create(_ffi.default_ctx().handle, 0 if offsets is None else len(offsets) - 1,
                                                 _ffi.ptr(offsets), _ffi.ptr(t), C.byref(h)), "tgp_qsep_series_create")
    return h


def test_create_refuses_bad_offsets_and_null_arrays():
    t = np.arange(6.0)
    for offsets, message in (([0, 3, 3], "series 1 is empty"), ([0, 3, 2], "must not decrease"),
                             ([1, 3, 6], "start at 0"), ([0], "at least one series")):
        with pytest.raises(ValueError, match=message):
            _create(offsets, t)
    with pytest.raises(ValueError, match="null argument"):
        _create([0, 3, 6], None)
    h = C.c_void_p()
    with pytest.raises(ValueError, match="null argument"):
        _ffi.check(_ffi.lib().tgp_qsep_series_create(_ffi.default_ctx().handle, 2, None, _ffi.ptr(t), C.byref(h)))
    h = _create([0, 3, 6], t)  # and the same arrays are accepted when they are right
    assert h.value
    _ffi.lib().tgp_qsep_series_destroy(h)


def test_logprob_refuses_null_arrays():
    ks, ts, nz, rs = _inputs("matern32", [17, 40], range(2))
    s = QuasisepSeriesSet(ts)
    leaves, smap, h, P, noise, resid = pack_series(s.lengths, ks, rs, nz)
    info, out = np.zeros(2, dtype=np.int32), np.empty(2)
    full = [leaves, smap, h, P, noise, resid, info, out]
    for missing in range(len(full)):
        a = [None if i == missing else x for i, x in enumerate(full)]
        with pytest.raises(ValueError, match="null"):
            _ffi.check(_ffi.lib().tgp_qsep_series_logprob(
                s._handle, _ffi.ptr(a[0]), leaves.shape[1], _ffi.ptr(a[1]), h.shape[1], _ffi.ptr(a[2]), _ffi.ptr(a[3]),
                _ffi.ptr(a[4]), _ffi.ptr(a[5]), _ffi.ptr(a[6]), _ffi.ptr(a[7]), None))
    got = s.log_probability(ks, rs, nz)  # the refusals left the set usable
    s.close()
    assert [got[b] for b in range(2)] == [_single("matern32", n, b) for b, n in enumerate([17, 40])]


def test_a_series_beyond_the_cap_is_refused():
    """12 000 000 points with J = 8 need more than 12 n = 1.44 * 10^8 doubles, the cap is 2^27 = 1.34 * 10^8; the check
    precedes every allocation of the chain's buffer, and a short neighbour does not help.  With J = 1 the set fits."""
    n = 12_000_000
    assert qs.series_split([40, n], 8) is None and qs.series_split([40, n], 1) == [2]
    t = np.arange(n, dtype=np.float64)
    s = QuasisepSeriesSet([t[:40], t], assume_sorted=True)
    with pytest.raises(ValueError, match=r"series 1 \(n = 12000000\) .*exceeds its cap"):
        s.log_probability(_member("celerite4", 0), [np.zeros(40), np.zeros(n)], [1.0, 1.0])
    got, info = s.log_probability(_member("exp", 0), [np.zeros(40), np.zeros(n)], [1.0, 1.0], return_info=True)
    s.close()
    assert not info.any() and np.all(np.isfinite(got))
