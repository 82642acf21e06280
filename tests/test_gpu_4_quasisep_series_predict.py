"""Prediction for sets of series (``QuasisepSeriesSet.predict`` / ``tgp_qsep_series_predict``): every member to the bit
against the device's single calls on a fresh ``QuasisepSolver`` -- ``log_probability`` and ``predict_mean_var`` at that
member's test points -- whatever the set's size, the member's position, the other members' lengths and test points and
the split into launch chains; against the sequential oracle (``_quasisep_predict_np.predict``, at small N also its
``dense``) at the project's posterior bar, rtol = atol = 5e-7 (README "Parity")."""
import ctypes as C
import functools

import numpy as np
import pytest

import tinygp_amd
from tinygp_amd import _ffi
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.noise import Diagonal
from tinygp_amd.solvers import QuasisepSeriesSet, QuasisepSolver
from tinygp_amd.solvers.quasisep import pack_series, pack_series_tests

import _quasisep_predict_np as op
import _quasisep_series as qs
import _quasisep_series_predict as qp
from _quasisep_cases import CASES
from _quasisep_grad_batch import member, member_noise

pytestmark = pytest.mark.gpu

BAR = dict(rtol=5e-7, atol=5e-7)
worst = {"mean": 0.0, "var": 0.0}  # the largest differences from the oracle that this run met


def _member(name, b):
    return member(CASES, q, name, b)


def _single_call(k, t, noise, r, xt, return_var=True):
    """The device's single calls on a fresh solver: ``(value, info, mean, var)``; ``xt`` None: at the data."""
    s = QuasisepSolver(k, t, Diagonal(noise), assume_sorted=True)
    try:
        v = float(s.log_probability(r))
        out = s.predict_mean_var(r, t if xt is None else xt, return_var=return_var)
        mean, var = out if return_var else (out, None)
        return v, int(s.info), np.asarray(mean), None if var is None else np.asarray(var)
    finally:
        s.close()


def _points(n, m, nan=False):
    """Member test points: ``None`` (its own data), or ``test_points(n, m)``, one of them NaN if asked."""
    if m is None:
        return None
    x = qp.test_points(n, m)
    if nan:
        x = np.array(x)
        x[m // 2] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def _single(name, n, b, m, nan=False):
    """Member b of case ``name`` on the series of length n at its m test points, alone; computed once."""
    t, noise, r = qs.series(n)
    out = _single_call(_member(name, b), t, member_noise(noise, b), r, _points(n, m, nan))
    for a in out[2:]:
        a.setflags(write=False)
    return out


def _inputs(name, lengths, bs):
    """Member i: the series of length lengths[i] under kernel and noise number bs[i]."""
    data = [qs.series(n) for n in lengths]
    return ([_member(name, b) for b in bs], [d[0] for d in data],
            [member_noise(d[1], b) for d, b in zip(data, bs)], [d[2] for d in data])


def _same(got, i, want, tag=""):
    """Member i of a set's result has the bits of the single calls'."""
    v, _, mean, var = want
    assert got[0][i] == v, (tag, i, got[0][i], v)
    assert got[1][i].dtype == np.float64 and got[1][i].shape == mean.shape, (tag, i)
    assert np.array_equal(got[1][i], mean, equal_nan=True), (tag, i, "mean")
    if got[2] is not None:
        assert got[2][i].dtype == np.float64 and np.array_equal(got[2][i], var, equal_nan=True), (tag, i, "variance")


def _evaluate(name, lengths, bs, xts, **kw):
    ks, ts, nz, rs = _inputs(name, lengths, bs)
    s = QuasisepSeriesSet(ts, assume_sorted=True)
    try:
        values, mus, variances, info = s.predict(ks, rs, nz, xts, return_info=True, **kw)
    finally:
        s.close()
    assert values.shape == (len(lengths),) and values.dtype == np.float64 and not info.any()
    assert len(mus) == len(lengths) and (variances is None or len(variances) == len(lengths))
    return values, mus, variances


def _raw(s, kernels, ys, diags, xts, *, mean=True, var=True):
    """The low-level call: ``(out, info, mean, var, nchains, test_offsets)``."""
    leaves, smap, h, P, noise, resid = pack_series(s.lengths, kernels, ys, diags)
    offsets, xtest, at_data = pack_series_tests(s.lengths, xts)
    nb, total = len(s), int(offsets[-1])
    info, out = np.zeros(nb, dtype=np.int32), np.empty(nb)
    mu, va = np.empty(total) if mean else None, np.empty(total) if var else None
    nchains = C.c_int32(-1)
    _ffi.check(_ffi.lib().tgp_qsep_series_predict(
        s._handle, _ffi.ptr(leaves), leaves.shape[1], _ffi.ptr(smap), h.shape[1], _ffi.ptr(h), _ffi.ptr(P),
        _ffi.ptr(noise), _ffi.ptr(resid), _ffi.ptr(offsets), _ffi.ptr(xtest), _ffi.ptr(at_data), _ffi.ptr(info),
        _ffi.ptr(out), _ffi.ptr(mu), _ffi.ptr(va), C.byref(nchains)), "tgp_qsep_series_predict")
    return out, info, mu, va, nchains.value, offsets


def _dim(name):
    return CASES[name](q)._lower_ssm().J


def _hold_to_oracle(k, t, noise, r, xt, mean, var, tag, dense):
    """The finite test points against the sequential oracle, and at small N against dense LAPACK."""
    x = t if xt is None else np.asarray(xt)
    keep = np.isfinite(x)
    if not keep.any():
        return
    for what, ref in (("oracle", op.predict), ("dense", op.dense))[:2 if dense else 1]:
        wm, wv = ref(k, t, noise, r, x[keep])
        dm, dv = np.abs(mean[keep] - wm).max(), np.abs(var[keep] - wv).max()
        worst["mean"], worst["var"] = max(worst["mean"], dm), max(worst["var"], dv)
        print(f"{tag} {what}: mean {dm:.2e}, variance {dv:.2e}; worst so far {worst['mean']:.2e}, {worst['var']:.2e}")
        np.testing.assert_allclose(mean[keep], wm, **BAR)
        np.testing.assert_allclose(var[keep], wv, **BAR)


# -- 1. every scan edge and every test-point count in one set ------------------------------------------------------------------
EDGE_COUNTS = [7, 300, None, 0, 300, 1, 300]  # for lengths 1, 15, 16, 17, 1024, 1025, 4097; 1024's hold a NaN


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("name", qs.EDGE_CASES)
def test_every_scan_edge_in_one_set(name, reverse):
    """One- and two-level scans, 64 and 65 chunks and last chunks of one step side by side, J = 1, 2, 6 and 8, with 0, 1,
    7 and 300 unsorted test points (before, after and on the data, duplicates, either side of the last chunk boundary,
    one NaN) and one member at its own data.  A length keeps its kernel, noise and test points when the order is
    reversed.  The forward order is also held to the sequential oracle, up to 1025 points to dense LAPACK as well."""
    order = list(range(len(qs.EDGE_LENGTHS)))[::-1 if reverse else 1]
    lengths = [qs.EDGE_LENGTHS[b] for b in order]
    counts = [EDGE_COUNTS[b] for b in order]
    xts = [_points(n, m, n == 1024) for n, m in zip(lengths, counts)]
    got = _evaluate(name, lengths, order, xts)
    for i, (n, b, m) in enumerate(zip(lengths, order, counts)):
        _same(got, i, _single(name, n, b, m, n == 1024), f"{name} n={n} m={m}")
        assert got[1][i].shape == (n if m is None else m,)
    i = lengths.index(1024)
    at = int(np.flatnonzero(np.isnan(xts[i]))[0])
    assert np.isnan(got[1][i][at]) and np.isfinite(np.delete(got[1][i], at)).all()
    if reverse:
        return
    for i, (n, b) in enumerate(zip(lengths, order)):
        t, noise, r = qs.series(n)
        _hold_to_oracle(_member(name, b), t, member_noise(noise, b), r, xts[i], got[1][i], got[2][i],
                        f"{name} n={n}", n <= 1025)


# -- 2. where the test points lie -----------------------------------------------------------------------------------------------
def test_every_placement_of_the_test_points():
    """Six members on the same 1025 points (65 chunks of 16 steps, the last of one step): all test points before the
    first datum, all after the last, all on data points with duplicates, all inside one chunk, either side of the last
    chunk boundary in descending order, and one NaN between finite points."""
    name, n = "m32cos_plus_sho", 1025
    t, noise, r = qs.series(n)
    assert qs.extent(n) == (16, 65, (65, 2))
    rng = np.random.default_rng(5)
    xts = [t[0] - rng.uniform(0.0, 3.0, 7),
           t[-1] + rng.uniform(0.0, 3.0, 7),
           t[rng.integers(0, n, 300)],
           rng.uniform(t[33], t[46], 300),
           np.sort(np.concatenate([rng.uniform(t[1020], t[1024] + 0.5, 20), t[1022:1025]]))[::-1].copy(),
           np.array([t[500] + 0.01, np.nan, t[3] - 0.01])]
    assert len(np.unique(xts[2])) < 300 and set(op.intervals(t, xts[3]) // 16) == {2}
    assert {1023, 1024} <= set(op.intervals(t, xts[4]))
    got = _evaluate(name, [n] * 6, range(6), xts)
    for b, xt in enumerate(xts):
        k, nz = _member(name, b), member_noise(noise, b)
        _same(got, b, _single_call(k, t, nz, r, xt), f"placement {b}")
        _hold_to_oracle(k, t, nz, r, xt, got[1][b], got[2][b], f"placement {b}", True)
    assert np.isnan(got[1][5][1]) and np.isnan(got[2][5][1]) and np.isfinite(got[1][5][[0, 2]]).all()


# -- 3. position and company do not matter -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [2, 5, 65])
def test_position_and_company_do_not_matter(nb):
    """The probe -- 257 points, J = 6, 300 test points -- at every position of sets of 2, 5 and 65 members (65: the probe
    is in the chain of 64 or alone in the second); its neighbours bring 0, 1, 7 or 300 test points or none of their own."""
    name, n, m = qs.PROBE_CASE, qs.PROBE_LENGTH, 300
    want = _single(name, n, 7, m)
    company = [0, 1, None, 7, 300]
    for pos in range(nb):
        lengths = [qs.COMPANY_LENGTHS[b % 4] for b in range(nb)]
        bs = [b % 11 for b in range(nb)]
        counts = [company[(b + pos) % 5] for b in range(nb)]
        lengths[pos], bs[pos], counts[pos] = n, 7, m
        got = _evaluate(name, lengths, bs, [_points(k, c) for k, c in zip(lengths, counts)])
        _same(got, pos, want, f"set of {nb}, position {pos}")


# -- 4. splits ------------------------------------------------------------------------------------------------------------------------
def test_sixty_five_series_run_as_two_chains():
    name, n, nb = "matern32", 40, 65
    bs = [b % 13 for b in range(nb)]
    counts = [[0, 1, 7, 300, None][b % 5] for b in range(nb)]
    ks, ts, nz, rs = _inputs(name, [n] * nb, bs)
    assert qp.series_predict_split([n] * nb, [n if c is None else c for c in counts], 2) == [64, 1]
    s = QuasisepSeriesSet(ts)
    out, info, mu, va, nchains, off = _raw(s, ks, rs, nz, [_points(n, c) for c in counts])
    s.close()
    assert nchains == 2 and not info.any() and np.all(np.isfinite(out))
    got = (out, [mu[lo:hi] for lo, hi in zip(off[:-1], off[1:])], [va[lo:hi] for lo, hi in zip(off[:-1], off[1:])])
    for b in (0, 1, 2, 3, 4, 62, 63, 64):
        _same(got, b, _single(name, n, bs[b], counts[b]))


def test_the_cap_cuts_the_chain():
    """Six series of 2^20 points predicted at their own data, J = 2: 24.7 M doubles each, so five fill a chain and the
    sixth runs alone (the mirror's worked example)."""
    name, n, nb = "matern32", 1 << 20, 6
    assert qp.series_predict_split([n] * nb, [n] * nb, 2) == [5, 1]
    ks, ts, nz, rs = _inputs(name, [n] * nb, range(nb))
    s = QuasisepSeriesSet(ts, assume_sorted=True)
    out, info, mu, va, nchains, off = _raw(s, ks, rs, nz, [None] * nb)
    s.close()
    assert nchains == 2 and not info.any() and np.all(np.isfinite(out)) and list(off) == [n * b for b in range(nb + 1)]
    got = (out, mu.reshape(nb, n), va.reshape(nb, n))
    for b in (4, 5):
        _same(got, b, _single(name, n, b, None))


def test_a_series_beyond_the_cap_is_refused():
    """5 000 000 points at their own data with J = 8 need 28 n = 1.4 * 10^8 doubles and more, the cap is 2^27 = 1.34 * 10^8;
    the check precedes every allocation of the chain's buffer and every launch, and a short neighbour does not help.
    Without its test points the series fits (the mirror's worked example) -- that call is not made here."""
    n = 5_000_000
    assert qp.series_predict_split([40, n], [7, n], 8) is None and qp.series_predict_split([40, n], [7, 0], 8) == [2]
    t = np.zeros(n)
    s = QuasisepSeriesSet([t[:40], t], assume_sorted=True)
    with pytest.raises(ValueError, match=r"series 1 \(n = 5000000\) .*exceeds its cap"):
        s.predict(_member("celerite4", 0), [t[:40], t], [1.0, 1.0], [t[:7], None])
    s.close()


# -- 5. what is asked for ----------------------------------------------------------------------------------------------------------
def test_result_modes_keep_the_bits():
    """Without the variance, without the mean (the C call), with neither: the rest keeps its bits."""
    name, lengths, counts = "m32cos_plus_sho", [1025, 17, 300, 4097], [300, None, 0, 7]
    ks, ts, nz, rs = _inputs(name, lengths, range(4))
    xts = [_points(n, m) for n, m in zip(lengths, counts)]
    s = QuasisepSeriesSet(ts)
    full = s.predict(ks, rs, nz, xts)
    bare = s.predict(ks, rs, nz, xts, return_var=False)
    raw = _raw(s, ks, rs, nz, xts)
    only_var = _raw(s, ks, rs, nz, xts, mean=False)
    only_mean = _raw(s, ks, rs, nz, xts, var=False)
    neither = _raw(s, ks, rs, nz, xts, mean=False, var=False)
    plain = s.log_probability(ks, rs, nz)
    s.close()
    assert bare[2] is None and len(bare) == 3
    for b, (n, m) in enumerate(zip(lengths, counts)):
        _same(full, b, _single(name, n, b, m))
        _same(bare, b, _single(name, n, b, m))
        lo, hi = raw[5][b], raw[5][b + 1]
        assert np.array_equal(raw[2][lo:hi], full[1][b]) and np.array_equal(raw[3][lo:hi], full[2][b])
    for got in (raw, only_var, only_mean, neither):
        assert np.array_equal(got[0], full[0]) and np.array_equal(got[0], plain) and not got[1].any() and got[4] == 1
    assert only_var[2] is None and np.array_equal(only_var[3], raw[3])
    assert only_mean[3] is None and np.array_equal(only_mean[2], raw[2])


def test_one_shared_kernel_equals_equal_copies():
    name, lengths, counts = "m32cos_plus_sho", [17, 1025, 300], [7, 300, None]
    _, ts, nz, rs = _inputs(name, lengths, range(3))
    xts = [_points(n, m) for n, m in zip(lengths, counts)]
    s = QuasisepSeriesSet(ts)
    shared = s.predict(_member(name, 2), rs, nz, xts)
    copies = s.predict([_member(name, 2) for _ in lengths], rs, nz, xts)
    s.close()
    assert np.all(np.isfinite(shared[0])) and np.array_equal(shared[0], copies[0])
    for x, y in zip(shared[1] + shared[2], copies[1] + copies[2]):
        assert np.array_equal(x, y)
    t, _, r = qs.series(1025)
    _same(shared, 1, _single_call(_member(name, 2), t, nz[1], r, xts[1]))


# -- 6. the handle ---------------------------------------------------------------------------------------------------------------
def test_the_handle_serves_call_after_call():
    """Value, prediction, gradient, prediction at other test points, prediction with J = 8, the first prediction again:
    the resident table is cut again before each, and every call has the bits of a fresh set's and of the single calls."""
    lengths = [1025, 17, 300]
    _, ts, nz, rs = _inputs("matern32", lengths, range(3))
    first = [_member("matern32", b) for b in range(3)]        # J = 2
    second = [_member("celerite4", b) for b in range(3)]      # J = 8
    xa = [_points(n, m) for n, m in zip(lengths, [300, 7, None])]
    xb = [_points(n, m) for n, m in zip(lengths, [7, None, 300])]

    def fresh(method, ks, *args, **kw):
        s = QuasisepSeriesSet(ts)
        try:
            return getattr(s, method)(ks, rs, nz, *args, **kw)
        finally:
            s.close()

    s = QuasisepSeriesSet(ts)
    a = s.log_probability(first, rs, nz)
    b = s.predict(first, rs, nz, xa)
    c = s.value_and_grad(first, rs, nz)
    d = s.predict(first, rs, nz, xb)
    e = s.predict(second, rs, nz, xb)
    f = s.predict(first, rs, nz, xa)
    g = s.log_probability(first, rs, nz)
    s.close()
    assert np.array_equal(a, fresh("log_probability", first)) and np.array_equal(g, a) and np.array_equal(c[0], a)
    want_c = fresh("value_and_grad", first)
    assert np.array_equal(c[1]["kernel"], want_c[1]["kernel"])
    assert all(np.array_equal(x, y) for key in ("noise_diag", "mean") for x, y in zip(c[1][key], want_c[1][key]))
    for got, (name, ks, xts, counts) in ((b, ("matern32", first, xa, [300, 7, None])),
                                         (d, ("matern32", first, xb, [7, None, 300])),
                                         (e, ("celerite4", second, xb, [7, None, 300])),
                                         (f, ("matern32", first, xa, [300, 7, None]))):
        want = fresh("predict", ks, xts)
        assert np.array_equal(got[0], want[0])
        assert all(np.array_equal(x, y) for x, y in zip(got[1] + got[2], want[1] + want[2]))
        for i, (n, m) in enumerate(zip(lengths, counts)):
            _same(got, i, _single(name, n, i, m), name)
    assert np.array_equal(a, b[0])
    with pytest.raises(ValueError, match="closed"):
        s.predict(first, rs, nz, xa)


# -- 7. failure stays in its member ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 1, 2])
def test_failure_stays_in_its_member(pos):
    """noise = -10 at local step 5 of one series: h^T P^- h <= k(0) = 1.44 (1 + 0.04 b)^2, so that pivot is negative."""
    name, lengths, counts = "matern32", [300, 1025, 64], {300: 7, 1025: 300, 64: None}
    lengths = lengths[-pos:] + lengths[:-pos]  # the series of 1025 points fails: in the middle, last, first
    bad = lengths.index(1025)
    ks, ts, nz, rs = _inputs(name, lengths, range(3))
    xts = [_points(n, counts[n]) for n in lengths]
    s = QuasisepSeriesSet(ts)
    sound = s.predict(ks, rs, nz, xts)
    nz[bad] = nz[bad].copy()
    nz[bad][5] = -10.0
    values, mus, variances, info = s.predict(ks, rs, nz, xts, return_info=True)
    raw = _raw(s, ks, rs, nz, xts)
    s.close()
    assert list(info) == list(raw[1]) == [6 if b == bad else 0 for b in range(3)]
    assert values[bad] == -np.inf and np.isnan(raw[0][bad])
    assert mus[bad].shape == variances[bad].shape == (300,) and np.all(np.isnan(mus[bad])) and np.all(np.isnan(variances[bad]))
    lo, hi = raw[5][bad], raw[5][bad + 1]
    assert np.all(np.isnan(raw[2][lo:hi])) and np.all(np.isnan(raw[3][lo:hi]))
    want = _single_call(ks[bad], ts[bad], nz[bad], rs[bad], xts[bad])
    assert want[1] == 6 and np.all(np.isnan(want[2])) and np.all(np.isnan(want[3]))
    for b in range(3):
        if b != bad:
            _same((values, mus, variances), b, _single(name, lengths[b], b, counts[lengths[b]]))
            assert np.array_equal(mus[b], sound[1][b]) and np.array_equal(variances[b], sound[2][b])
            assert values[b] == sound[0][b]


# -- 8. the public function -------------------------------------------------------------------------------------------------------
def test_public_function_and_the_means():
    """``predict_series`` against single solvers on ``ys - means``: a scalar mean is added to the prediction, a vector
    mean enters the residual and ``test_means`` is what is added; ``include_mean=False`` adds nothing."""
    name, lengths, counts = "m32cos_plus_sho", [1000, 33, 257, 1], [300, None, 7, 0]
    ks, ts, nz, ys = _inputs(name, lengths, range(4))
    xts = [_points(n, m) for n, m in zip(lengths, counts)]
    scalars = [0.0, 0.3, -0.2, 1.5]
    vectors = [0.1 * np.cos(t) for t in ts]
    at_tests = [0.1 * np.cos(t if x is None else x) for t, x in zip(ts, xts)]
    for means, test_means, added in ((scalars, None, scalars), (vectors, at_tests, at_tests), (None, None, [0.0] * 4)):
        got = tinygp_amd.predict_series(ks, ts, ys, xts, diags=nz, means=means, test_means=test_means)
        off = tinygp_amd.predict_series(ks, ts, ys, xts, diags=nz, means=means, include_mean=False, return_var=False)
        assert len(got) == 3 and off[2] is None
        for b in range(4):
            r = ys[b] if means is None else ys[b] - means[b]
            v, _, mean, var = _single_call(ks[b], ts[b], nz[b], r, xts[b])
            _same(got, b, (v, 0, mean + added[b], var))
            _same(off, b, (v, 0, mean, var))
    with pytest.raises(ValueError, match=r"means\[0\] of series 0 is a vector"):
        tinygp_amd.predict_series(ks, ts, ys, xts, diags=nz, means=vectors)
    with pytest.raises(ValueError, match=r"X_tests must hold one entry per series \(4\); got 3"):
        tinygp_amd.predict_series(ks, ts, ys, xts[:3], diags=nz)


# -- 9. argument errors of the C entry point ---------------------------------------------------------------------------------
def test_predict_refuses_bad_arguments():
    name, lengths = "matern32", [17, 40]
    ks, ts, nz, rs = _inputs(name, lengths, range(2))
    xts = [_points(17, 7), None]
    s = QuasisepSeriesSet(ts)
    leaves, smap, h, P, noise, resid = pack_series(s.lengths, ks, rs, nz)
    offsets, xtest, at_data = pack_series_tests(s.lengths, xts)
    info, out, mu, va = np.zeros(2, dtype=np.int32), np.empty(2), np.empty(47), np.empty(47)
    full = [leaves, smap, h, P, noise, resid, offsets, xtest, at_data, info, out, mu, va]

    def call(a):
        _ffi.check(_ffi.lib().tgp_qsep_series_predict(
            s._handle, _ffi.ptr(a[0]), leaves.shape[1], _ffi.ptr(a[1]), h.shape[1], *(_ffi.ptr(x) for x in a[2:]), None))

    for missing in (0, 1, 2, 3, 4, 5, 6, 7, 9, 10):
        with pytest.raises(ValueError, match="null"):
            call([None if i == missing else x for i, x in enumerate(full)])
    with pytest.raises(ValueError, match=r"the test offsets start at 0 \(got 1\)"):
        call(full[:6] + [offsets + 1] + full[7:])
    with pytest.raises(ValueError, match=r"the test offsets must not decrease \(series 1: 3 after 7\)"):
        call(full[:6] + [np.array([0, 7, 3])] + full[7:])
    with pytest.raises(ValueError, match=r"series 0 predicts at its own 17 data points.*\(got 7\)"):
        call(full[:8] + [np.array([1, 1], dtype=np.int32)] + full[9:])
    with pytest.raises(ValueError, match=r"series 1 predicts at its own 40 data points.*\(got 39\)"):
        call(full[:6] + [np.array([0, 7, 46])] + full[7:])
    # the flags, the means, the variances and, where every member is at its own data, the test points may be missing
    call(full[:8] + [None] + full[9:])
    call(full[:11] + [None, None])
    call(full[:6] + [np.array([0, 17, 57]), None, np.array([1, 1], dtype=np.int32)] + full[9:11] + [np.empty(57), None])
    call(full)  # the refusals left the set usable
    got = s.predict(ks, rs, nz, xts)
    s.close()
    assert np.array_equal(out, got[0]) and np.array_equal(mu, np.concatenate(got[1]))
    assert np.array_equal(va, np.concatenate(got[2]))
    for b, (n, m) in enumerate(zip(lengths, [7, None])):
        _same(got, b, _single(name, n, b, m))
