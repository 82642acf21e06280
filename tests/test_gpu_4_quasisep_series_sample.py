"""Posterior draws for sets of series (``QuasisepSeriesSet.sample_conditional`` / ``tgp_qsep_series_sample`` /
``tinygp_amd.sample_conditional_series``): every member to the bit against the device's single calls on a fresh
``QuasisepSolver`` -- ``log_probability`` and ``sample_conditional`` with that member's test points and normals --
whatever the set's size, the member's position, its company, the number of columns and the split into launch chains and
column passes; against the sequential statement ``_quasisep_sample_np.sample`` at the project's posterior bar, rtol =
atol = 5e-7 (README "Parity"), and, fed every unit vector, against the dense conditional mean and covariance at 1e-9
(the bar of ``test_gpu_4_quasisep_sample.py``).  Coordinates keep distinct neighbours 0.02 apart
(``_quasisep_sample_np.lattice`` says why).  Every test prints the figures it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest

import tinygp_amd
from tinygp_amd import GaussianProcess, _ffi
from tinygp_amd.kernels import quasisep as q
from tinygp_amd.noise import Diagonal
from tinygp_amd.solvers import QuasisepSeriesSet, QuasisepSolver
from tinygp_amd.solvers.quasisep import pack_series, pack_series_normals, pack_series_sample_tests

import _quasisep_sample_np as so
import _quasisep_series_sample as ss
from _quasisep_cases import CASES
from _quasisep_grad_batch import member, member_noise

pytestmark = pytest.mark.gpu

BAR = dict(rtol=5e-7, atol=5e-7)


def _kernel(name, b):
    return member(CASES, q, name, b)


def _dim(name):
    return CASES[name](q)._lower_ssm().J


def _normals(n, m, J, R):
    """Columns 0 .. R - 1 of the member's 65: column c is the same whatever R (the deep member is drawn at its own R)."""
    if n > 5000:
        return ss.normals(n, m, J, R)
    xi, eps = ss.normals(n, m, J, 65)
    return xi[:, :, :R], eps[:, :R]


@functools.lru_cache(maxsize=None)
def _single(name, n, m, b, R):
    """Member (n, m) under kernel and noise number b, alone on a fresh solver: ``(value, info, data, test)``; m None:
    the test side is the data side.  Computed once, read-only."""
    t, noise, r, xt = ss.problem(n, m)
    xi, eps = _normals(n, m, _dim(name), R)
    s = QuasisepSolver(_kernel(name, b), t, Diagonal(member_noise(noise, b)), assume_sorted=True)
    try:
        v = float(s.log_probability(r))
        if m is None:
            data = test = np.asarray(s.sample_conditional(r, None, xi=xi, eps=eps))
        else:
            data, test = (np.asarray(a) for a in s.sample_conditional(r, xt, xi=xi, eps=eps, return_data=True))
        info = int(s.info)
    finally:
        s.close()
    data.setflags(write=False), test.setflags(write=False)
    return v, info, data, test


def _inputs(name, members, bs, R):
    probs = [ss.problem(n, m) for n, m in members]
    J = _dim(name)
    nm = [_normals(n, m, J, R) for n, m in members]
    return dict(kernels=[_kernel(name, b) for b in bs], ts=[p[0] for p in probs],
                diags=[member_noise(p[1], b) for p, b in zip(probs, bs)], ys=[p[2] for p in probs],
                xts=[None if m is None else p[3] for p, (n, m) in zip(probs, members)],
                xi=[a[0] for a in nm], eps=[a[1] for a in nm])


def _draw(name, members, bs, R, return_data=True, diags=None):
    """The set's call: ``(values, tests, datas or None, info, chains, passes)``."""
    a = _inputs(name, members, bs, R)
    s = QuasisepSeriesSet(a["ts"], assume_sorted=True)
    try:
        out = s.sample_conditional(a["kernels"], a["ys"], a["diags"] if diags is None else diags, a["xts"], xi=a["xi"],
                                   eps=a["eps"], return_data=return_data, return_info=True)
        chains, passes = s.sample_chains, s.sample_passes
    finally:
        s.close()
    values, tests = out[0], out[1]
    assert values.shape == (len(members),) and values.dtype == np.float64 and len(tests) == len(members)
    return values, tests, out[2] if return_data else None, out[-1], chains, passes


def _same(got, i, want, tag):
    """Member i of a set's result has the bits of the single calls'."""
    v, info, data, test = want
    assert got[3][i] == info and got[0][i] == v, (tag, i, got[0][i], v)
    assert got[1][i].dtype == np.float64 and got[1][i].shape == test.shape, (tag, i, got[1][i].shape, test.shape)
    assert np.array_equal(got[1][i], test), (tag, i, "test side", np.abs(got[1][i] - test).max())
    if got[2] is not None:
        assert got[2][i].shape == data.shape and np.array_equal(got[2][i], data), (tag, i, "data side")


# -- 1. bits against fresh solvers, both extents on their edges ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_set(name):
    return _draw(name, ss.EDGE_SET, range(len(ss.EDGE_SET)), ss.EDGE_COLS)


@pytest.mark.parametrize("name", ss.EDGE_CASES)
def test_every_member_has_the_bits_of_a_fresh_solver(name):
    """One set of eleven members, J = 2, 6 and 8, R = 9 (a second column group with one live column): data extents of 1,
    15, 16, 17, 1000 (63 chunks), 1024 (64) and 1025 (65, the last of one step) points beside merged grids of 2, 16, 17,
    26, 1024 (64 chunks), 1025 (65) and 1325 points; members at their own points, with one test point and with an empty
    array of them.  Value, data side and test side equal the single calls' bit for bit."""
    got = _edge_set(name)
    assert not got[3].any() and np.isfinite(got[0]).all() and got[4] == 1 and got[5] == 1
    for i, (n, m) in enumerate(ss.EDGE_SET):
        _same(got, i, _single(name, n, m, i, ss.EDGE_COLS), f"{name} n={n} m={m}")
        assert got[1][i].shape == (n if m is None else m, ss.EDGE_COLS) and got[2][i].shape == (n, ss.EDGE_COLS)
        assert np.isfinite(got[1][i]).all() and np.isfinite(got[2][i]).all()
    print(f"series sample {name}: {len(ss.EDGE_SET)} members, R = {ss.EDGE_COLS}, all equal to fresh solvers")


# -- 2. the oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ss.EDGE_CASES)
def test_a_member_of_that_set_matches_the_oracle(name):
    """One member per kernel -- (17, 9) at J = 2, (1000, 24) at J = 6, (1000, 25) at J = 8 -- against the sequential
    statement with a dense closure, so that the set is not held to its sibling alone."""
    i = ss.ORACLE_MEMBERS[name]
    n, m = ss.EDGE_SET[i]
    t, noise, r, xt = ss.problem(n, m)
    xi, eps = _normals(n, m, _dim(name), ss.EDGE_COLS)
    wd, wt = so.sample(_kernel(name, i), t, member_noise(noise, i), r, xt, xi, eps)
    got = _edge_set(name)
    ed, et = np.abs(got[2][i] - wd).max(), np.abs(got[1][i] - wt).max()
    print(f"series sample {name} n={n} m={m} against the oracle: data {ed:.2e}, test {et:.2e}")
    np.testing.assert_allclose(got[2][i], wd, **BAR)
    np.testing.assert_allclose(got[1][i], wt, **BAR)


# -- 3. the exact distribution -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ss.EDGE_CASES)
def test_exact_distribution_of_three_members_in_one_set(name):
    """Members (1, 1), (5, 3) and (17, 9) in one set, fed every unit vector of their normals as a column (the shorter
    members' further columns are zero): S S^T and the value at zero normals against the dense joint conditional
    covariance and mean of data and test points, every entry within 1e-9."""
    J = _dim(name)
    probs = [ss.problem(n, m) for n, m in ss.SMALL_SET]
    units = [so.unit_normals(n, m, J) for n, m in ss.SMALL_SET]
    R = max(u[0].shape[2] for u in units)
    xi = [np.concatenate([u[0], np.zeros(u[0].shape[:2] + (R - u[0].shape[2],))], axis=2) for u in units]
    eps = [np.concatenate([u[1], np.zeros((u[1].shape[0], R - u[1].shape[1]))], axis=1) for u in units]
    ks = [_kernel(name, b) for b in range(3)]
    ts, nz, xts = [p[0] for p in probs], [member_noise(p[1], b) for b, p in enumerate(probs)], [p[3] for p in probs]
    s = QuasisepSeriesSet(ts, assume_sorted=True)
    try:
        _, St, Sd, info = s.sample_conditional(ks, [np.zeros(len(t)) for t in ts], nz, xts, xi=xi, eps=eps,
                                               return_data=True, return_info=True)
        assert not info.any() and s.sample_chains == 1 and s.sample_passes == -(-R // 64)
        _, mt, md = s.sample_conditional(ks, [p[2] for p in probs], nz, xts, xi=[np.zeros(a.shape[:2]) for a in xi],
                                         eps=[np.zeros(len(t)) for t in ts], return_data=True)
    finally:
        s.close()
    for b, (n, m) in enumerate(ss.SMALL_SET):
        S, mean = np.vstack([Sd[b], St[b]]), np.concatenate([md[b], mt[b]])
        assert S.shape == (n + m, R) and not S[:, units[b][0].shape[2]:].any()
        wmean, wcov = so.dense(ks[b], ts[b], nz[b], probs[b][2], np.concatenate([ts[b], xts[b]]))
        ecov, emean = np.abs(S @ S.T - wcov).max(), np.abs(mean - wmean).max()
        print(f"series sample distribution {name} n={n} m={m} R={R}: max |S S^T - cov| = {ecov:.2e}, "
              f"max |mean - dense| = {emean:.2e}")
        assert ecov <= 1e-9 and emean <= 1e-9


# -- 4. invariance, bit for bit ----------------------------------------------------------------------------------------------------
INV_CASE = "m32cos_plus_sho"
INV_SET = [(17, 9), (40, 5), (300, 0), (1000, 25), (16, None)]
INV_BS = [3, 1, 4, 0, 5]


@functools.lru_cache(maxsize=None)
def _inv_base(R=9):
    return _draw(INV_CASE, INV_SET, INV_BS, R)


def test_the_set_reversed_and_every_member_alone():
    base = _inv_base()
    assert not base[3].any()
    for i, (n, m) in enumerate(INV_SET):
        _same(base, i, _single(INV_CASE, n, m, INV_BS[i], 9), f"base n={n}")
    rev = _draw(INV_CASE, INV_SET[::-1], INV_BS[::-1], 9)
    for i in range(len(INV_SET)):
        j = len(INV_SET) - 1 - i
        assert rev[0][j] == base[0][i] and np.array_equal(rev[1][j], base[1][i]) and np.array_equal(rev[2][j], base[2][i])
    for i, member_ in enumerate(INV_SET):
        alone = _draw(INV_CASE, [member_], [INV_BS[i]], 9)
        assert alone[4] == 1 and alone[0][0] == base[0][i]
        assert np.array_equal(alone[1][0], base[1][i]) and np.array_equal(alone[2][0], base[2][i])


def test_sixty_five_copies_run_as_two_chains():
    """B = 65 copies of the 40-point member: the member limit cuts after 64, the last copy runs in a chain of its own."""
    got = _draw(INV_CASE, [(40, 5)] * 65, [1] * 65, 9)
    assert ss.series_sample_split([40] * 65, [5] * 65, _dim(INV_CASE), 9) == [ss.Chain(64, 9, 1), ss.Chain(1, 9, 1)]
    assert got[4] == 2 and got[5] == 2 and not got[3].any()
    want = _single(INV_CASE, 40, 5, 1, 9)
    for i in (0, 1, 31, 63, 64):
        _same(got, i, want, f"copy {i}")
    assert all(np.array_equal(got[1][i], want[3]) and np.array_equal(got[2][i], want[2]) for i in range(65))


@pytest.mark.parametrize("R", [1, 8, 9, 65])
def test_a_column_does_not_depend_on_the_number_of_columns(R):
    """R = 1, 8, 9 and 65 (two passes: 64 + 1): chains and passes as the host rule says, column c as in the R = 65 call
    and as a fresh solver draws it."""
    got = _draw(INV_CASE, INV_SET, INV_BS, R)
    counts = [0 if m is None else m for _, m in INV_SET]
    rule = ss.series_sample_split([n for n, _ in INV_SET], counts, _dim(INV_CASE), R)
    assert (got[4], got[5]) == (len(rule), sum(c.passes for c in rule)) == (1, 2 if R == 65 else 1)
    wide = _inv_base(65)
    for i, (n, m) in enumerate(INV_SET):
        assert got[0][i] == wide[0][i]
        assert np.array_equal(got[1][i], wide[1][i][:, :R]) and np.array_equal(got[2][i], wide[2][i][:, :R])
        _same(got, i, _single(INV_CASE, n, m, INV_BS[i], R), f"R={R} n={n}")


def test_the_test_side_alone():
    """Without the data side (no member at its own points): the same test-side bits, and nothing else asked of the device."""
    members, bs = INV_SET[:4], INV_BS[:4]
    got = _draw(INV_CASE, members, bs, 9, return_data=False)
    base = _inv_base()
    assert got[2] is None
    for i in range(4):
        assert got[0][i] == base[0][i] and np.array_equal(got[1][i], base[1][i])


# -- 5. depth ---------------------------------------------------------------------------------------------------------------------
def test_a_deep_grid_beside_a_short_member():
    """(65 537, 40) beside (40, 5), R = 1: chunks of 32 and a scan of 2049 (data) and 2050 (grid) chunks through groups of
    64 beside a member whose scans have one level."""
    name = "celerite4"
    got = _draw(name, ss.DEEP_SET, [0, 1], 1)
    assert got[4] == 1 and got[5] == 1
    for i, (n, m) in enumerate(ss.DEEP_SET):
        _same(got, i, _single(name, n, m, i, 1), f"deep n={n}")
        assert np.isfinite(got[1][i]).all() and np.isfinite(got[2][i]).all()


# -- 6. failure ---------------------------------------------------------------------------------------------------------------------
def test_a_failed_member_touches_no_other():
    """A negative noise entry at step 17 of the middle member: its info is 17, its value -inf, its draws NaN; the others
    keep the bits they have in the set where it is healthy."""
    members, bs = [(17, 9), (40, 5), (1000, 24)], [0, 1, 2]
    good = _draw("matern32", members, bs, 9)
    diags = list(_inputs("matern32", members, bs, 9)["diags"])
    diags[1] = np.array(diags[1])
    diags[1][16] = -10.0
    bad = _draw("matern32", members, bs, 9, diags=diags)
    assert list(bad[3]) == [0, 17, 0] and bad[0][1] == -np.inf
    assert bad[1][1].shape == (5, 9) and np.isnan(bad[1][1]).all() and np.isnan(bad[2][1]).all()
    for i in (0, 2):
        assert bad[0][i] == good[0][i] and np.array_equal(bad[1][i], good[1][i]) and np.array_equal(bad[2][i], good[2][i])


def _raw(s, a, xts, R, **change):
    """The low-level call with the arrays of ``_inputs``; ``change``: arguments replaced (None: a null pointer)."""
    leaves, smap, h, P, noise, resid = pack_series(s.lengths, a["kernels"], a["ys"], a["diags"])
    offsets, xtest, at_data = pack_series_sample_tests(s.lengths, [None if x is None else np.zeros(len(x)) for x in xts])
    xtest = np.concatenate([np.asarray(x, dtype=np.float64) for x in xts if x is not None] + [np.empty(0)])
    xi, eps, _, _ = pack_series_normals(s.lengths, np.diff(offsets), h.shape[1], a["xi"], a["eps"])
    nb = len(s)
    args = dict(offsets=offsets, xtest=xtest, at_data=at_data, R=R, xi=xi, eps=eps, info=np.zeros(nb, dtype=np.int32),
                out=np.empty(nb), data=np.empty((int(s.lengths.sum()), R)), test=np.empty((max(len(xtest), 1), R)))
    args.update(change)
    p = lambda k: _ffi.ptr(args[k])  # noqa: E731
    chains, passes = C.c_int32(-1), C.c_int32(-1)
    _ffi.check(_ffi.lib().tgp_qsep_series_sample(
        s._handle, _ffi.ptr(leaves), leaves.shape[1], _ffi.ptr(smap), h.shape[1], _ffi.ptr(h), _ffi.ptr(P),
        _ffi.ptr(noise), _ffi.ptr(resid), p("offsets"), p("xtest"), p("at_data"), args["R"], p("xi"), p("eps"), p("info"),
        p("out"), p("data"), p("test"), C.byref(chains), C.byref(passes)), "tgp_qsep_series_sample")
    return args, chains.value, passes.value


def test_argument_errors_name_the_series():
    members, bs = [(17, 9), (40, 5), (16, None)], [0, 1, 2]
    a = _inputs("matern32", members, bs, 3)
    s = QuasisepSeriesSet(a["ts"], assume_sorted=True)
    try:
        for bad in (np.nan, np.inf):
            xts = [a["xts"][0], np.array(a["xts"][1]), None]
            xts[1][3] = bad
            with pytest.raises(ValueError, match=r"X_tests\[1\] of series 1 must be finite"):
                s.sample_conditional(a["kernels"], a["ys"], a["diags"], xts, xi=a["xi"], eps=a["eps"])
            with pytest.raises(ValueError, match=r"test point 3 of series 1 is not finite"):
                _raw(s, a, xts, 3)
        with pytest.raises(ValueError, match=r"need at least one column of draws \(got 0\)"):
            _raw(s, a, a["xts"], 0)
        with pytest.raises(ValueError, match=r"the test offsets start at 0 \(got 1\)"):
            _raw(s, a, a["xts"], 3, offsets=np.array([1, 9, 14, 14], dtype=np.int64))
        with pytest.raises(ValueError, match=r"the test offsets must not decrease \(series 1: 5 after 9\)"):
            _raw(s, a, a["xts"], 3, offsets=np.array([0, 9, 5, 14], dtype=np.int64))
        with pytest.raises(ValueError, match=r"series 1 draws at its own data.*must be 0 \(got 5\)"):
            _raw(s, a, a["xts"], 3, at_data=np.array([0, 1, 1], dtype=np.int32))
        for name in ("offsets", "xtest", "xi", "eps", "info", "out"):
            with pytest.raises(ValueError, match="null"):
                _raw(s, a, a["xts"], 3, **{name: None})
        # the set still serves: the flags may be null, and either output
        args, chains, passes = _raw(s, a, a["xts"], 3, at_data=None, data=None)
        want = s.sample_conditional(a["kernels"], a["ys"], a["diags"], a["xts"], xi=a["xi"], eps=a["eps"])
        assert (chains, passes) == (1, 1) and np.array_equal(args["out"], want[0])
        assert np.array_equal(args["test"][:9], want[1][0]) and np.array_equal(args["test"][9:14], want[1][1])
        args, chains, passes = _raw(s, a, a["xts"], 3, test=None, data=None)
        assert (chains, passes) == (1, 0) and np.array_equal(args["out"], want[0])
    finally:
        s.close()


# -- 7. the front end -------------------------------------------------------------------------------------------------------------
def test_sample_conditional_series_draws_as_gaussian_process_does():
    name = "m32cos_plus_sho"
    members = [(40, 5), (17, 9), (16, None)]
    probs = [ss.problem(n, m) for n, m in members]
    ks = [_kernel(name, b) for b in range(3)]
    Xs, nz, ys = [p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs]
    xts = [probs[0][3], probs[1][3], None]
    vec = np.linspace(-1.0, 1.0, 17)
    # member 0 against GaussianProcess with the same seed, to the bit: 1-D, shaped, with a scalar mean
    for shape in (None, (2, 3)):
        values, samples = tinygp_amd.sample_conditional_series(ks, Xs, ys, xts, diags=nz, key=3, shape=shape,
                                                               means=[0.75, 0.0, 0.0])
        gp = GaussianProcess(ks[0], Xs[0], diag=nz[0], mean=0.75)
        want = gp.sample_conditional(ys[0], xts[0], key=3, shape=shape)
        tail = () if shape is None else shape
        assert [s.shape for s in samples] == [tail + (5,), tail + (9,), tail + (16,)]
        assert samples[0].dtype == np.float64 and np.array_equal(samples[0], want)
        assert values[0] == float(gp.log_probability(ys[0]))
        # ... and the later members continue the same generator
        rng = np.random.default_rng(3)
        R = int(np.prod(tail, dtype=np.int64))
        given = []
        for (n, m) in members:
            xi = rng.standard_normal((n + (0 if m is None else m), 6, R))
            given.append((xi, rng.standard_normal((n, R))))
        v2, again = tinygp_amd.sample_conditional_series(ks, Xs, ys, xts, diags=nz, key=None, shape=shape,
                                                         means=[0.75, 0.0, 0.0], normals=given)
        assert np.array_equal(v2, values) and all(np.array_equal(x, y) for x, y in zip(samples, again))
        gp2 = GaussianProcess(ks[2], Xs[2], diag=nz[2])
        s2 = gp2.solver.sample_conditional(ys[2], None, xi=given[2][0], eps=given[2][1])
        assert np.array_equal(samples[2], np.moveaxis(s2, 0, -1).reshape(tail + (16,)))
    # a vector mean enters the residual; what include_mean adds at the test points is test_means
    values, with_mean = tinygp_amd.sample_conditional_series(ks, Xs, ys, xts, diags=nz, key=3,
                                                             means=[0.0, vec, 0.5], test_means=[None, 2.0, None])
    _, without = tinygp_amd.sample_conditional_series(ks, Xs, ys, xts, diags=nz, key=3, means=[0.0, vec, 0.5],
                                                      include_mean=False)
    assert np.array_equal(with_mean[1], without[1] + 2.0) and np.array_equal(with_mean[2], without[2] + 0.5)
    assert np.array_equal(with_mean[0], without[0])
    _, plain = tinygp_amd.sample_conditional_series(ks, Xs, [ys[0], ys[1] - vec, ys[2] - 0.5], xts, diags=nz, key=3)
    assert np.array_equal(plain[1], without[1]) and np.array_equal(plain[2], without[2])
