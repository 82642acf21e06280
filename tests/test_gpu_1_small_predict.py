"""Predictions of batches of small dense GPs in one launch, one workgroup per member and per chunk of test points
(``csrc/small.hip``, ``tgp_small_predict``) through ``tinygp_amd.predict_datasets``, ``DirectSolver.predict_batch`` and
``GaussianProcess.predict_batch``.

Inputs and references: ``_dense_small_predict.py`` (float64 LAPACK, its own conditions asserted) and, for every leaf and
operator, the single path ``GaussianProcess.predict``.  Bars: the project's fp64 solve bar against the reference (rtol
1e-10 plus atol 1e-10 max|want| per member, for mean and variance), 1e-8 for the value, the posterior bar (rtol = atol =
5e-7) against the single path; value bits, chunking, independence and the routes to the single path are held with
tolerance zero."""
import numpy as np
import pytest

import tinygp_amd
from tinygp_amd import GaussianProcess, kernels, transforms
from tinygp_amd.kernels import quasisep
from tinygp_amd.noise import Dense, Diagonal
from tinygp_amd.solvers import DirectSolver, small

import _dense_np as dn
import _dense_small as ds
import _dense_small_predict as sp

pytestmark = pytest.mark.gpu

CAP = ds.CAP
CHUNK = small.PRED_CHUNK
JITTER = np.sqrt(np.finfo(np.float64).eps)  # what condition() adds to the variances by default
POST = dn.posterior_bar(np.float64)


def _same(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert np.array_equal(a, b, equal_nan=True), (what, a, b)


def _sets(n, d, members, Xt, **kwargs):
    """``predict_datasets`` of members b of the (n, d) inputs, every one at the test points ``Xt``."""
    B = len(members)
    X = dn.train(n, d)[0]
    return tinygp_amd.predict_datasets([ds.member_kernel(kernels, d, b) for b in members], [X] * B, [ds.resid(n)] * B,
                                       [Xt] * B, diags=[ds.member_noise(n, d, b) for b in members], **kwargs)


def _batch(n, d, members, Xt, **kwargs):
    """``DirectSolver.predict_batch`` of the same members (no jitter in its variances)."""
    X, diag = dn.train(n, d)
    solver = DirectSolver(ds.member_kernel(kernels, d, 0), X, Diagonal(diag))
    try:
        return solver.predict_batch([ds.member_kernel(kernels, d, b) for b in members], ds.resid(n), Xt,
                                    np.stack([ds.member_noise(n, d, b) for b in members]), **kwargs)
    finally:
        solver.close()


def _single(model, X, diag, y, Xt, **kwargs):
    gp = GaussianProcess(model, X, diag=diag)
    try:
        return gp.predict(y, Xt, return_var=True, **kwargs)
    finally:
        gp.solver.close()


# ---- 1. parity with the LAPACK reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
@pytest.mark.parametrize("n", ds.EDGE_NS)
def test_parity_with_the_lapack_reference_at_the_edges(n, d):
    worst = dict(value=0.0, mean=0.0, var=0.0)
    for B in (1, 3):
        for mr in sp.RANDOM_COUNTS:
            Xt = sp.query(n, d, mr)
            values, mu, var, info = _batch(n, d, range(B), Xt, return_info=True)
            assert values.shape == (B,) and mu.shape == var.shape == (B, mr + 2) and not info.any()
            assert mu.dtype == var.dtype == np.float64
            sets = _sets(n, d, range(B), Xt)
            bare = _sets(n, d, range(B), Xt, return_var=False)
            assert bare[2] is None and np.array_equal(bare[0], values)
            for b in range(B):
                ref = sp.reference(n, d, b, mr)
                worst["value"] = max(worst["value"], abs(values[b] - ref.value) / (ds.BAR * max(1.0, abs(ref.value))))
                worst["mean"] = max(worst["mean"], sp.bars(mu[b], ref.mean))
                worst["var"] = max(worst["var"], sp.bars(var[b], ref.var))
            print(f"n={n} d={d}: worst fraction of the bars " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
            for b in range(B):
                ref = sp.reference(n, d, b, mr)
                what = f"n={n} d={d} B={B} m={mr + 2} member {b}"
                assert ds.within_bar(values[b], ref.value), what
                sp.check(mu[b], ref.mean, what)
                sp.check(var[b], ref.var, what)
                # the two entry points: the same bits, the jitter of condition() on the data sets' variances
                assert sets[0][b] == values[b], what
                _same(sets[1][b], mu[b], what)
                _same(sets[2][b], var[b] + JITTER, what)
                _same(bare[1][b], mu[b], what + " (mean only)")


# ---- 2. test-point edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
@pytest.mark.parametrize("n", (65, CAP))
def test_every_group_and_chunk_edge_of_the_test_points(n, d):
    # 4 T - 1, 4 T, 4 T + 1 for T = 1, 2 and 4: the last group of the four waves, whatever T the kernel is built with
    ms = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
    X, y, noise = dn.train(n, d)[0], ds.resid(n), ds.member_noise(n, d, 1)
    k = ds.member_kernel(kernels, d, 1)
    P = np.asarray(sp.many_points(max(ms), d))
    plain = tinygp_amd.log_probability_datasets([k], [X], [y], diags=[noise])
    # every point sent alone: one member per point
    M = len(P)
    alone = tinygp_amd.predict_datasets(k, [X] * M, [y] * M, [P[t:t + 1] for t in range(M)], diags=[noise] * M)
    alone_mu, alone_var = np.concatenate(alone[1]), np.concatenate(alone[2])
    assert np.all(alone[0] == plain[0]) and np.all(np.isfinite(alone_mu)) and np.all(alone_var > 0.0)
    # the longest list against the single path: the chunks are stitched in the caller's order
    want_mu, want_var = _single(k, X, noise, y, P)
    np.testing.assert_allclose(alone_mu, want_mu, **POST)
    np.testing.assert_allclose(alone_var, want_var, **POST)
    for m in ms:
        values, mu, var = tinygp_amd.predict_datasets([k], [X], [y], [P[:m]], diags=[noise])
        assert values[0] == plain[0], m  # the first chunk's value has the bits of tgp_small_logprob
        assert mu[0].shape == var[0].shape == (m,)
        _same(mu[0], alone_mu[:m], f"n={n} d={d} m={m}: means")
        _same(var[0], alone_var[:m], f"n={n} d={d} m={m}: variances")
        bare = tinygp_amd.predict_datasets([k], [X], [y], [P[:m]], diags=[noise], return_var=False)
        _same(bare[1][0], alone_mu[:m], f"n={n} d={d} m={m}: mean only")


# ---- 3. independence, tolerance zero on every output ------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
def test_a_members_bits_do_not_depend_on_the_batch(d):
    n, me, mr = 17, 2, 5
    Xt = sp.query(n, d, mr)

    def member(result, m):
        return result[0][m], np.asarray(result[1][m]), np.asarray(result[2][m])

    def same(a, b, what):
        assert a[0] == b[0], what
        _same(a[1], b[1], what)
        _same(a[2], b[2], what)

    alone = member(_sets(n, d, [me], Xt), 0)
    ref = sp.reference(n, d, me, mr)
    sp.check(alone[1], ref.mean)
    sp.check(alone[2], ref.var + JITTER)
    same(alone, member(_sets(n, d, [me], Xt), 0), "across two calls")
    for members in ([me, 0, 1], [0, me, 1], [0, 1, me]):  # first, middle and last of B = 3
        same(alone, member(_sets(n, d, members, Xt), members.index(me)), members)
    # inside B = 300 of mixed structures, lengths and numbers of test points
    B, at = 300, 137
    X, y = dn.train(n, d)[0], ds.resid(n)
    ks, Xs, ys, Xts, nz = [], [], [], [], []
    for m in range(B):
        nn = (n, 8, 33)[m % 3]
        ks.append(ds.member_kernel(kernels, d, m % 7, other=m % 2 == 1))
        Xs.append(dn.train(nn, d)[0])
        ys.append(ds.resid(nn))
        Xts.append(sp.query(nn, d, sp.RANDOM_COUNTS[m % 2]))
        nz.append(ds.member_noise(nn, d, m % 7))
    ks[at], Xs[at], ys[at], Xts[at], nz[at] = ds.member_kernel(kernels, d, me), X, y, Xt, ds.member_noise(n, d, me)
    mixed = tinygp_amd.predict_datasets(ks, Xs, ys, Xts, diags=nz)
    same(alone, member(mixed, at), "inside B = 300")
    assert np.all(np.isfinite(mixed[0])) and all(np.all(np.isfinite(v)) for v in mixed[2])
    # beside a neighbour at the cap (the launch's LDS is sized by the larger member) with several chunks of its own
    big_X, big_t = dn.train(CAP, d)[0], np.asarray(sp.many_points(CHUNK + 3, d))
    got = tinygp_amd.predict_datasets(
        [ds.member_kernel(kernels, d, 0), ds.member_kernel(kernels, d, me), ds.member_kernel(kernels, d, 1)],
        [big_X, X, big_X], [ds.resid(CAP), y, ds.resid(CAP)], [big_t, Xt, sp.query(CAP, d, 5)],
        diags=[ds.member_noise(CAP, d, 0), ds.member_noise(n, d, me), ds.member_noise(CAP, d, 1)])
    same(alone, member(got, 1), "beside a neighbour at the cap")
    big = sp.reference(CAP, d, 1, 5)
    sp.check(got[1][2], big.mean)
    sp.check(got[2][2], big.var + JITTER)
    # through the shared-points entry
    values, mu, var = _batch(n, d, [0, me], Xt)
    same(alone, (values[1], mu[1], var[1] + JITTER), "through DirectSolver.predict_batch")
    # the same test point at another position of the member's list
    order = np.array([6, 0, 3, 3, 5, 1, 2, 4, 6])
    moved = member(_sets(n, d, [me], np.asarray(Xt)[order]), 0)
    assert moved[0] == alone[0]
    _same(moved[1], alone[1][order], "means at other positions")
    _same(moved[2], alone[2][order], "variances at other positions")


# ---- 4. every leaf and operator against the single path ---------------------------------------------------------------------
@pytest.mark.parametrize("D", ds.LEAF_DS)
def test_every_leaf_and_operator_against_the_single_path(D):
    members = ds.leaf_members(kernels, transforms)
    X, n, y = ds.leaf_points(D), ds.LEAF_N, ds.resid(ds.LEAF_N)
    Q = np.random.default_rng([13, D]).uniform(0.0, 3.0 / D, (6, D))
    Xt = np.concatenate([Q[:, 0] if D == 1 else Q, np.stack([X[0], X[-1]]) + 0.01])
    noise = np.stack([ds.leaf_noise() * (1.0 + 0.1 * b) for b in range(len(members))])
    ks = [k for _, k, _ in members]
    assert len(ks) == 17
    gp = GaussianProcess(ks[1], X, diag=ds.leaf_noise())
    try:
        lowered = [small.lower_member(k, X) for k in ks]
        assert small.batch_route(n, True, lowered)  # one launch
        assert all(small.lower_test(k, None, X, Xt, low) is not None for k, low in zip(ks, lowered))
        mu, var = gp.predict_batch(y, ks, Xt, diags=noise)
        values = gp.solver.log_probability_batch(ks, y, noise)
        raw = gp.solver.predict_batch(ks, y, Xt, noise)
    finally:
        gp.solver.close()
    assert mu.shape == var.shape == (17, 8) and np.array_equal(raw[0], values)
    worst = dict(mean=0.0, var=0.0)
    for m, (name, k, _) in enumerate(members):
        want_mu, want_var = _single(k, X, noise[m], y, Xt)
        for key, got, want in (("mean", mu[m], want_mu), ("var", var[m], want_var)):
            worst[key] = max(worst[key], float(np.max(np.abs(got - want) / (POST["atol"] + POST["rtol"] * np.abs(want)))))
            np.testing.assert_allclose(got, want, err_msg=f"D={D} {name} {key}", **POST)
    print(f"D={D}: worst fraction of the posterior bar " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- 5. a prediction program --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
def test_each_addend_of_a_sum_as_the_prediction_kernel(d):
    n, mr = 65, 5
    X, y, noise, Xt = dn.train(n, d)[0], ds.resid(n), ds.member_noise(n, d, 0), sp.query(n, d, mr)
    k1, k2 = ds.member_kernel(kernels, d, 0), ds.member_kernel(kernels, d, 0, other=True)
    k = k1 + k2
    values, mu, var = tinygp_amd.predict_datasets(k, [X] * 3, [y] * 3, [Xt] * 3, diags=[noise] * 3,
                                                  predict_kernels=[None, k1, k2])
    assert values[0] == values[1] == values[2]  # the model is the same: the same value
    for m, term in ((0, None), (1, k1), (2, k2)):
        want_mu, want_var = _single(k, X, noise, y, Xt, kernel=term)
        np.testing.assert_allclose(mu[m], want_mu, err_msg=f"term {m}", **POST)
        np.testing.assert_allclose(var[m], want_var, err_msg=f"term {m}", **POST)
    sp.check(mu[1] + mu[2], mu[0], "the means of the addends sum to the full mean")
    assert np.all(var[1] > 0.0) and np.all(var[2] > 0.0)
    # the LAPACK reference with another kernel for k* and k**: member 0's own model, its other kernel as the term
    got = tinygp_amd.predict_datasets(k1, [X], [y], [Xt], diags=[noise], predict_kernels=[k2])
    ref = sp.reference(n, d, 0, mr, True)
    sp.check(got[1][0], ref.mean)
    sp.check(got[2][0], ref.var + JITTER)
    # a term under another input transform than the model's lowers the data points differently: the single path
    moved = transforms.Linear(0.5, k1)
    assert small.lower_test(k, moved, X, Xt, small.lower_member(k, X)) is None
    got = tinygp_amd.predict_datasets(k, [X] * 2, [y] * 2, [Xt] * 2, diags=[noise] * 2, predict_kernels=[k1, moved])
    want_mu, want_var = _single(k, X, noise, y, Xt, kernel=moved)
    _same(got[1][1], want_mu, "the single path's own bits")
    _same(got[2][1], want_var, "the single path's own bits")
    _same(got[1][0], mu[1], "its batched neighbour")
    _same(got[2][0], var[1], "its batched neighbour")


# ---- 6. other cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
def test_ragged_sets_with_ragged_test_points(d):
    ns = ds.RAGGED
    counts = (5, 1, 0, None, 5, 1)  # random test points: 0 -> m = 0 (value only), None -> the data set's own points
    Xs = [dn.train(n, d)[0] for n in ns]
    Xts = [None if c is None else (sp.query(n, d, c) if c else Xs[b][:0]) for b, (n, c) in enumerate(zip(ns, counts))]
    ks = [ds.member_kernel(kernels, d, b) for b in range(len(ns))]
    nz = [ds.member_noise(n, d, b) for b, n in enumerate(ns)]
    values, mu, var, info = tinygp_amd.predict_datasets(ks, Xs, [ds.resid(n) for n in ns], Xts, diags=nz,
                                                        return_info=True)
    plain = tinygp_amd.log_probability_datasets(ks, Xs, [ds.resid(n) for n in ns], diags=nz)
    assert np.array_equal(values, plain) and not info.any() and info.dtype == np.int32
    for b, (n, c) in enumerate(zip(ns, counts)):
        if c is None:
            assert mu[b].shape == var[b].shape == (n,)
            want_mu, want_var = _single(ks[b], Xs[b], nz[b], ds.resid(n), Xs[b])
            np.testing.assert_allclose(mu[b], want_mu, **POST)
            np.testing.assert_allclose(var[b], want_var, **POST)
        elif c == 0:
            assert mu[b].shape == var[b].shape == (0,) and mu[b].dtype == np.float64
        else:
            ref = sp.reference(n, d, b, c)
            sp.check(mu[b], ref.mean, f"data set {b}")
            sp.check(var[b], ref.var + JITTER, f"data set {b}")
    # nobody has test points: the values alone
    none = tinygp_amd.predict_datasets(ks, Xs, [ds.resid(n) for n in ns], [X[:0] for X in Xs], diags=nz)
    assert np.array_equal(none[0], plain) and all(v.shape == (0,) for v in none[1] + none[2])


@pytest.mark.parametrize("n,p", ds.FAIL_CASES)
def test_failed_pivot_is_reported_and_stays_in_its_member(n, p):
    d, members = 3, [0, 1, 2]
    Xt = np.asarray(sp.many_points(CHUNK + 2, d)) if n == 65 and p == 0 else sp.query(n, d, 5)  # (once over two chunks)
    X = dn.train(n, d)[0]
    ks = [ds.member_kernel(kernels, d, b) for b in members]
    good = [np.array(ds.member_noise(n, d, b)) for b in members]
    ys = [np.array(ds.resid(n)) for _ in members]

    def run(noise, resid):
        return tinygp_amd.predict_datasets(ks, [X] * 3, resid, [Xt] * 3, diags=noise, return_info=True)

    clean = run(good, ys)
    assert not clean[3].any()
    for bad_value in (-2.0, np.nan):
        noise = [np.array(v) for v in good]
        noise[1][p] = bad_value  # the leading minor is positive definite, K_pp + noise_p < 0: pivot p + 1 fails
        values, mu, var, info = run(noise, ys)
        assert info.tolist() == [0, p + 1, 0], (bad_value, info)
        assert values[1] == -np.inf and np.all(np.isnan(mu[1])) and np.all(np.isnan(var[1]))
        assert mu[1].shape == var[1].shape == (len(Xt),)
        for b in (0, 2):
            assert values[b] == clean[0][b]
            _same(mu[b], clean[1][b], f"neighbour {b}")
            _same(var[b], clean[2][b], f"neighbour {b}")
    resid = [np.array(v) for v in ys]
    resid[1][n // 2] = np.nan
    values, mu, var, info = run(good, resid)
    assert info.tolist() == [0, 0, 0] and values[1] == -np.inf
    assert np.all(np.isnan(mu[1])) and np.all(np.isnan(var[1]))
    for b in (0, 2):
        assert values[b] == clean[0][b]
        _same(mu[b], clean[1][b], f"neighbour {b} of a NaN residual")
        _same(var[b], clean[2][b], f"neighbour {b} of a NaN residual")
    # the shared-points entry reports the same
    noise = np.stack(good)
    noise[1, p] = -2.0
    solver = DirectSolver(ks[0], X, Diagonal(good[0]))
    try:
        values, mu, var, info = solver.predict_batch(ks, ys[0], Xt, noise, return_info=True)
    finally:
        solver.close()
    assert info.tolist() == [0, p + 1, 0] and values[1] == -np.inf and np.all(np.isnan(mu[1])) and np.all(np.isnan(var[1]))
    _same(mu[0], clean[1][0], "neighbour 0")


@pytest.mark.parametrize("d", ds.DS)
def test_above_the_cap_and_without_a_program_is_the_single_path(d):
    n, mr = CAP + 1, 5
    X, diag = dn.train(n, d)
    y, Xt = ds.resid(n), sp.query(n, d, mr)
    ks = [ds.member_kernel(kernels, d, b) for b in range(2)]
    nz = [ds.member_noise(n, d, b) for b in range(2)]
    values, mu, var = tinygp_amd.predict_datasets(ks, [X] * 2, [y] * 2, [Xt] * 2, diags=nz)
    for b in range(2):
        want_mu, want_var = _single(ks[b], X, nz[b], y, Xt)
        _same(mu[b], want_mu, f"member {b}")  # the same path: the same bits
        _same(var[b], want_var, f"member {b}")
        ref = sp.reference(n, d, b, mr)
        np.testing.assert_allclose(mu[b], ref.mean, **POST)
        np.testing.assert_allclose(var[b], ref.var + JITTER, **POST)
        assert ds.within_bar(values[b], ref.value)
    # one such member among small ones: the order of the results is the caller's
    sizes = (17, n, 64)
    sets = tinygp_amd.predict_datasets(ks[1], [dn.train(s, d)[0] for s in sizes], [ds.resid(s) for s in sizes],
                                       [sp.query(s, d, mr) for s in sizes], diags=[ds.member_noise(s, d, 1) for s in sizes])
    _same(sets[1][1], mu[1], "a large data set among small ones")
    for m, s in ((0, 17), (2, 64)):
        sp.check(sets[1][m], sp.reference(s, d, 1, mr).mean)
    # the shared-points entries above the cap: every member on the single path, the same shapes
    solver = DirectSolver(ks[0], X, Diagonal(diag))
    try:
        bv, bmu, bvar = solver.predict_batch(ks, y, Xt, np.stack(nz))
    finally:
        solver.close()
    assert bmu.shape == bvar.shape == (2, mr + 2)
    np.testing.assert_allclose(bmu, np.stack(mu), **POST)
    np.testing.assert_allclose(bvar + JITTER, np.stack(var), **POST)
    # kernels.Custom: no device program
    n = 40
    X, y, Xt, noise = dn.train(n, d)[0], ds.resid(n), sp.query(n, d, mr), ds.member_noise(n, d, 0)
    s = 2.5
    custom = kernels.Custom(lambda a, b: 0.9 * np.exp(-0.5 * np.sum(np.square(a - b)) / s**2))
    assert small.lower_member(custom, X) is None
    got = tinygp_amd.predict_datasets([ks[0], custom], [X] * 2, [y] * 2, [Xt] * 2, diags=[noise] * 2)
    want_mu, want_var = _single(custom, X, noise, y, Xt)
    _same(got[1][1], want_mu, "Custom")
    _same(got[2][1], want_var, "Custom")
    sp.check(got[1][0], sp.reference(n, d, 0, mr).mean)
    same_as = 0.9 * (kernels.ExpSquared(s) if d == 1 else kernels.ExpSquared(s, distance=kernels.L2Distance()))
    other = tinygp_amd.predict_datasets(same_as, [X], [y], [Xt], diags=[noise])
    np.testing.assert_allclose(got[1][1], other[1][0], **POST)
    np.testing.assert_allclose(got[2][1], other[2][0], **POST)
    # a noise model that is not Diagonal: every member on the single path, with that model
    N = np.diag(noise) + 0.01
    dense = GaussianProcess(ks[0], X, noise=Dense(N))
    try:
        dmu, dvar = dense.predict_batch(y, ks, Xt)
        for b, k in enumerate(ks):
            gp = GaussianProcess(k, X, noise=Dense(N))
            want_mu, want_var = gp.predict(y, Xt, return_var=True)
            gp.solver.close()
            np.testing.assert_allclose(dmu[b], want_mu, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(dvar[b], want_var, rtol=1e-12, atol=1e-12)
        assert not np.allclose(dmu[0], sp.reference(n, d, 0, mr).mean, rtol=1e-6, atol=0)  # (another noise model)
    finally:
        dense.solver.close()


def test_quasisep_kernels_raise_the_pinned_error():
    t = np.sort(np.random.default_rng(3).uniform(0.0, 10.0, 30))
    ks = [quasisep.Matern32(1.0 + 0.1 * b) for b in range(2)]
    dense = GaussianProcess(ks[0], t, diag=0.1, solver=DirectSolver)
    try:
        with pytest.raises(NotImplementedError, match="QuasisepSolver"):
            dense.solver.predict_batch(ks, np.zeros(30), t[:5])
        with pytest.raises(NotImplementedError, match="QuasisepSolver"):
            dense.predict_batch(np.zeros(30), [kernels.Matern32(1.0), ks[1]], t[:5])
        with pytest.raises(NotImplementedError, match="QuasisepSolver"):
            tinygp_amd.predict_datasets(ks[0], [t], [np.zeros(30)], [t[:5]], diags=[0.1])
    finally:
        dense.solver.close()
    sparse = GaussianProcess(ks[0], t, diag=0.1)
    with pytest.raises(NotImplementedError, match="has no predict_batch"):
        sparse.predict_batch(np.zeros(30), ks, t[:5])
    sparse.solver.close()


@pytest.mark.parametrize("d", ds.DS)
def test_fp32_inputs_are_computed_in_fp64_and_returned_as_fp32(d):
    n, B, mr = 65, 3, 5
    X32, diag32 = dn.train(n, d, "float32")
    y32, Xt32 = ds.resid(n, "float32"), sp.query(n, d, mr, "float32")
    assert X32.dtype == y32.dtype == Xt32.dtype == np.float32
    ks = [ds.member_kernel(kernels, d, b) for b in range(B)]
    solver = DirectSolver(ks[0], X32, Diagonal(diag32))
    assert solver.dtype == np.float32
    try:
        values, mu, var = solver.predict_batch(ks, y32, Xt32)
        empty = solver.predict_batch([], y32, Xt32)
    finally:
        solver.close()
    assert values.dtype == mu.dtype == var.dtype == np.float32 and mu.shape == (B, mr + 2)
    assert empty[0].shape == (0,) and empty[1].shape == empty[2].shape == (0, mr + 2) and empty[1].dtype == np.float32
    # the same numbers as the float64 call on the rounded inputs, rounded once
    solver = DirectSolver(ks[0], X32.astype(np.float64), Diagonal(diag32.astype(np.float64)))
    try:
        v64, mu64, var64 = solver.predict_batch(ks, y32.astype(np.float64), Xt32.astype(np.float64))
    finally:
        solver.close()
    assert np.array_equal(values, v64.astype(np.float32)) and np.array_equal(mu, mu64.astype(np.float32))
    assert np.array_equal(var, var64.astype(np.float32))
    sets = tinygp_amd.predict_datasets(ks, [X32] * B, [y32] * B, [Xt32] * B, diags=[diag32] * B)
    assert sets[0].dtype == np.float64 and sets[1][0].dtype == sets[2][0].dtype == np.float32
    assert np.array_equal(sets[0], v64) and np.array_equal(sets[1][1], mu[1])
    jitter32 = np.sqrt(np.finfo(np.float32).eps)  # condition() adds sqrt(eps) of the data's dtype
    assert np.array_equal(sets[2][1], (var64[1] + jitter32).astype(np.float32))
    gp = GaussianProcess(ks[1], X32, diag=diag32)
    want_mu, want_var = gp.predict(y32, Xt32, return_var=True)
    gp.solver.close()
    np.testing.assert_allclose(sets[1][1], want_mu, **dn.posterior_bar(np.float32))
    np.testing.assert_allclose(sets[2][1], want_var, **dn.posterior_bar(np.float32))


@pytest.mark.parametrize("d", ds.DS)
def test_means_and_include_mean(d):
    n, mr, B = 33, 5, 3
    X, y, Xt = dn.train(n, d)[0], ds.resid(n), sp.query(n, d, mr)
    m = mr + 2
    ks = [ds.member_kernel(kernels, d, b) for b in range(B)]
    nz = [ds.member_noise(n, d, b) for b in range(B)]
    vec, tvec = np.linspace(-0.3, 0.4, n), np.linspace(0.1, 0.2, m)

    def run(**kwargs):
        return tinygp_amd.predict_datasets(ks, [X] * B, [y] * B, [Xt] * B, diags=nz, **kwargs)

    zero = run()
    got = run(means=[None, 0.7, vec], test_means=[None, None, tvec])
    off = run(means=[None, 0.7, vec], test_means=[None, None, 0.25], include_mean=False)
    bare = run(means=[None, 0.7, vec], include_mean=False)  # (no test mean needed when none is added)
    # member 1: GaussianProcess(..., mean=0.7); member 2: the residual y - vec, the test mean added
    gp = GaussianProcess(ks[1], X, diag=nz[1], mean=0.7)
    want = gp.predict(y, Xt, return_var=True)
    want_off = gp.predict(y, Xt, include_mean=False)
    value = float(gp.log_probability(y))
    gp.solver.close()
    np.testing.assert_allclose(got[1][1], want[0], **POST)
    np.testing.assert_allclose(got[2][1], want[1], **POST)
    np.testing.assert_allclose(off[1][1], want_off, **POST)
    assert ds.within_bar(got[0][1], value) and got[0][1] != zero[0][1]
    _same(got[1][1], off[1][1] + 0.7, "a scalar mean is added to the predictions")
    gp = GaussianProcess(ks[2], X, diag=nz[2])
    want_mu, want_var = gp.predict(y - vec, Xt, return_var=True)
    gp.solver.close()
    np.testing.assert_allclose(off[1][2], want_mu, **POST)
    np.testing.assert_allclose(got[2][2], want_var, **POST)
    _same(got[1][2], off[1][2] + tvec, "a vector mean needs the mean at the test points")
    _same(bare[1][2], off[1][2], "include_mean=False")
    for b in range(B):
        _same(got[2][b], zero[2][b], "the variances do not see the mean")
    _same(got[1][0], zero[1][0], "a member without a mean")
    with pytest.raises(ValueError, match=r"means\[2\] of data set 2 is a vector"):
        run(means=[None, 0.7, vec])
    # GaussianProcess.predict_batch: (B, M), constants added, this GP's mean function without `means`
    gp = GaussianProcess(ks[0], X, diag=nz[0], mean=0.3)
    try:
        mu, var = gp.predict_batch(y, ks, Xt, diags=np.stack(nz), means=np.array([0.0, 0.7, -0.2]))
        only = gp.predict_batch(y, ks, Xt, diags=np.stack(nz), means=np.array([0.0, 0.7, -0.2]), return_var=False)
        own = gp.predict_batch(y, ks[:1], Xt)
        own_off = gp.predict_batch(y, ks[:1], Xt, include_mean=False, return_var=False)
        at_data = gp.predict_batch(y, ks, None, diags=np.stack(nz), return_var=False)
        want_own = gp.predict(y, Xt, return_var=True)
    finally:
        gp.solver.close()
    assert mu.shape == var.shape == only.shape == (B, m) and at_data.shape == (B, n) and own_off.shape == (1, m)
    _same(only, mu, "return_var=False")
    np.testing.assert_allclose(mu[1], want[0], **POST)
    np.testing.assert_allclose(var[1], want[1], **POST)
    _same(mu[0], zero[1][0], "a zero mean")
    np.testing.assert_allclose(own[0][0], want_own[0], **POST)
    np.testing.assert_allclose(own[1][0], want_own[1], **POST)
    np.testing.assert_allclose(own_off[0] + 0.3, own[0][0], rtol=1e-14, atol=1e-14)


def test_the_c_call_names_the_member_it_refuses():
    d, n = 3, 9
    X = dn.train(n, d)[0]
    members = [small.lower_member(ds.member_kernel(kernels, d, b), X) + (ds.member_noise(n, d, b), ds.resid(n))
               for b in range(2)]
    Q = np.asarray(dn.query_points(4, d)[0])
    other = ds.member_kernel(kernels, d, 0, other=True).program()
    pp = small.pack_predict(members, [Q, Q + 1.0], [None, other])
    ctx = tinygp_amd._ffi.default_ctx()
    good = small.run_packed_predict(ctx, pp)
    assert not good[1].any() and good[2].shape == good[3].shape == (8,)
    with pytest.raises(ValueError, match=r"member 1: negative number of test points \(-1\)"):
        small.run_packed_predict(ctx, pp._replace(m=np.array([4, -1], dtype=np.int32)))
    with pytest.raises(ValueError, match=r"member 1: test rows 5 \.\. 9 lie outside Xt \(8 rows\)"):
        small.run_packed_predict(ctx, pp._replace(xt_off=np.array([0, 5], dtype=np.int64)))
    with pytest.raises(ValueError, match=r"member 0: test rows -1 \.\. 3 lie outside Xt"):
        small.run_packed_predict(ctx, pp._replace(xt_off=np.array([-1, 4], dtype=np.int64)))
    with pytest.raises(ValueError, match=r"member 1: negative offset into the predictions \(-4\)"):
        small.run_packed_predict(ctx, pp._replace(out_off=np.array([0, -4], dtype=np.int64)))
    broken = pp.pred_progs.copy()
    broken["op"][-1] = 9999
    with pytest.raises(ValueError, match=r"member 1: prediction program: "):
        small.run_packed_predict(ctx, pp._replace(pred_progs=broken))
    with pytest.raises(ValueError, match=r"member 1: n must be 1 \.\. "):  # the value call's own texts
        small.run_packed_predict(ctx, pp._replace(packed=pp.packed._replace(n=np.array([n, 0], dtype=np.int32))))
    again = small.run_packed_predict(ctx, pp)  # a refused call leaves nothing behind
    for a, b in zip(good, again):
        assert np.array_equal(a, b)
