"""Conditional covariance and joint posterior draws of batches of small dense GPs in one launch, one workgroup per member
(``csrc/small.hip``, ``tgp_small_condition``) through ``tinygp_amd.condition_datasets``,
``tinygp_amd.sample_conditional_datasets``, ``DirectSolver.condition_batch`` and the two ``GaussianProcess`` methods.

Inputs and references: ``_dense_small_condition.py`` (float64 LAPACK, its own conditions asserted) and, for every leaf
and operator, the single path ``GaussianProcess.condition``.  Bars: 1e-8 for the value; the project's fp64 solve bar
against the reference (rtol 1e-10 plus atol 1e-10 max|want| per member) for mean, covariance and draws at tau = 0.1;
the posterior bar (rtol = atol = 5e-7) against the single path and with the default jitter; value bits, symmetry,
independence and the routes to the single path are held with tolerance zero.

Measured on an MI355X (largest fraction of a bar over every case): see DESIGN 12.3."""
import numpy as np
import pytest

import tinygp_amd
from oracle import tinygp_np as o
from tinygp_amd import GaussianProcess, _ffi, kernels, transforms
from tinygp_amd.kernels import quasisep
from tinygp_amd.noise import Dense, Diagonal
from tinygp_amd.solvers import DirectSolver, QuasisepSolver, small

import _dense_np as dn
import _dense_small as ds
import _dense_small_predict as sp
import _dense_small_condition as sc

pytestmark = pytest.mark.gpu

CAP = ds.CAP
TAU = sc.TAU
POST = dn.posterior_bar(np.float64)
condition = tinygp_amd.condition_datasets
sample = tinygp_amd.sample_conditional_datasets


def _same(a, b, what):
    assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), (what, a, b)


def _inputs(n, d, members, m):
    """The arguments of the two ``*_datasets`` calls for members b of the (n, d) inputs at the case's m test points."""
    B = len(members)
    return ([ds.member_kernel(kernels, d, b) for b in members], [dn.train(n, d)[0]] * B, [ds.resid(n)] * B,
            [sc.test_points(n, d, m)] * B), dict(diags=[ds.member_noise(n, d, b) for b in members])


def _sets(n, d, members, m, tau=TAU, **kwargs):
    args, kw = _inputs(n, d, members, m)
    return condition(*args, test_diags=[tau] * len(members), **kw, **kwargs)


def _draws(n, d, members, m, S, tau=TAU, **kwargs):
    args, kw = _inputs(n, d, members, m)
    return sample(*args, key=None, shape=(S,), xi=[sc.normals(n, m)[:S]] * len(members),
                  test_diags=[tau] * len(members), **kw, **kwargs)


def _batch(n, d, members, m, **kwargs):
    """``DirectSolver.condition_batch`` of the same members over shared points."""
    X, diag = dn.train(n, d)
    solver = DirectSolver(ds.member_kernel(kernels, d, 0), X, Diagonal(diag))
    try:
        return solver.condition_batch([ds.member_kernel(kernels, d, b) for b in members], ds.resid(n),
                                      sc.test_points(n, d, m), np.stack([ds.member_noise(n, d, b) for b in members]),
                                      **kwargs)
    finally:
        solver.close()


def _single(model, X, diag, y, Xt, tau=None, xi=None, **kwargs):
    """``(log_probability, gp.loc, gp.covariance, loc + L xi)`` of the single call, L from LAPACK on its covariance."""
    gp = GaussianProcess(model, X, diag=diag, **{k: kwargs.pop(k) for k in ("mean",) if k in kwargs})
    try:
        value, cond = gp.condition(y, Xt, diag=tau, **kwargs)
        loc, cov = np.asarray(cond.loc), np.asarray(cond.covariance)
        f = None if xi is None else small.host_draws(loc, cov, xi)[0]
        return float(value), loc, cov, f
    finally:
        gp.solver.close()


# ---- 1. parity with the LAPACK reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
@pytest.mark.parametrize("part", range(4))
def test_parity_with_the_lapack_reference_at_the_edges(part, d):
    worst = dict(value=0.0, mean=0.0, cov=0.0, draws=0.0)
    for n, m in sc.SHAPES[part::4]:
        for B, S in ((1, 1), (3, 5)):
            values, mu, cov, info = _sets(n, d, range(B), m, return_info=True)
            v2, f, info2, cinfo = _draws(n, d, range(B), m, S, return_info=True)
            bv, bmu, bcov, bf, binfo, bcinfo = _batch(n, d, range(B), m, test_diag=TAU, xi=sc.normals(n, m)[:S],
                                                      return_info=True)
            assert not info.any() and not info2.any() and not cinfo.any() and not binfo.any() and not bcinfo.any()
            assert bmu.shape == (B, m) and bcov.shape == (B, m, m) and bf.shape == (B, S, m)
            refs = [sc.reference(n, d, b, m) for b in range(B)]
            for b, ref in enumerate(refs):
                worst["value"] = max(worst["value"], abs(values[b] - ref.value) / (ds.BAR * max(1.0, abs(ref.value))))
                worst["mean"] = max(worst["mean"], sp.bars(mu[b], ref.mean))
                worst["cov"] = max(worst["cov"], sp.bars(cov[b], ref.cov))
                worst["draws"] = max(worst["draws"], sp.bars(f[b], ref.draws[:S]))
            print(f"n={n} m={m} d={d} B={B}: worst fraction of the bars "
                  + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
            for b, ref in enumerate(refs):
                what = f"n={n} m={m} d={d} B={B} S={S} member {b}"
                assert mu[b].shape == (m,) and cov[b].shape == (m, m) and f[b].shape == (S, m), what
                assert ds.within_bar(values[b], ref.value), what
                sp.check(mu[b], ref.mean, what)
                sp.check(cov[b], ref.cov, what)
                sp.check(f[b], ref.draws[:S], what)
                # the three entry points: the same bits
                assert values[b] == v2[b] == bv[b], what
                _same(bmu[b], mu[b], what)
                _same(bcov[b], cov[b], what)
                _same(bf[b], f[b], what)


@pytest.mark.parametrize("d", ds.DS)
@pytest.mark.parametrize("n,m", sc.JITTER_SHAPES)
def test_default_jitter(n, m, d):
    """``test_diags=None``: Sigma* is conditioned up to 7.7e9.  The covariance is held entry by entry; a draw goes
    through chol(Sigma*), so the float64 reference itself is e64 away from the long-double one, and the device gets
    8 e64 as in ``test_gpu_4_quasisep_range.py``."""
    B, S = 3, 5
    args, kw = _inputs(n, d, range(B), m)
    values, mu, cov, info = condition(*args, **kw, return_info=True)
    v2, f, info2, cinfo = sample(*args, key=None, shape=(S,), xi=[sc.normals(n, m)[:S]] * B, **kw, return_info=True)
    assert not info.any() and not info2.any() and not cinfo.any()
    for b in range(B):
        ref = sc.reference(n, d, b, m, True)
        what = f"n={n} m={m} d={d} member {b}"
        off = ~np.eye(m, dtype=bool)
        sp.check(np.where(off, cov[b], 0.0), np.where(off, ref.cov, 0.0), what)
        np.testing.assert_allclose(cov[b], ref.cov, **POST, err_msg=what)
        want, e64 = ref.draws[:S], ref.figures.e64[:S]
        bound = np.maximum(POST["atol"] + POST["rtol"] * np.abs(want), 8.0 * e64)
        err = np.abs(f[b] - want)
        print(f"{what}: cond(Sigma*) {ref.figures.cond_star:.3g}, draws: largest error / bound "
              f"{float(np.max(err / bound)):.3g}, largest error / (8 e64) {float(np.max(err / np.maximum(8.0 * e64, 1e-300))):.3g}")
        assert np.all(err <= bound), what


# ---- 2. tolerance zero ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
def test_value_bits_symmetry_and_partial_calls(d):
    for n, m in ((17, 7), (65, 63), (3, 189), (CAP - 1, 1)):
        args, kw = _inputs(n, d, range(3), m)
        plain = tinygp_amd.log_probability_datasets(*args[:3], **kw)
        values, mu, cov = _sets(n, d, range(3), m)
        v2, f = _draws(n, d, range(3), m, 5)
        bv, bmu, bcov, bf = _batch(n, d, range(3), m, test_diag=TAU, xi=sc.normals(n, m)[:5])
        _, cmu, ccov, none = _batch(n, d, range(3), m, test_diag=TAU)  # covariance only
        _, dmu, nocov, df = _batch(n, d, range(3), m, test_diag=TAU, xi=sc.normals(n, m)[:5], return_cov=False)
        assert none is None and nocov is None
        for b in range(3):
            what = f"n={n} m={m} d={d} member {b}"
            assert values[b] == plain[b] == v2[b] == bv[b], what
            assert np.array_equal(cov[b], cov[b].T), what
            _same(ccov[b], cov[b], what), _same(cmu[b], mu[b], what), _same(dmu[b], mu[b], what)
            _same(df[b], f[b], what), _same(bf[b], f[b], what), _same(bcov[b], cov[b], what)


@pytest.mark.parametrize("d", ds.DS)
def test_a_members_bits_do_not_depend_on_the_batch(d):
    n, m, me, S = 17, 7, 2, 3
    k, X, y, Q = ds.member_kernel(kernels, d, me), dn.train(n, d)[0], ds.resid(n), sc.test_points(n, d, m)
    nz, z = ds.member_noise(n, d, me), sc.normals(n, m)

    def run(ks, Xs, ys, Qs, nzs, zs, at):
        v, mu, cov = condition(ks, Xs, ys, Qs, diags=nzs, test_diags=[TAU] * len(ks))
        v2, f = sample(ks, Xs, ys, Qs, key=None, shape=(len(zs[at]),), xi=zs, diags=nzs, test_diags=[TAU] * len(ks))
        assert v[at] == v2[at]
        return v[at], mu[at], cov[at], f[at]

    def same(a, b, what):
        assert a[0] == b[0], what
        for x, w in zip(a[1:], b[1:]):
            _same(x, w, what)

    alone = run([k], [X], [y], [Q], [nz], [z[:S]], 0)
    again = run([k], [X], [y], [Q], [nz], [z[:S]], 0)
    same(alone, again, "across calls")
    # at every position of B = 3, beside a neighbour at the cap
    nb_n, nb_m = CAP - 8, 8
    other = (ds.member_kernel(kernels, d, 0, other=True), dn.train(nb_n, d)[0], ds.resid(nb_n),
             sc.test_points(nb_n, d, nb_m), ds.member_noise(nb_n, d, 0), sc.normals(nb_n, nb_m)[:S])
    mine = (k, X, y, Q, nz, z[:S])
    for at in range(3):
        rows = [other] * 3
        rows[at] = mine
        same(alone, run(*[list(c) for c in zip(*rows)], at), f"position {at} of 3")
    # inside B = 300 of mixed structures, lengths and m
    rng = np.random.default_rng([31, d])
    cols = [[], [], [], [], []]
    for b in range(300):
        nn, mm = int(rng.integers(1, 60)), int(rng.integers(1, 40))
        row = (ds.member_kernel(kernels, d, b % 5, other=bool(b % 2)), dn.train(nn, d)[0], ds.resid(nn),
               dn.query_points(mm, d)[0], ds.member_noise(nn, d, b % 3))
        for c, v in zip(cols, (k, X, y, Q, nz) if b == 137 else row):
            c.append(v)
    v, mu, cov = condition(*cols[:4], diags=cols[4], test_diags=[TAU] * 300)
    assert v[137] == alone[0]
    _same(mu[137], alone[1], "inside 300"), _same(cov[137], alone[2], "inside 300")
    # .. and with ragged S, which is the C call's own (the public calls take one shape): the first 40 of them, member 11
    lows = [small.lower_member(kk, XX) for kk, XX in zip(cols[0][:40], cols[1][:40])]
    members = [(low[0], low[1], nn, yy) for low, nn, yy in zip(lows, cols[4], cols[2])]
    tests = [small.lower_test(kk, None, XX, QQ, low)[0] for kk, XX, QQ, low in zip(cols[0], cols[1], cols[3], lows)]
    zs = [rng.standard_normal((b % 4, len(t))) for b, t in enumerate(tests)]
    low = small.lower_member(k, X)
    members[11], tests[11], zs[11] = (low[0], low[1], nz, y), small.lower_test(k, None, X, Q, low)[0], np.array(z[:S])
    pc = small.pack_condition(members, tests, [np.full(len(t), TAU) for t in tests], None, zs)
    assert pc.ndraw.tolist()[:12] == [0, 1, 2, 3] * 2 + [0, 1, 2, S]
    out, info, cinfo, fm, fc, fs = small.run_packed_condition(_ffi.default_ctx(), pc)
    assert not info.any() and not cinfo.any() and out[11] == alone[0]
    at, co, xo = int(pc.pp.out_off[11]), int(pc.cov_off[11]), int(pc.xi_off[11])
    _same(fm[at:at + m], alone[1], "ragged S"), _same(fc[co:co + m * m].reshape(m, m), alone[2], "ragged S")
    _same(fs[xo:xo + S * m].reshape(S, m), alone[3], "ragged S")


@pytest.mark.parametrize("d", ds.DS)
def test_a_draws_bits_depend_on_its_own_normals_alone(d):
    for n, m in ((17, 7), (3, 129), (64, 128)):
        z = sc.normals(n, m)
        nine = _draws(n, d, [1], m, 9)[1][0]
        assert nine.shape == (9, m)
        args, kw = _inputs(n, d, [1], m)
        for s in (0, 3, 4, 8):
            one = sample(*args, key=None, shape=(1,), xi=[z[s:s + 1]], test_diags=[TAU], **kw)[1][0]
            _same(one[0], nine[s], f"n={n} m={m} draw {s} alone")
        moved = sample(*args, key=None, shape=(9,), xi=[z[::-1]], test_diags=[TAU], **kw)[1][0]
        _same(moved[::-1], nine, f"n={n} m={m}: other positions")


# ---- 3. consistency with the predictions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
def test_mean_and_diagonal_agree_with_predict_datasets(d):
    for n, m in ((17, 7), (65, 63), (128, 64)):
        args, kw = _inputs(n, d, range(3), m)
        _, pmu, pvar = tinygp_amd.predict_datasets(*args, **kw)
        _, mu, cov = _sets(n, d, range(3), m)
        for b in range(3):
            sp.check(mu[b], pmu[b], f"n={n} m={m} member {b}: mean")
            sp.check(np.diag(cov[b]) - TAU, pvar[b] - sc.JITTER, f"n={n} m={m} member {b}: variance")


# ---- 4. against the single path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", ds.LEAF_DS)
def test_every_leaf_and_operator_against_the_single_path(D):
    X, y = ds.leaf_points(D), ds.resid(ds.LEAF_N)
    Q = np.random.default_rng([13, D]).uniform(0.0, 3.0 / D, (9,) + np.shape(X)[1:])
    z = np.random.default_rng([14, D]).standard_normal((3, 9))
    members = ds.leaf_members(kernels, transforms)
    B = len(members)
    assert B == 17
    ks, nzs = [mem[1] for mem in members], [ds.leaf_noise() * (1.0 + 0.1 * b) for b in range(B)]
    values, mu, cov = condition(ks, [X] * B, [y] * B, [Q] * B, diags=nzs, test_diags=[TAU] * B)
    _, f = sample(ks, [X] * B, [y] * B, [Q] * B, key=None, shape=(3,), xi=[z] * B, diags=nzs, test_diags=[TAU] * B)
    for b, (name, k, _) in enumerate(members):
        want = _single(k, X, nzs[b], y, Q, TAU, z)
        assert ds.within_bar(values[b], want[0]), name
        np.testing.assert_allclose(mu[b], want[1], **POST, err_msg=name)
        np.testing.assert_allclose(cov[b], want[2], **POST, err_msg=name)
        np.testing.assert_allclose(f[b], want[3], **POST, err_msg=name)


@pytest.mark.parametrize("d", ds.DS)
def test_each_addend_of_a_sum_as_the_prediction_kernel(d):
    n, m = 33, 9
    X, y, Q, nz = dn.train(n, d)[0], ds.resid(n), sc.test_points(n, d, m), ds.member_noise(n, d, 0)
    k1, k2 = ds.member_kernel(kernels, d, 0), ds.member_kernel(kernels, d, 1, other=True)
    full = k1 + k2
    values, mu, cov = condition([full] * 3, [X] * 3, [y] * 3, [Q] * 3, diags=[nz] * 3, test_diags=[TAU] * 3,
                                predict_kernels=[None, k1, k2])
    assert values[0] == values[1] == values[2]
    for b, pk in enumerate((None, k1, k2)):
        want = _single(full, X, nz, y, Q, TAU, kernel=pk)
        np.testing.assert_allclose(mu[b], want[1], **POST)
        np.testing.assert_allclose(cov[b], want[2], **POST)
    np.testing.assert_allclose(mu[1] + mu[2], mu[0], **POST)


# ---- 5. shapes and routes ---------------------------------------------------------------------------------------------------
def test_ragged_sets_none_test_points_means_and_fp32():
    d = 3
    k = ds.member_kernel(kernels, d, 0)
    ns, ms = (5, 40, 1, 17), (7, 0, 3, None)
    Xs, ys = [dn.train(n, d)[0] for n in ns], [ds.resid(n) for n in ns]
    Qs = [None if m is None else (dn.query_points(m, d)[0] if m else np.empty((0, 3))) for m in ms]
    nzs = [ds.member_noise(n, d, 0) for n in ns]
    taus = [0.1, None, np.linspace(0.1, 0.2, 3), 0.05]
    values, mu, cov = condition(k, Xs, ys, Qs, diags=nzs, test_diags=taus)
    assert [c.shape for c in cov] == [(7, 7), (0, 0), (3, 3), (17, 17)] and [len(v) for v in mu] == [7, 0, 3, 17]
    for b in (0, 2, 3):
        want = _single(k, Xs[b], nzs[b], ys[b], Xs[b] if Qs[b] is None else Qs[b], taus[b])
        assert ds.within_bar(values[b], want[0])
        np.testing.assert_allclose(mu[b], want[1], **POST)
        np.testing.assert_allclose(cov[b], want[2], **POST)
    assert values[1] == tinygp_amd.log_probability_datasets(k, Xs[1:2], ys[1:2], diags=nzs[1:2])[0]
    # ragged S is the C call's (test above); shape () and (2, 3) here, and the generator's order
    v2, f = sample(k, Xs, ys, Qs, key=5, shape=(2, 3), diags=nzs, test_diags=taus)
    assert [s.shape for s in f] == [(2, 3, 7), (2, 3, 0), (2, 3, 3), (2, 3, 17)] and np.array_equal(v2, values)
    rng = np.random.default_rng(5)
    xi = [rng.standard_normal((6, m)) for m in (7, 0, 3, 17)]
    _, g = sample(k, Xs, ys, Qs, key=None, shape=(6,), xi=xi, diags=nzs, test_diags=taus)
    for a, b in zip(f, g):
        _same(a.reshape(6, -1), b, "the generator is read member by member")
    assert sample(k, Xs, ys, Qs, key=5, diags=nzs, test_diags=taus)[1][0].shape == (7,)
    # means: a scalar is added, a vector needs test_means, include_mean=False adds nothing
    base = condition(k, Xs[:1], [ys[0] - 0.5], Qs[:1], diags=nzs[:1], test_diags=[0.1])
    with_mean = condition(k, Xs[:1], ys[:1], Qs[:1], diags=nzs[:1], test_diags=[0.1], means=[0.5])
    assert with_mean[0][0] == base[0][0]
    _same(with_mean[1][0], base[1][0] + 0.5, "scalar mean"), _same(with_mean[2][0], base[2][0], "scalar mean")
    vec = condition(k, Xs[:1], ys[:1], Qs[:1], diags=nzs[:1], test_diags=[0.1], means=[np.full(5, 0.5)],
                    test_means=[np.arange(7.0)])
    _same(vec[1][0], base[1][0] + np.arange(7.0), "vector mean")
    bare = condition(k, Xs[:1], ys[:1], Qs[:1], diags=nzs[:1], test_diags=[0.1], means=[np.full(5, 0.5)],
                     include_mean=False)
    _same(bare[1][0], base[1][0], "include_mean=False")
    with pytest.raises(ValueError, match=r"means\[0\] of data set 0 is a vector"):
        condition(k, Xs[:1], ys[:1], Qs[:1], diags=nzs[:1], means=[np.full(5, 0.5)])
    # fp32 inputs: computed in fp64, returned as fp32
    X32, y32 = dn.train(17, d, "float32")[0], ds.resid(17, "float32")
    v32, mu32, cov32 = condition(k, [X32], [y32], [Qs[0].astype(np.float32)], diags=[ds.member_noise(17, d, 0, "float32")])
    assert mu32[0].dtype == cov32[0].dtype == np.float32 and np.isfinite(v32[0])
    want = _single(k, X32, ds.member_noise(17, d, 0, "float32"), y32, Qs[0].astype(np.float32))
    np.testing.assert_allclose(cov32[0], want[2], **dn.posterior_bar(np.float32))
    np.testing.assert_allclose(mu32[0], want[1], **dn.posterior_bar(np.float32))


def test_gaussian_process_methods():
    n, d, m = 17, 3, 7
    X, nz0 = dn.train(n, d)
    y, Q = ds.resid(n), sc.test_points(n, d, m)
    ks = [ds.member_kernel(kernels, d, b) for b in range(3)]
    gp = GaussianProcess(ks[0], X, diag=nz0, mean=0.25)
    try:
        mu, cov = gp.condition_batch(y, ks, Q)
        assert mu.shape == (3, m) and cov.shape == (3, m, m)
        want = _single(ks[1], X, nz0, y, Q, mean=0.25)
        np.testing.assert_allclose(mu[1], want[1], **POST)
        np.testing.assert_allclose(cov[1], want[2], **POST)
        f = gp.sample_conditional_batch(y, ks, Q, key=3, shape=(2, 2), diag=TAU)
        assert f.shape == (3, 2, 2, m) and np.all(np.isfinite(f))
        xi = np.random.default_rng(3).standard_normal((3, 4, m))
        got = gp.solver.condition_batch(ks, y - 0.25, Q, test_diag=TAU, xi=xi, return_cov=False)[3] + 0.25
        _same(f.reshape(3, 4, m), got, "the normals are (B, R, M) from the generator")
        assert gp.sample_conditional_batch(y, ks, None, key=3, diag=TAU).shape == (3, n)
        with pytest.raises(TypeError, match="has no sample_conditional"):  # unchanged
            gp.sample_conditional(y, Q, key=1)
    finally:
        gp.solver.close()
    t = np.sort(np.random.default_rng(1).uniform(0, 5, 9))
    qgp = GaussianProcess(quasisep.Matern32(1.0), t, diag=0.1)
    assert isinstance(qgp.solver, QuasisepSolver)
    with pytest.raises(NotImplementedError, match="has no condition_batch"):
        qgp.condition_batch(np.zeros(9), [quasisep.Matern32(1.0)])
    with pytest.raises(NotImplementedError, match="has no condition_batch"):
        qgp.sample_conditional_batch(np.zeros(9), [quasisep.Matern32(1.0)], key=1)


def test_routes_to_the_single_path_carry_that_calls_bits():
    d = 3
    k = ds.member_kernel(kernels, d, 0)
    n, m = CAP - 3, 4  # n + m = cap + 1
    X, y, Q, nz = dn.train(n, d)[0], ds.resid(n), sc.test_points(n, d, m), ds.member_noise(n, d, 0)
    z = sc.normals(n, m)[:2]
    custom = kernels.Custom(lambda a, b: 1.2 * np.exp(-0.5 * np.sum(np.square(a - b))))
    other_tf = transforms.Linear(0.5, ds.member_kernel(kernels, d, 0, other=True))
    Xs, ys, Qs, nzs = [X, X[:9], X[:9]], [y, y[:9], y[:9]], [Q, Q, Q], [nz, nz[:9], nz[:9]]
    ks, pks = [k, custom, k], [None, None, other_tf]
    values, mu, cov = condition(ks, Xs, ys, Qs, diags=nzs, test_diags=[TAU] * 3, predict_kernels=pks)
    _, f = sample(ks, Xs, ys, Qs, key=None, shape=(2,), xi=[z] * 3, diags=nzs, test_diags=[TAU] * 3, predict_kernels=pks)
    for b in range(3):
        want = _single(ks[b], Xs[b], nzs[b], ys[b], Qs[b], TAU, z, kernel=pks[b])
        assert values[b] == want[0], b
        _same(mu[b], want[1], b), _same(cov[b], want[2], b), _same(f[b], want[3], b)
    # DirectSolver.condition_batch: all members batched or none (noise.Dense, n + m above the cap)
    solver = DirectSolver(k, X[:9], Dense(np.diag(nz[:9])))
    try:
        bv, bmu, bcov, bf = solver.condition_batch([k, k], y[:9], Q, test_diag=TAU, xi=z)
        want = _single(k, X[:9], nz[:9], y[:9], Q, TAU, z)
        np.testing.assert_allclose(bmu[1], want[1], **POST), np.testing.assert_allclose(bcov[0], want[2], **POST)
        np.testing.assert_allclose(bf[1], want[3], **POST)
    finally:
        solver.close()
    with pytest.raises(NotImplementedError, match="QuasisepSolver"):
        condition(quasisep.Matern32(1.0), [np.arange(4.0)], [np.zeros(4)], [np.arange(3.0)], diags=[0.1])


# ---- 6. failures, each confined to its member -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", ds.FAIL_CASES)
def test_a_failed_data_block_is_confined_to_its_member(n, p):
    d, m = 1, 3
    args, kw = _inputs(n, d, range(3), m)
    good = _sets(n, d, range(3), m)
    gf = _draws(n, d, range(3), m, 2)[1]
    for kind in ("pivot", "nan noise", "nan resid"):
        nzs, ys = [np.array(v) for v in kw["diags"]], [np.array(v) for v in args[2]]
        if kind == "pivot":
            nzs[1][p] = -10.0
        elif kind == "nan noise":
            nzs[1][p] = np.nan
        else:
            ys[1][p] = np.nan
        values, mu, cov, info = condition(args[0], args[1], ys, args[3], diags=nzs, test_diags=[TAU] * 3, return_info=True)
        v2, f, info2, cinfo = sample(args[0], args[1], ys, args[3], key=None, shape=(2,), xi=[sc.normals(n, m)[:2]] * 3,
                                     diags=nzs, test_diags=[TAU] * 3, return_info=True)
        assert values[1] == -np.inf and v2[1] == -np.inf, kind
        if kind != "nan resid":  # (n + m above the cap: the single path's own info)
            assert (info[1] == p + 1 == info2[1]) if n + m <= CAP else (info[1] != 0 and info2[1] != 0), (kind, info)
        assert np.all(np.isnan(mu[1])) and np.all(np.isnan(cov[1])) and np.all(np.isnan(f[1])), kind
        for b in (0, 2):
            assert values[b] == good[0][b] and info[b] == 0 and cinfo[b] == 0, kind
            _same(mu[b], good[1][b], kind), _same(cov[b], good[2][b], kind), _same(f[b], gf[b], kind)


@pytest.mark.parametrize("n,m,q", [(65, 65, 0), (65, 65, 1), (65, 65, 64), (3, 129, 63), (3, 129, 64)])
def test_a_failed_conditional_pivot_gives_nan_draws_only(n, m, q):
    """tau_q = -(pk(x*_q, x*_q) + 1): the leading q x q block of Sigma* is positive definite (a Schur complement of a
    positive definite matrix plus 0.1) and entry (q, q) is below -1, so ``cond_info = q + 1`` follows from the inputs."""
    d = 3
    args, kw = _inputs(n, d, range(3), m)
    taus = [np.full(m, TAU) for _ in range(3)]
    xq = np.asarray(args[3][1][q:q + 1], dtype=np.float64)
    kqq = float(ds.member_kernel(o, d, 1)(xq, xq)[0, 0])
    taus[1][q] = -(kqq + 1.0)
    values, mu, cov = condition(*args, test_diags=taus, **kw)
    v2, f, info, cinfo = sample(*args, key=None, shape=(3,), xi=[sc.normals(n, m)[:3]] * 3, test_diags=taus, **kw,
                                return_info=True)
    good = _sets(n, d, range(3), m)
    gf = _draws(n, d, range(3), m, 3)[1]
    assert info.tolist() == [0, 0, 0] and cinfo.tolist() == [0, q + 1, 0]
    assert np.all(np.isnan(f[1])) and v2[1] == values[1] == good[0][1]
    ref = sc.reference(n, d, 1, m)
    want = np.array(ref.cov)
    want[q, q] += taus[1][q] - TAU
    sp.check(mu[1], ref.mean), sp.check(cov[1], want)
    for b in (0, 2):
        _same(f[b], gf[b], b), _same(cov[b], good[2][b], b)


def test_every_new_argument_error_of_the_c_call_names_its_member():
    d, n, m = 3, 9, 4
    members = [small.lower_member(ds.member_kernel(kernels, d, b), dn.train(n, d)[0]) + (ds.member_noise(n, d, b), ds.resid(n))
               for b in range(2)]
    Q = np.asarray(dn.query_points(m, d)[0])
    z = np.zeros((2, m))
    ctx = _ffi.default_ctx()

    def call(pc, **over):
        pp, p = pc.pp, pc.pp.packed
        nb = len(p.n)
        a = dict(m=pp.m, xt_off=pp.xt_off, tvec_off=pp.out_off, mean_off=pp.out_off, cov_off=pc.cov_off, ndraw=pc.ndraw,
                 xi_off=pc.xi_off, xi=pc.xi, xt_rows=pp.Xt.shape[0], pred=None, pred_off=None, samples=np.empty(64))
        a.update(over)
        info, cinfo, out = np.zeros(nb, np.int32), np.zeros(nb, np.int32), np.empty(nb)
        mean, cov = np.empty(64), np.empty(256)
        pred_off = None if a["pred_off"] is None else np.ascontiguousarray(a["pred_off"], np.int32)
        keep = [np.ascontiguousarray(a[k], np.int64) for k in ("xt_off", "tvec_off", "mean_off", "cov_off", "xi_off")]
        keep32 = [np.ascontiguousarray(a[k], np.int32) for k in ("m", "ndraw")]
        rc = _ffi.lib().tgp_small_condition(
            ctx.handle, nb, _ffi.ptr(p.progs), p.prog_off.ctypes.data_as(_ffi._pi32), p.x_off.ctypes.data_as(_ffi._pi64),
            p.n.ctypes.data_as(_ffi._pi32), p.d, _ffi.ptr(p.X), p.X.shape[0], p.vec_off.ctypes.data_as(_ffi._pi64),
            _ffi.ptr(p.noise), _ffi.ptr(p.resid), _ffi.ptr(pp.Xt), a["xt_rows"], keep[0].ctypes.data_as(_ffi._pi64),
            keep32[0].ctypes.data_as(_ffi._pi32), None if a["pred"] is None else _ffi.ptr(a["pred"]),
            None if pred_off is None else pred_off.ctypes.data_as(_ffi._pi32), _ffi.ptr(pc.tdiag),
            keep[1].ctypes.data_as(_ffi._pi64), keep[2].ctypes.data_as(_ffi._pi64), mean.ctypes.data_as(_ffi._pdbl),
            keep[3].ctypes.data_as(_ffi._pi64), cov.ctypes.data_as(_ffi._pdbl), keep32[1].ctypes.data_as(_ffi._pi32),
            None if a["xi"] is None else _ffi.ptr(np.ascontiguousarray(a["xi"])), keep[4].ctypes.data_as(_ffi._pi64),
            None if a["samples"] is None else a["samples"].ctypes.data_as(_ffi._pdbl), info.ctypes.data_as(_ffi._pi32),
            cinfo.ctypes.data_as(_ffi._pi32), out.ctypes.data_as(_ffi._pdbl))
        return rc, _ffi.lib().tgp_last_error().decode()

    pc = small.pack_condition(members, [Q, Q + 1.0], [np.full(m, TAU)] * 2, None, [z, z])
    assert call(pc)[0] == 0
    for over, text in ((dict(m=[m, CAP - n + 1], xt_rows=10**6), f"member 1: data and test points together must be at most {CAP}"),
                       (dict(m=[m, -1]), "member 1: negative number of test points"),
                       (dict(ndraw=[2, -1]), "member 1: negative number of draws"),
                       (dict(tvec_off=[0, -1]), "member 1: negative offset into the test diagonal"),
                       (dict(cov_off=[0, -1]), "member 1: negative offset into the test diagonal"),
                       (dict(xi_off=[-1, 0]), "member 0: negative offset into the test diagonal"),
                       (dict(mean_off=[0, -1]), "member 1: negative offset into the predictions"),
                       (dict(xt_off=[0, 2 * m - 1]), "member 1: test rows"),
                       (dict(xi=None), "member 0: 2 draws are asked for, but xi_host or samples_host is null"),
                       (dict(samples=None), "member 0: 2 draws are asked for"),
                       (dict(pred=np.array([(99, 0, 1.0, 0.0)], dtype=small.KOP_DTYPE), pred_off=[0, 0, 1]), "member 1: prediction program")):
        rc, err = call(pc, **over)
        assert rc == _ffi.E_ARG and text in err, (over, err)
