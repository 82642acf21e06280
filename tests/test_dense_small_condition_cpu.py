"""The host side of the joint posterior of the batched small dense path (``tinygp_amd/solvers/small.py``,
``tgp_small_condition``) without a GPU: the reference's own conditions at every case ``test_gpu_1_small_condition.py``
reads, the agreement of header, prototype and binding, the staging bytes, the routing by n + m, the order in which the
generator is read and every ``ValueError`` that names a data set."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import tinygp_amd
from tinygp_amd import GaussianProcess, _ffi, kernels
from tinygp_amd.solvers import DirectSolver, QuasisepSolver, small

import _dense_np as dn
import _dense_small as ds
import _dense_small_condition as sc

ROOT = Path(__file__).resolve().parent.parent
CAP = ds.CAP


def _member(n, d, b):
    prog, P = small.lower_member(ds.member_kernel(kernels, d, b), dn.train(n, d)[0])
    return prog, P, ds.member_noise(n, d, b), ds.resid(n)


# ---- the reference's own conditions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
def test_reference_conditions_at_every_case(d):
    hi = dict(cond=0.0, cond_star=0.0, mean_diff=0.0, cov_diff=0.0, draw_diff=0.0)
    lo = dict(first_row=np.inf, last_row=np.inf, block=np.inf, first_col=np.inf, last_col=np.inf)
    for case in sc.cases():
        if case[1] != d:
            continue
        ref = sc.reference(*case)  # (a) - (d) are asserted inside
        m = case[3]
        assert ref.mean.shape == (m,) and ref.cov.shape == (m, m) and ref.draws.shape == (sc.SMAX, m)
        assert not ref.cov.flags.writeable and not ref.draws.flags.writeable
        for key in hi:
            hi[key] = max(hi[key], getattr(ref.figures, key))
        for key in lo:
            lo[key] = min(lo[key], getattr(ref.figures, key))
    print(f"d = {d}: worst " + " ".join(f"{k} {v:.3g}" for k, v in hi.items())
          + "; lowest (in bars) " + " ".join(f"{k} {v:.3g}" for k, v in lo.items()))
    assert hi["cond"] <= ds.COND_MAX and hi["cond_star"] <= sc.COND_STAR_MAX
    assert max(hi["mean_diff"], hi["cov_diff"], hi["draw_diff"]) <= sc.LONGDOUBLE_TOL
    assert min(lo.values()) >= sc.WEIGHT_MIN
    # the default jitter: the float64 reference still factors every case, its own distance from long double is kept
    worst_cond, least_eig = 0.0, np.inf
    for n, m in sc.JITTER_SHAPES:
        for b in range(3):
            f = sc.reference(n, d, b, m, True).figures
            worst_cond, least_eig = max(worst_cond, f.cond_star), min(least_eig, f.min_eig)
            assert f.cond <= ds.COND_MAX and f.e64.shape == (sc.SMAX, m) and np.all(np.isfinite(f.e64))
    print(f"d = {d}, default jitter: worst cond(Sigma*) {worst_cond:.3g}, smallest eigenvalue {least_eig:.3g}")
    assert least_eig > 0.0


def test_the_shapes_cover_the_seams_and_the_cap():
    shapes = set(sc.SHAPES)
    assert {(1, 1), (1, 3), (2, 2), (3, 1), (63, 65), (64, 64), (65, 63), (64, 128), (128, 64), (127, 65), (129, 63),
            (96, 96), (1, 191), (191, 1), (189, 3), (3, 189)} <= shapes
    assert all((n, m) in shapes for n in (15, 16, 17, 63, 64, 65, 127, 128, 129) for m in (1, 3))
    assert all((n, m) in shapes for n in (1, 3) for m in (63, 64, 65, 127, 128, 129))
    assert any(n + m == CAP - 1 for n, m in shapes) and max(n + m for n, m in shapes) == CAP
    Q = sc.test_points(65, 3, 7)
    X = dn.train(65, 3)[0]
    assert Q.shape == (7, 3) and np.allclose(Q[5], X[0] + 0.01, rtol=0, atol=1e-15)
    assert np.array_equal(sc.test_points(65, 3, 2), dn.query_points(2, 3)[0])


# ---- header, prototype, binding -----------------------------------------------------------------------------------------
def test_header_prototype_and_binding_agree():
    text = (ROOT / "include" / "tgp_hip.h").read_text()
    assert int(re.search(r"#define\s+TGP_ABI_VERSION\s+(\d+)", text).group(1)) == _ffi.ABI_VERSION == 6
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"int\s+tgp_small_condition\s*\((.*?)\)\s*;", plain, flags=re.S)
    args = [" ".join(a.split()) for a in proto.group(1).split(",")]
    ctype = {"tgp_ctx*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "const tgp_kop*": C.c_void_p,
             "const int32_t*": _ffi._pi32, "const int64_t*": _ffi._pi64, "const double*": C.c_void_p,
             "int32_t*": _ffi._pi32, "double*": _ffi._pdbl}
    want = [ctype[a.rsplit(" ", 1)[0]] for a in args]
    names = [a.rsplit(" ", 1)[1] for a in args]
    # the arguments of tgp_small_predict up to pred_prog_off, then the conditioning's, then the outputs
    pred = re.search(r"int\s+tgp_small_predict\s*\((.*?)\)\s*;", plain, flags=re.S)
    pred_names = [" ".join(a.split()).rsplit(" ", 1)[1] for a in pred.group(1).split(",")]
    assert names[:18] == pred_names[:18] and names[17] == "pred_prog_off"
    assert names[18:] == ["test_diag_host", "tvec_off", "mean_off", "mean_host", "cov_off", "cov_host", "ndraw", "xi_host",
                          "xi_off", "samples_host", "info_host", "cond_info_host", "out_host"]
    assert _ffi.SIGNATURES["tgp_small_condition"] == want
    lib = _ffi.load_library()  # needs no GPU
    assert lib.tgp_small_condition.argtypes == want and lib.tgp_abi_version() == 6
    null = [None, 1] + [None] * 4 + [1, None, 0] + [None] * 4 + [0] + [None] * 17
    assert len(null) == len(want) and lib.tgp_small_condition(*null) == _ffi.E_ARG
    assert b"null context" in lib.tgp_last_error()


# ---- staging bytes ----------------------------------------------------------------------------------------------------------
def test_launch_bytes_count_rows_programs_points_and_outputs():
    d, n = 3, 17
    members = [_member(n, d, b) for b in range(2)]
    other = ds.member_kernel(kernels, d, 0, other=True).program()

    def bytes_of(ms, Ss=(0, 0), second=None, cov=True):
        tests = [np.asarray(dn.query_points(m, d)[0]) if m else np.empty((0, d)) for m in ms]
        pc = small.pack_condition(members, tests, [np.full(m, 0.1) for m in ms], second,
                                  [np.zeros((s, m)) for s, m in zip(Ss, ms)])
        return small.condition_launch_bytes(pc, cov)

    base = bytes_of([0, 0])
    # two table rows of 80 bytes, two programs, ONE copy of the points, two noise and residual vectors, two values,
    # info and cond_info
    assert base == 2 * 80 + 2 * _ffi.KPROG_BYTES + (n * d + 2 * 2 * n) * 8 + 2 * 8 + 2 * 8
    # 5 test points: their coordinates, test diagonal, means and the 25 covariances
    assert bytes_of([5, 0]) - base == 5 * d * 8 + 2 * 5 * 8 + 25 * 8
    assert bytes_of([5, 0], cov=False) - base == 5 * d * 8 + 2 * 5 * 8
    # 3 draws of them: normals and samples
    assert bytes_of([5, 0], (3, 0)) - bytes_of([5, 0]) == 2 * 3 * 5 * 8
    assert bytes_of([5, 0], (3, 7)) == bytes_of([5, 0], (3, 0))  # draws of no points take nothing
    assert bytes_of([0, 0], second=[None, other]) - base == _ffi.KPROG_BYTES
    # B = 1024 members at (n, m) = (64, 128) with covariances and 16 draws stay under the staging cap of one launch
    per_member = 80 + _ffi.KPROG_BYTES + (64 * 16 + 2 * 64 + 128 * 16 + 2 * 128 + 128 * 128 + 2 * 16 * 128) * 8 + 16
    assert 1024 * per_member < small.STAGE_BYTES == 1 << 30


def test_packing_of_test_diagonals_normals_and_offsets():
    d = 3
    members = [_member(n, d, b) for b, n in enumerate((9, 17, 5))]
    tests = [np.asarray(dn.query_points(4, d)[0]), np.empty((0, d)), np.asarray(dn.query_points(7, d)[0])]
    taus = [np.full(4, 0.1), np.empty(0), np.linspace(0.1, 0.2, 7)]
    zs = [np.arange(8.0).reshape(2, 4), None, np.arange(21.0).reshape(3, 7)]
    pc = small.pack_condition(members, tests, taus, None, zs)
    assert pc.pp.m.tolist() == [4, 0, 7] and pc.pp.out_off.tolist() == [0, 4, 4]
    assert pc.cov_off.dtype == np.int64 and pc.cov_off.tolist() == [0, 16, 16]
    assert pc.ndraw.dtype == np.int32 and pc.ndraw.tolist() == [2, 0, 3]
    assert pc.xi_off.dtype == np.int64 and pc.xi_off.tolist() == [0, 8, 8] and pc.xi.shape == (29,)
    assert np.array_equal(pc.xi[8:], np.arange(21.0)) and np.array_equal(pc.tdiag[4:], taus[2])
    with pytest.raises(ValueError, match=r"member 2: its test diagonal must have shape \(7,\); got \(4,\)"):
        small.pack_condition(members, tests, [taus[0], taus[1], taus[0]])
    with pytest.raises(ValueError, match=r"data set 9: its normals must have shape \(S, 4\); got \(2, 5\)"):
        small.pack_condition(members, tests, taus, None, [np.zeros((2, 5)), None, None],
                             labels=["data set 9", "data set 1", "data set 2"])
    big = [_member(CAP - 3, d, 0)]
    with pytest.raises(ValueError, match=rf"member 0: .*at most {CAP} data and test points per member \(got {CAP - 3} \+ 4\)"):
        small.pack_condition(big, tests[:1], taus[:1])


# ---- the route --------------------------------------------------------------------------------------------------------------
class _FakeLib:
    """Stands where the loaded library would: records the members of every ``tgp_small_condition`` call."""

    def __init__(self):
        self.calls = []

    def tgp_small_condition(self, handle, nb, progs, prog_off, x_off, n, d, X, x_rows, vec_off, noise, resid, Xt, xt_rows,
                            xt_off, m, pred_progs, pred_prog_off, tdiag, tvec_off, mean_off, mean, cov_off, cov, ndraw,
                            xi, xi_off, samples, info, cond_info, out):
        self.calls.append(dict(nb=nb, n=[n[b] for b in range(nb)], m=[m[b] for b in range(nb)],
                               S=[ndraw[b] for b in range(nb)], cov=bool(cov), samples=bool(samples)))
        for b in range(nb):
            out[b] = -1.0 - b
        return 0


def test_routing_by_n_plus_m_at_the_cap(monkeypatch):
    fake, singles = _FakeLib(), []
    monkeypatch.setattr(_ffi, "lib", lambda: fake)
    monkeypatch.setattr(_ffi, "default_ctx", lambda: type("Ctx", (), {"handle": None})())

    def single(kernel, X, y, diag, mean, X_test, test_diag, predict_kernel, xi, ctx):
        m = len(test_diag)
        singles.append((len(y), m))
        return -99.0, 0, 0, np.zeros(m), np.zeros((m, m)), None if xi is None else np.zeros((len(xi), m))

    monkeypatch.setattr(small, "_single_condition", single)
    d, k = 3, ds.member_kernel(kernels, 3, 0)
    ns, ms = (CAP - 4, CAP - 4, CAP, 5), (4, 5, 1, 0)
    Xs, ys = [dn.train(n, d)[0] for n in ns], [ds.resid(n) for n in ns]
    Qs = [dn.query_points(m, d)[0] if m else np.empty((0, d)) for m in ms]
    values, mu, cov = tinygp_amd.condition_datasets(k, Xs, ys, Qs, diags=[0.1] * 4)
    assert fake.calls == [dict(nb=2, n=[CAP - 4, 5], m=[4, 0], S=[0, 0], cov=True, samples=False)]
    assert singles == [(CAP - 4, 5), (CAP, 1)] and values.tolist() == [-1.0, -99.0, -99.0, -2.0]
    assert [c.shape for c in cov] == [(4, 4), (5, 5), (1, 1), (0, 0)]
    fake.calls.clear(), singles.clear()
    values, f = tinygp_amd.sample_conditional_datasets(k, Xs, ys, Qs, key=1, shape=(2,), diags=[0.1] * 4)
    assert fake.calls == [dict(nb=2, n=[CAP - 4, 5], m=[4, 0], S=[2, 2], cov=False, samples=True)]
    assert singles == [(CAP - 4, 5), (CAP, 1)] and [s.shape for s in f] == [(2, 4), (2, 5), (2, 1), (2, 0)]
    low = small.lower_member(k, Xs[0])
    assert small.condition_route(CAP - 4, 4, low) and not small.condition_route(CAP - 4, 5, low)
    assert small.condition_route(CAP, 0, low) and not small.condition_route(CAP + 1, 0, low)
    assert not small.condition_route(5, 3, None)


def test_the_generator_is_read_in_member_order(monkeypatch):
    seen = []

    def core(kernels_, Xs, ys, X_tests, diags, means, test_means, test_diags, predict_kernels, include_mean, xis,
             want_cov, ctx):
        ms = [len(q) for q in X_tests]
        draws = [np.asarray(xis(b, m)) for b, m in enumerate(ms)]
        seen.extend(draws)
        assert want_cov is False
        return np.zeros(len(ms)), np.zeros(len(ms), np.int32), np.zeros(len(ms), np.int32), None, None, draws

    monkeypatch.setattr(small, "_condition_sets", core)
    Qs = [np.zeros(4), np.zeros(0), np.zeros(7)]
    _, f = small.sample_conditional_datasets(None, [None] * 3, [None] * 3, Qs, key=11, shape=(2, 3), diags=None)
    rng = np.random.default_rng(11)
    for got, m in zip(seen, (4, 0, 7)):
        assert np.array_equal(got, rng.standard_normal((6, m)))
    assert [s.shape for s in f] == [(2, 3, 4), (2, 3, 0), (2, 3, 7)]
    # a Generator is used as it is and moves on; xi= replaces the draw
    gen = np.random.default_rng(11)
    small.sample_conditional_datasets(None, [None] * 3, [None] * 3, Qs, key=gen, diags=None)
    assert np.array_equal(gen.standard_normal(2), np.random.default_rng(11).standard_normal(13)[11:])
    xi = [np.ones((6, 4)), np.ones((6, 0)), np.ones((6, 7))]
    _, f = small.sample_conditional_datasets(None, [None] * 3, [None] * 3, Qs, key=None, shape=(6,), xi=xi, diags=None)
    assert all(np.array_equal(a, b) for a, b in zip(f, xi))
    with pytest.raises(ValueError, match=r"xi\[2\] must have shape \(6, 7\) for data set 2.*got \(5, 7\)"):
        small.sample_conditional_datasets(None, [None] * 3, [None] * 3, Qs, key=None, shape=(6,),
                                          xi=xi[:2] + [np.ones((5, 7))], diags=None)


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_data_set_errors_name_the_data_set():
    k = kernels.Matern32(1.5)
    Xs = [dn.train(5, 3)[0], dn.train(7, 3)[0]]
    ys = [ds.resid(5), ds.resid(7)]
    Qs = [dn.query_points(4, 3)[0], dn.query_points(3, 3)[0]]
    for call, extra in ((tinygp_amd.condition_datasets, {}), (tinygp_amd.sample_conditional_datasets, dict(key=1))):
        with pytest.raises(ValueError, match=r"X_tests must hold one entry per data set \(2\); got 1"):
            call(k, Xs, ys, Qs[:1], diags=[0.1, 0.1], **extra)
        with pytest.raises(ValueError, match=r"test_diags must hold one entry per data set \(2\); got 3"):
            call(k, Xs, ys, Qs, diags=[0.1, 0.1], test_diags=[0.1] * 3, **extra)
        with pytest.raises(ValueError, match=r"test_diags\[1\] must have shape \(3,\) or be a scalar for data set 1; got \(4,\)"):
            call(k, Xs, ys, Qs, diags=[0.1, 0.1], test_diags=[0.1, np.zeros(4)], **extra)
        with pytest.raises(ValueError, match=r"means\[1\] of data set 1 is a vector: .*test_means\[1\] \(a scalar or \(3,\)\)"):
            call(k, Xs, ys, Qs, diags=[0.1, 0.1], means=[0.5, np.zeros(7)], **extra)
        with pytest.raises(ValueError, match=r"test_means\[0\] is given, but means\[0\] of data set 0 is not a vector"):
            call(k, Xs, ys, Qs, diags=[0.1, 0.1], means=[0.5, None], test_means=[0.5, None], **extra)
        with pytest.raises(ValueError, match=r"ys\[1\] must have shape \(7,\) for data set 1; got \(5,\)"):
            call(k, Xs, [ys[0], ys[0]], Qs, diags=[0.1, 0.1], **extra)


def test_public_entry_points_exist():
    assert tinygp_amd.condition_datasets is small.condition_datasets
    assert tinygp_amd.sample_conditional_datasets is small.sample_conditional_datasets
    assert callable(DirectSolver.condition_batch) and not hasattr(QuasisepSolver, "condition_batch")
    assert callable(GaussianProcess.condition_batch) and callable(GaussianProcess.sample_conditional_batch)
    assert "TGP_SMALL_MAX_N" in small.condition_datasets.__doc__
    assert small.jitter(np.float64) == sc.JITTER


def test_host_draws_are_loc_plus_l_xi_and_report_the_failed_minor():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((5, 5))
    cov, loc, xi = A @ A.T + np.eye(5), rng.standard_normal(5), rng.standard_normal((4, 5))
    f, bad = small.host_draws(loc, cov, xi)
    assert bad == 0 and np.allclose(f, loc + xi @ np.linalg.cholesky(cov).T, rtol=1e-13, atol=1e-13)
    cov[2, 2] = -1.0
    f, bad = small.host_draws(loc, cov, xi)
    assert bad == 3 and f.shape == (4, 5) and np.all(np.isnan(f))
    assert small.host_draws(np.zeros(0), np.zeros((0, 0)), np.zeros((4, 0)))[0].shape == (4, 0)
