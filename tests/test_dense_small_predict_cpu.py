"""The host side of the predictions of the batched small dense path (``tinygp_amd/solvers/small.py``,
``tgp_small_predict``) without a GPU: the reference's own conditions at every case ``test_gpu_1_small_predict.py`` reads,
the agreement of header, prototype and binding, the packing of test points, second programs, chunk rows and staging
bytes, the routing rules and every ``ValueError`` that names a data set."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import tinygp_amd
from tinygp_amd import GaussianProcess, _ffi, kernels, transforms
from tinygp_amd.kernels import quasisep
from tinygp_amd.solvers import DirectSolver, QuasisepSolver, small

import _dense_np as dn
import _dense_small as ds
import _dense_small_predict as sp

ROOT = Path(__file__).resolve().parent.parent
CHUNK = small.PRED_CHUNK


def _member(n, d, b, kernel=None):
    X = dn.train(n, d)[0]
    prog, P = small.lower_member(ds.member_kernel(kernels, d, b) if kernel is None else kernel, X)
    return prog, P, ds.member_noise(n, d, b), ds.resid(n)


# ---- the reference's own conditions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
def test_reference_conditions_at_every_case(d):
    hi = dict(cond=0.0, mean_diff=0.0, var_diff=0.0)
    lo = dict(first_row=np.inf, last_row=np.inf, block=np.inf, first_term=np.inf, last_term=np.inf, min_var=np.inf)
    for case in sp.cases():
        if case[1] != d:
            continue
        ref = sp.reference(*case)  # (a) - (d) are asserted inside
        assert ref.mean.shape == ref.var.shape == (case[3] + 2,) and not ref.mean.flags.writeable
        for key in hi:
            hi[key] = max(hi[key], getattr(ref.figures, key))
        for key in lo:
            lo[key] = min(lo[key], getattr(ref.figures, key))
    print(f"d = {d}: worst " + " ".join(f"{k} {v:.3g}" for k, v in hi.items())
          + "; lowest (in bars) " + " ".join(f"{k} {v:.3g}" for k, v in lo.items()))
    assert hi["cond"] <= ds.COND_MAX and max(hi["mean_diff"], hi["var_diff"]) <= sp.LONGDOUBLE_TOL
    assert min(lo[k] for k in ("first_row", "last_row", "block", "first_term", "last_term")) >= sp.WEIGHT_MIN
    assert lo["min_var"] > 0.0  # every variance is a positive share of k**
    # a prediction kernel of its own: (a), (b) and (d) hold there too
    for n in (17, 65, ds.CAP):
        f = sp.reference(n, d, 0, 5, True).figures
        assert f.cond <= ds.COND_MAX and min(f.first_term, f.last_term) >= sp.WEIGHT_MIN


def test_the_added_test_points_sit_beside_the_first_and_last_data_point():
    for d in ds.DS:
        X, Q = dn.train(65, d)[0], sp.query(65, d, 5)
        assert Q.shape == (7,) + X.shape[1:] and not Q.flags.writeable
        assert np.array_equal(Q[:5], dn.query_points(5, d)[0])
        assert np.allclose(Q[5], X[0] + 0.01, rtol=0, atol=1e-15) and np.allclose(Q[6], X[-1] + 0.01, rtol=0, atol=1e-15)


# ---- header, prototype, binding -----------------------------------------------------------------------------------------
def test_header_prototype_and_binding_agree():
    text = (ROOT / "include" / "tgp_hip.h").read_text()
    assert int(re.search(r"#define\s+TGP_SMALL_PRED_CHUNK\s+(\d+)", text).group(1)) == _ffi.SMALL_PRED_CHUNK == CHUNK
    assert int(re.search(r"#define\s+TGP_ABI_VERSION\s+(\d+)", text).group(1)) == _ffi.ABI_VERSION == 6
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"int\s+tgp_small_predict\s*\((.*?)\)\s*;", plain, flags=re.S)
    args = [" ".join(a.split()) for a in proto.group(1).split(",")]
    ctype = {"tgp_ctx*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "const tgp_kop*": C.c_void_p,
             "const int32_t*": _ffi._pi32, "const int64_t*": _ffi._pi64, "const double*": C.c_void_p,
             "int32_t*": _ffi._pi32, "double*": _ffi._pdbl}
    want = [ctype[a.rsplit(" ", 1)[0]] for a in args]
    names = [a.rsplit(" ", 1)[1] for a in args]
    # the arguments of tgp_small_logprob up to the residual, then the prediction's, then the outputs
    value = re.search(r"int\s+tgp_small_logprob\s*\((.*?)\)\s*;", plain, flags=re.S)
    value_names = [" ".join(a.split()).rsplit(" ", 1)[1] for a in value.group(1).split(",")]
    assert names[:12] == value_names[:12]
    assert names[12:] == ["Xt_host", "xt_rows", "xt_off", "m", "pred_progs", "pred_prog_off", "out_off", "info_host",
                          "out_host", "mean_host", "var_host"]
    assert _ffi.SIGNATURES["tgp_small_predict"] == want
    lib = _ffi.load_library()  # needs no GPU
    assert lib.tgp_small_predict.argtypes == want and lib.tgp_abi_version() == 6
    assert lib.tgp_small_predict(*([None, 1] + [None] * 4 + [1, None, 0] + [None] * 4 + [0] + [None] * 9)) == _ffi.E_ARG
    assert b"null context" in lib.tgp_last_error()
    assert _ffi.KPROG_BYTES == 8 * -(-(4 + 2 * 4 * 32) // 8) + 2 * 8 * 32


# ---- packing ----------------------------------------------------------------------------------------------------------
def test_test_points_offsets_and_second_programs_are_stacked_member_by_member():
    d = 3
    members = [_member(n, d, b) for b, n in enumerate((9, 17, 5))]
    tests = [np.asarray(dn.query_points(m, d)[0]) for m in (4, 0, 7)]
    other = ds.member_kernel(kernels, d, 1, other=True).program()
    pp = small.pack_predict(members, [tests[0], np.empty((0, d)), tests[2]], [None, other, None])
    assert pp.packed.n.tolist() == [9, 17, 5] and pp.packed.vec_off.tolist() == [0, 9, 26]
    assert pp.m.dtype == np.int32 and pp.m.tolist() == [4, 0, 7]
    assert pp.xt_off.dtype == np.int64 and pp.xt_off.tolist() == [0, 4, 4]
    assert pp.out_off.dtype == np.int64 and pp.out_off.tolist() == [0, 4, 4]
    assert pp.Xt.shape == (11, d) and pp.Xt.dtype == np.float64 and pp.Xt.flags.c_contiguous
    assert np.array_equal(pp.Xt[:4], tests[0]) and np.array_equal(pp.Xt[4:], tests[2])
    assert pp.pred_prog_off.dtype == np.int32 and pp.pred_prog_off.tolist() == [0, 0, len(other), len(other)]
    assert pp.pred_progs.dtype == small.KOP_DTYPE
    assert [tuple(op) for op in pp.pred_progs.tolist()] == [(int(a), int(m), float(x), float(y)) for a, m, x, y in other]
    # nobody names a second program: the call gets NULL
    none = small.pack_predict(members, tests)
    assert none.pred_progs is None and none.pred_prog_off is None
    # nobody has test points: an empty (0, d) array, still contiguous
    empty = small.pack_predict(members, [np.empty((0, d))] * 3)
    assert empty.Xt.shape == (0, d) and empty.m.tolist() == [0, 0, 0] and empty.out_off.tolist() == [0, 0, 0]


def test_shared_test_points_are_uploaded_once():
    d, n, m = 3, 9, 40
    members = [_member(n, d, b) for b in range(4)]
    grid = np.asarray(dn.query_points(m, d)[0])
    mine = np.asarray(dn.query_points(m + 1, d)[0])
    pp = small.pack_predict(members, [grid, grid, mine, np.array(grid)])
    assert pp.xt_off.tolist() == [0, 0, m, 0] and pp.Xt.shape == (2 * m + 1, d)
    assert pp.out_off.tolist() == [0, m, 2 * m, 3 * m + 1]  # the outputs are every member's own
    assert pp.packed.x_off.tolist() == [0, 0, 0, 0] and pp.packed.X.shape == (n, d)
    shared = small.predict_launch_bytes(pp)
    apart = small.predict_launch_bytes(small.pack_predict(members, [grid, grid + 1.0, mine, grid + 2.0]))
    assert apart - shared == 2 * m * d * 8


def test_chunk_rows_of_a_member_with_more_test_points_than_a_chunk():
    assert small.predict_rows(0) == [(0, 0)] and small.predict_rows(1) == [(0, 1)]
    assert small.predict_rows(CHUNK) == [(0, CHUNK)] and small.predict_rows(CHUNK + 1) == [(0, CHUNK), (CHUNK, 1)]
    assert small.predict_rows(2 * CHUNK + 1) == [(0, CHUNK), (CHUNK, CHUNK), (2 * CHUNK, 1)]
    for m in (CHUNK - 1, 3 * CHUNK, 3 * CHUNK + 7):
        rows = small.predict_rows(m)
        assert sum(c for _, c in rows) == m and all(1 <= c <= CHUNK for _, c in rows)
        assert [at for at, _ in rows] == list(range(0, m, CHUNK))
    assert small.predict_rows(10, chunk=4) == [(0, 4), (4, 4), (8, 2)]


def test_launch_bytes_count_rows_programs_points_and_outputs():
    d, n = 3, 17
    members = [_member(n, d, b) for b in range(2)]
    other = ds.member_kernel(kernels, d, 0, other=True).program()

    def bytes_of(ms, second=None, var=True):
        tests = [np.asarray(dn.query_points(m, d)[0]) if m else np.empty((0, d)) for m in ms]
        return small.predict_launch_bytes(small.pack_predict(members, tests, second), var)

    base = bytes_of([0, 0])
    # two table rows, two programs, ONE copy of the points, two noise and residual vectors, two values, info
    assert base == 2 * 64 + 2 * _ffi.KPROG_BYTES + (n * d + 2 * 2 * n) * 8 + 2 * 8 + 8
    assert bytes_of([5, 0]) - base == 5 * d * 8 + 5 * 16
    assert bytes_of([5, 0], var=False) - base == 5 * d * 8 + 5 * 8
    assert bytes_of([0, 0], [None, other]) - base == _ffi.KPROG_BYTES
    m = 2 * CHUNK + 1  # two more table rows; the points and the outputs are counted once
    assert bytes_of([m, 0]) - base == 2 * 64 + m * d * 8 + m * 16
    # B = 1024 members at the cap with 1024 test points each stay under the staging cap of one launch
    per_member = (64 * 4 + _ffi.KPROG_BYTES + (ds.CAP * 16 + 2 * ds.CAP + 1024 * 16) * 8 + 16 + 1024 * 16)
    assert 1024 * per_member < small.STAGE_BYTES == 1 << 30


def test_packing_errors_name_the_member():
    good = _member(8, 3, 0)
    Q = np.asarray(dn.query_points(4, 3)[0])
    with pytest.raises(ValueError, match=r"tests must hold one entry per member \(2\); got 1"):
        small.pack_predict([good, good], [Q])
    with pytest.raises(ValueError, match=r"member 1: its test points must have shape \(m, 3\) like its points; got \(4,\)"):
        small.pack_predict([good, good], [Q, Q[:, 0]])
    with pytest.raises(ValueError, match=r"data set 7: its test points must have shape \(m, 3\)"):
        small.pack_predict([good, good], [Q, Q[:, :2]], labels=["data set 3", "data set 7"])
    with pytest.raises(ValueError, match=r"member 1: .*1 \.\. 32 operations \(got 33\)"):
        small.pack_predict([good, good], [Q, Q], [None, [good[0][0]] * 33])
    with pytest.raises(ValueError, match=r"pred_progs must hold one entry per member \(2\); got 1"):
        small.pack_predict([good, good], [Q, Q], [good[0]])


# ---- the route --------------------------------------------------------------------------------------------------------
def test_route_of_the_test_points_and_the_prediction_kernel():
    X3, Q3 = dn.train(6, 3)[0], dn.query_points(4, 3)[0]
    k = kernels.Exp(1.1) + kernels.Matern32(1.3)
    low = small.lower_member(k, X3)
    Pt, second = small.lower_test(k, None, X3, Q3, low)
    assert np.array_equal(Pt, Q3) and Pt.dtype == np.float64 and second is None
    Pt, second = small.lower_test(k, None, X3, None, low)  # the member's own points, sent as test points
    assert np.array_equal(Pt, low[1]) and second is None
    # one addend as the prediction kernel: its program rides along
    Pt, second = small.lower_test(k, kernels.Matern32(1.3), X3, Q3, low)
    assert np.array_equal(Pt, Q3) and second == kernels.Matern32(1.3).program()
    # the model under an input transform: the test points go through it too
    scaled = transforms.Linear(0.5, k)
    low_s = small.lower_member(scaled, X3)
    Pt, second = small.lower_test(scaled, None, X3, Q3, low_s)
    assert np.array_equal(Pt, 0.5 * Q3)
    # a prediction kernel under ANOTHER transform than the model's lowers the data points differently: single path
    assert small.lower_test(scaled, kernels.Matern32(1.3), X3, Q3, low_s) is None
    assert small.lower_test(k, transforms.Linear(0.5, kernels.Matern32(1.3)), X3, Q3, low) is None
    assert small.lower_test(scaled, transforms.Linear(0.5, kernels.Matern32(1.3)), X3, Q3, low_s) is not None
    # a prediction kernel without a device program, pytree test points, test points of another dimension
    custom = kernels.Custom(lambda a, b: np.exp(-np.sum(np.square(a - b))))
    assert small.lower_test(k, custom, X3, Q3, low) is None
    assert small.lower_test(k, None, X3, {"a": Q3}, low) is None
    assert small.lower_test(k, None, X3, dn.query_points(4, 1)[0], low) is None
    # length and lowerability decide as for the value
    assert small.batched_route(ds.CAP, low) and not small.batched_route(ds.CAP + 1, low)


def test_data_set_errors_name_the_data_set():
    k = kernels.Matern32(1.5)
    Xs = [dn.train(5, 3)[0], dn.train(7, 3)[0]]
    ys = [ds.resid(5), ds.resid(7)]
    Qs = [dn.query_points(4, 3)[0], dn.query_points(3, 3)[0]]
    predict = tinygp_amd.predict_datasets
    with pytest.raises(ValueError, match=r"X_tests must hold one entry per data set \(2\); got 1"):
        predict(k, Xs, ys, Qs[:1], diags=[0.1, 0.1])
    with pytest.raises(ValueError, match=r"test_means must hold one entry per data set \(2\); got 3"):
        predict(k, Xs, ys, Qs, diags=[0.1, 0.1], test_means=[None] * 3)
    with pytest.raises(ValueError, match=r"predict_kernels must hold one entry per data set \(2\); got 1"):
        predict(k, Xs, ys, Qs, diags=[0.1, 0.1], predict_kernels=[k])
    with pytest.raises(ValueError, match=r"means\[1\] of data set 1 is a vector: .*test_means\[1\] \(a scalar or \(3,\)\)"):
        predict(k, Xs, ys, Qs, diags=[0.1, 0.1], means=[0.5, np.zeros(7)])
    with pytest.raises(ValueError, match=r"test_means\[1\] must have shape \(3,\) or be a scalar for data set 1; got \(4,\)"):
        predict(k, Xs, ys, Qs, diags=[0.1, 0.1], means=[None, np.zeros(7)], test_means=[None, np.zeros(4)])
    with pytest.raises(ValueError, match=r"test_means\[0\] is given, but means\[0\] of data set 0 is not a vector"):
        predict(k, Xs, ys, Qs, diags=[0.1, 0.1], means=[0.5, None], test_means=[0.5, None])
    with pytest.raises(ValueError, match=r"ys\[1\] must have shape \(7,\) for data set 1; got \(5,\)"):
        predict(k, Xs, [ys[0], ys[0]], Qs, diags=[0.1, 0.1])
    with pytest.raises(NotImplementedError, match="QuasisepSolver"):
        predict(quasisep.Matern32(1.0), [np.arange(4.0)], [np.zeros(4)], [np.arange(3.0)], diags=[0.1])
    with pytest.raises(NotImplementedError, match="QuasisepSolver"):
        predict(kernels.Matern32(1.0), [np.arange(4.0)], [np.zeros(4)], [np.arange(3.0)], diags=[0.1],
                predict_kernels=[quasisep.Matern32(1.0)])


def test_public_entry_points_exist():
    assert tinygp_amd.predict_datasets is small.predict_datasets
    assert callable(DirectSolver.predict_batch) and callable(GaussianProcess.predict_batch)
    assert not hasattr(QuasisepSolver, "predict_batch")
    doc = GaussianProcess.predict_batch.__doc__
    assert "posterior bar" in doc and "DirectSolver" in doc and "predict_datasets" in doc
    assert "TGP_SMALL_PRED_CHUNK" in small.predict_datasets.__doc__
