"""The host side of the batched small dense path (``tinygp_amd/solvers/small.py``, ``tgp_small_logprob``) without a GPU:
the packing of programs, offsets and shared coordinates, every validation error with its member or data set named, the
choice between the batched launches and the single path, the agreement of header, prototype and binding, and the
reference's own conditions at every shape ``test_gpu_1_small_batch.py`` uses."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import tinygp_amd
from tinygp_amd import _ffi, kernels, transforms
from tinygp_amd.kernels import quasisep
from tinygp_amd.solvers import small

import _dense_np as dn
import _dense_small as ds

ROOT = Path(__file__).resolve().parent.parent


def _member(n, d, b, kernel=None):
    X = dn.train(n, d)[0]
    prog, P = small.lower_member(ds.member_kernel(kernels, d, b) if kernel is None else kernel, X)
    return prog, P, ds.member_noise(n, d, b), ds.resid(n)


# ---- packing ----------------------------------------------------------------------------------------------------------
def test_programs_and_offsets_are_stacked_member_by_member():
    ks = [kernels.Matern32(1.5), 1.3 * kernels.ExpSquared(1.5), kernels.Exp(1.0) + kernels.Matern52(2.0) * kernels.Cosine(3.0)]
    members = [_member(17, 1, b, k) for b, k in enumerate(ks)]
    p = small.pack_members(members)
    assert p.progs.dtype == small.KOP_DTYPE and p.progs.dtype.itemsize == C.sizeof(_ffi.KOp) == 24
    for field, (ctype_name, _) in zip(p.progs.dtype.names, _ffi.KOp._fields_):
        assert field == ctype_name and p.progs.dtype.fields[field][1] == getattr(_ffi.KOp, field).offset
    assert p.prog_off.dtype == np.int32 and p.prog_off.tolist() == [0, 1, 4, 9]
    for b, k in enumerate(ks):
        got = [tuple(op) for op in p.progs[p.prog_off[b]:p.prog_off[b + 1]].tolist()]
        assert got == [(int(a), int(m), float(x), float(y)) for a, m, x, y in k.program()]
    assert p.n.dtype == np.int32 and p.n.tolist() == [17, 17, 17]
    assert p.vec_off.dtype == np.int64 and p.vec_off.tolist() == [0, 17, 34]
    for b in range(3):
        assert np.array_equal(p.noise[17 * b:17 * (b + 1)], ds.member_noise(17, 1, b))
        assert np.array_equal(p.resid[17 * b:17 * (b + 1)], ds.resid(17))
    assert p.d == 1 and p.X.dtype == p.noise.dtype == p.resid.dtype == np.float64 and p.X.flags.c_contiguous


def test_members_on_member_zeros_points_share_one_copy():
    n, d = 9, 3
    X = dn.train(n, d)[0]
    plain = [_member(n, d, b) for b in range(3)]
    p = small.pack_members(plain)
    assert p.x_off.dtype == np.int64 and p.x_off.tolist() == [0, 0, 0] and p.X.shape == (n, d)
    assert np.array_equal(p.X, X)
    # a per-member input scale ships its own coordinates; a scale of one folds back onto member 0's
    scaled = [transforms.Linear(s, ds.member_kernel(kernels, d, 0)) for s in (1.0, 0.5, 1.0, 2.0)]
    members = [small.lower_member(k, X) + (ds.member_noise(n, d, 0), ds.resid(n)) for k in scaled]
    p = small.pack_members(members)
    assert p.x_off.tolist() == [0, n, 0, 2 * n] and p.X.shape == (3 * n, d)
    assert np.array_equal(p.X[n:2 * n], 0.5 * X) and np.array_equal(p.X[2 * n:], 2.0 * X)
    # an equal copy of the array is still "the same points"; another length never is
    ragged = [_member(n, d, 0), (plain[1][0], np.array(X), plain[1][2], plain[1][3]), _member(5, d, 0)]
    p = small.pack_members(ragged)
    assert p.x_off.tolist() == [0, 0, n] and p.n.tolist() == [n, n, 5] and p.vec_off.tolist() == [0, n, 2 * n]


def test_one_dimensional_points_become_a_column():
    prog, P = small.lower_member(kernels.Exp(1.0), np.linspace(0.0, 1.0, 4, dtype=np.float32))
    assert P.shape == (4, 1) and P.dtype == np.float64 and prog == kernels.Exp(1.0).program()


# ---- validation -------------------------------------------------------------------------------------------------------
def test_packing_errors_name_the_member():
    good = _member(8, 1, 0)
    with pytest.raises(ValueError, match="at least one member"):
        small.pack_members([])
    with pytest.raises(ValueError, match=r"member 1: .*shape \(n, 1\)"):
        small.pack_members([good, _member(8, 3, 0)])
    prog, P, noise, resid = _member(ds.CAP, 1, 0)
    big = np.concatenate([P, P[:1] + 5.0])
    with pytest.raises(ValueError, match=rf"member 1: .*1 \.\. {ds.CAP} points .*got {ds.CAP + 1}"):
        small.pack_members([good, (prog, big, np.ones(ds.CAP + 1), np.ones(ds.CAP + 1))])
    with pytest.raises(ValueError, match=r"member 2: noise and resid must have shape \(8,\)"):
        small.pack_members([good, good, (good[0], good[1], good[2][:7], good[3])])
    with pytest.raises(ValueError, match=r"member 1: .*1 \.\. 32 operations \(got 33\)"):
        small.pack_members([good, ([good[0][0]] * 33, good[1], good[2], good[3])])
    with pytest.raises(ValueError, match=r"data set 7: .*1 \.\. 32 operations"):
        small.pack_members([good, ([good[0][0]] * 33, good[1], good[2], good[3])], labels=["data set 3", "data set 7"])


def test_data_set_errors_name_the_data_set():
    k = kernels.Matern32(1.5)
    Xs = [dn.train(5, 3)[0], dn.train(7, 3)[0]]
    ys = [ds.resid(5), ds.resid(7)]
    check = small.check_datasets
    members = check(k, Xs, ys, [0.1, np.full(7, 0.2)], [None, 0.5])
    assert [m[0] for m in members] == [k, k] and members[0][4] is None
    assert np.array_equal(members[0][3], np.full(5, 0.1)) and np.array_equal(members[1][4], np.full(7, 0.5))
    with pytest.raises(ValueError, match="at least one data set"):
        check(k, [], [], [])
    with pytest.raises(ValueError, match=r"kernels must be one kernel or one per data set \(2\); got 3"):
        check([k, k, k], Xs, ys, [0.1, 0.1])
    with pytest.raises(ValueError, match=r"ys must hold one entry per data set \(2\); got 1"):
        check(k, Xs, ys[:1], [0.1, 0.1])
    with pytest.raises(ValueError, match=r"diags must hold one entry per data set \(2\); got 3"):
        check(k, Xs, ys, [0.1, 0.1, 0.1])
    with pytest.raises(ValueError, match=r"means must hold one entry per data set \(2\); got 1"):
        check(k, Xs, ys, [0.1, 0.1], [None])
    with pytest.raises(ValueError, match=r"ys\[1\] must have shape \(7,\) for data set 1; got \(5,\)"):
        check(k, Xs, [ys[0], ys[0]], [0.1, 0.1])
    with pytest.raises(ValueError, match=r"ys\[0\] must have shape \(5,\) for data set 0; got \(\)"):
        check(k, Xs, [1.0, ys[1]], [0.1, 0.1])
    with pytest.raises(ValueError, match=r"diags\[1\] must have shape \(7,\) or be a scalar for data set 1; got \(5,\)"):
        check(k, Xs, ys, [0.1, np.full(5, 0.1)])
    with pytest.raises(ValueError, match=r"means\[0\] must have shape \(5,\) or be a scalar for data set 0; got \(2,\)"):
        check(k, Xs, ys, [0.1, 0.1], [np.zeros(2), None])
    with pytest.raises(ValueError, match="data set 1 is empty"):
        check(k, [Xs[0], np.zeros((0, 3))], [ys[0], np.zeros(0)], [0.1, 0.1])
    with pytest.raises(ValueError, match="data set 1: its points have 1 input dimensions, the set's have 3"):
        check(k, [Xs[0], dn.train(7, 1)[0]], ys, [0.1, 0.1])
    with pytest.raises(ValueError, match="data set 1: .*ndim=3"):
        check(k, [Xs[0], np.zeros((7, 3, 1))], ys, [0.1, 0.1])
    with pytest.raises(NotImplementedError, match="QuasisepSolver"):
        tinygp_amd.log_probability_datasets(quasisep.Matern32(1.0), [np.arange(4.0)], [np.zeros(4)], diags=[0.1])


# ---- the route --------------------------------------------------------------------------------------------------------
def test_route_by_length_and_lowerability():
    X1, X3 = dn.train(6, 1)[0], dn.train(6, 3)[0]
    low = small.lower_member(kernels.Matern32(1.5), X3)
    assert low is not None and small.batched_route(1, low) and small.batched_route(ds.CAP, low)
    assert not small.batched_route(ds.CAP + 1, low) and not small.batched_route(0, low)
    custom = kernels.Custom(lambda a, b: np.exp(-np.sum(np.square(a - b))))
    assert small.lower_member(custom, X3) is None and not small.batched_route(6, None)
    assert small.lower_member(kernels.Matern32(1.5) + custom, X3) is None
    assert small.lower_member(kernels.Matern32(1.5), np.zeros((6, 17))) is None  # beyond the device evaluator
    assert small.lower_member(kernels.Matern32(1.5), np.zeros((6, 16))) is not None
    assert small.lower_member(kernels.Matern32(1.5), {"a": X1, "b": X1}) is None  # pytree input
    prog, P = small.lower_member(transforms.Linear(np.array([1.0, 2.0, 0.5]), kernels.ExpSquared(1.0)), X3)
    assert np.array_equal(P, X3 * np.array([1.0, 2.0, 0.5])) and prog == kernels.ExpSquared(1.0).program()
    assert small.MAX_N == ds.CAP == _ffi.SMALL_MAX_N


def test_route_of_a_batch_by_length_noise_model_and_lowerability():
    X3 = dn.train(6, 3)[0]
    low = small.lower_member(kernels.Matern32(1.5), X3)
    other = small.lower_member(kernels.Exp(1.0) * kernels.Cosine(2.0), X3)
    assert small.batch_route(6, True, [low, other]) and small.batch_route(ds.CAP, True, [low])
    assert not small.batch_route(ds.CAP + 1, True, [low, other])  # above the cap
    assert not small.batch_route(6, False, [low, other])  # the solver's noise model is not Diagonal
    assert not small.batch_route(6, True, [low, None, other])  # a member without a device program
    sub = small.lower_member(transforms.Subspace(0, kernels.Matern32(1.5)), X3)
    assert sub[1].shape == (6, 1) and not small.batch_route(6, True, [low, sub])  # members of different dimension


def test_public_entry_points_exist():
    from tinygp_amd.solvers import DirectSolver, QuasisepSolver

    assert tinygp_amd.log_probability_datasets is small.log_probability_datasets
    assert callable(DirectSolver.log_probability_batch) and not hasattr(DirectSolver, "value_and_grad_batch")
    doc = tinygp_amd.GaussianProcess.log_probability_batch.__doc__
    assert "differ in structure" in doc and "1e-8" in doc and "QuasisepSolver" in doc
    assert callable(QuasisepSolver.log_probability_batch)


# ---- header, prototype, binding -----------------------------------------------------------------------------------------
def test_header_constant_prototype_and_binding_agree():
    text = (ROOT / "include" / "tgp_hip.h").read_text()
    cap = int(re.search(r"#define\s+TGP_SMALL_MAX_N\s+(\d+)", text).group(1))
    assert cap == _ffi.SMALL_MAX_N == small.MAX_N
    assert int(re.search(r"#define\s+TGP_ABI_VERSION\s+(\d+)", text).group(1)) == _ffi.ABI_VERSION == 6
    # the largest member, with the reduction scratch, fits the 160 KiB a workgroup may hold
    assert (cap * (cap + 1) // 2 + cap) * 8 + 2 * 256 * 8 <= 163840
    proto = re.search(r"int\s+tgp_small_logprob\s*\((.*?)\)\s*;", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S)
    args = [" ".join(a.split()) for a in proto.group(1).split(",")]
    ctype = {"tgp_ctx*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "const tgp_kop*": C.c_void_p,
             "const int32_t*": _ffi._pi32, "const int64_t*": _ffi._pi64, "const double*": C.c_void_p,
             "int32_t*": _ffi._pi32, "double*": _ffi._pdbl}
    want = [ctype[a.rsplit(" ", 1)[0]] for a in args]
    assert [a.rsplit(" ", 1)[1] for a in args] == ["ctx", "nb", "progs", "prog_off", "x_off", "n", "d", "X_host", "x_rows",
                                                   "vec_off", "noise_host", "resid_host", "info_host", "out_host"]
    assert _ffi.SIGNATURES["tgp_small_logprob"] == want
    lib = _ffi.load_library()  # needs no GPU
    assert lib.tgp_small_logprob.argtypes == want and lib.tgp_abi_version() == 6
    # without a context the call is refused before anything is touched; an empty batch is a success
    assert lib.tgp_small_logprob(None, 1, None, None, None, None, 1, None, 0, None, None, None, None, None) == _ffi.E_ARG
    assert b"null context" in lib.tgp_last_error()


# ---- the reference's own conditions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
def test_reference_conditions_at_every_edge_shape(d):
    worst_cond = worst_diff = 0.0
    for n in ds.EDGE_NS + (ds.CAP + 1,) + ds.RAGGED + tuple(n for n, _ in ds.FAIL_CASES) + (8,):
        for b in range(max(ds.BS) if n in ds.EDGE_NS else len(ds.RAGGED)):
            f = ds.reference(n, d, b).figures
            worst_cond, worst_diff = max(worst_cond, f.cond), max(worst_diff, f.longdouble_diff)
    print(f"d = {d}: worst cond {worst_cond:.3g}, worst float64 - long double {worst_diff:.3g}")
    assert worst_cond <= ds.COND_MAX and worst_diff <= ds.LONGDOUBLE_RTOL
    # member 0 is _dense_np's kernel itself
    X = dn.train(17, d)[0]
    assert np.array_equal(ds.member_kernel(ds.o, d, 0)(X, X), dn.kernel(ds.o, d)(X, X))
    assert np.array_equal(ds.member_kernel(ds.o, d, 0, other=True)(X, X), dn.other_kernel(ds.o, d)(X, X))


@pytest.mark.parametrize("D", ds.LEAF_DS)
def test_reference_conditions_of_every_leaf_and_operator(D):
    members = ds.leaf_members(kernels, transforms)
    names = [m[0] for m in members]
    for leaf in ("Constant", "Exp", "ExpSquared", "Matern32", "Matern52", "Cosine", "ExpSineSquared", "RationalQuadratic",
                 "DotProduct", "Polynomial", "sum", "product", "nested", "metrics", "linear_a", "linear_b"):
        assert leaf in names
    X = ds.leaf_points(D)
    structures = set()
    for b, (name, kernel, oracle_matrix) in enumerate(members):
        _, f = ds.leaf_reference(oracle_matrix, D, b)
        assert f.cond <= ds.COND_MAX and f.longdouble_diff <= ds.LONGDOUBLE_RTOL, name
        low = small.lower_member(kernel, X)
        assert low is not None, name
        structures.add(tuple((op, metric) for op, metric, _, _ in low[0]))
    assert len(structures) >= 14  # one batch, members of different structure
    pa = small.lower_member(members[names.index("linear_a")][1], X)[1]
    pb = small.lower_member(members[names.index("linear_b")][1], X)[1]
    assert not np.array_equal(pa, pb) and np.array_equal(pa, 0.8 * small.lower_member(members[1][1], X)[1])
