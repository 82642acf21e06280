"""Batches of small dense GPs in one launch, one workgroup per member (``csrc/small.hip``, ``tgp_small_logprob``) through
``DirectSolver.log_probability_batch``, ``log_probability_datasets`` and ``GaussianProcess.log_probability_batch``.

Inputs and references: ``_dense_small.py`` (SciPy LAPACK in float64 on the oracle's matrix, its own conditions asserted).
Bar: the project's log-likelihood bar, ``|got - want| <= 1e-8 max(1, |want|)``; independence and the above-the-cap route
are held with tolerance zero."""
import numpy as np
import pytest

import tinygp_amd
from tinygp_amd import GaussianProcess, _ffi, kernels, transforms
from tinygp_amd.kernels import quasisep
from tinygp_amd.noise import Dense, Diagonal
from tinygp_amd.solvers import DirectSolver, small

import _dense_np as dn
import _dense_small as ds

pytestmark = pytest.mark.gpu

CAP = ds.CAP


def _batch(n, d, members, *, noise=None, resid=None):
    """``(values, info)`` of the given members (indices b) over ``_dense_np.train(n, d)`` through the solver's batch."""
    X, diag = dn.train(n, d)
    solver = DirectSolver(ds.member_kernel(kernels, d, 0), X, Diagonal(diag))
    try:
        ks = [ds.member_kernel(kernels, d, b) for b in members]
        nz = np.stack([ds.member_noise(n, d, b) for b in members]) if noise is None else noise
        return solver.log_probability_batch(ks, ds.resid(n) if resid is None else resid, nz, return_info=True)
    finally:
        solver.close()


def _assert_bar(got, want, what):
    print(f"{what}: got {float(got)!r} want {want!r} |diff| {abs(float(got) - want):.3g}")
    assert ds.within_bar(got, want), (what, float(got), want)


# ---- 1. parity at the edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
@pytest.mark.parametrize("n", ds.EDGE_NS)
def test_parity_at_the_edges(n, d):
    for B in ds.BS:
        values, info = _batch(n, d, range(B))
        assert values.shape == (B,) and values.dtype == np.float64 and info.dtype == np.int32
        assert not info.any(), info
        for b in range(B):
            _assert_bar(values[b], ds.reference(n, d, b).value, f"n={n} d={d} B={B} member {b}")


# ---- 2. every leaf and operator ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", ds.LEAF_DS)
def test_every_leaf_and_operator_in_one_batch(D):
    members = ds.leaf_members(kernels, transforms)
    X, n = ds.leaf_points(D), ds.LEAF_N
    noise = np.stack([ds.leaf_noise() * (1.0 + 0.1 * b) for b in range(len(members))])
    solver = DirectSolver(members[1][1], X, Diagonal(ds.leaf_noise()))
    try:
        lowered = [small.lower_member(k, X) for _, k, _ in members]
        assert small.batch_route(n, True, lowered)  # one launch: none of them falls back to the single path
        names = [m[0] for m in members]
        pa, pb = lowered[names.index("linear_a")][1], lowered[names.index("linear_b")][1]
        assert not np.array_equal(pa, pb)  # two members carry coordinates of their own
        values, info = solver.log_probability_batch([k for _, k, _ in members], ds.resid(n), noise, return_info=True)
    finally:
        solver.close()
    assert not info.any(), info
    for b, (name, _, oracle_matrix) in enumerate(members):
        want, _ = ds.leaf_reference(oracle_matrix, D, b)
        _assert_bar(values[b], want, f"D={D} {name}")


# ---- 3. independence, tolerance zero --------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
def test_a_members_bits_do_not_depend_on_the_batch(d):
    n, me = 8, 2  # member 2 at n = 8
    alone, info = _batch(n, d, [me])
    assert info[0] == 0
    _assert_bar(alone[0], ds.reference(n, d, me).value, f"d={d} alone")
    again, _ = _batch(n, d, [me])
    assert again[0] == alone[0]  # across two runs
    for members in ([me, 0, 1], [0, me, 1], [0, 1, me]):  # first, middle and last of B = 3
        values, _ = _batch(n, d, members)
        assert values[members.index(me)] == alone[0], members
    # inside B = 3 000: more workgroups than the device holds at once
    B = 3000
    members = [b % 7 for b in range(B)]
    for at in (0, B // 2, B - 1):
        members[at] = me
    values, info = _batch(n, d, members)
    assert not info.any()
    mine = values[np.array(members) == me]
    assert np.all(mine == alone[0]), np.unique(mine)
    for b in range(7):
        assert np.all(values[np.array(members) == b] == values[members.index(b)])
        _assert_bar(values[members.index(b)], ds.reference(n, d, b).value, f"d={d} B={B} member {b}")
    # beside a neighbour at the cap: the launch's LDS is sized by the larger member
    Xs = [dn.train(CAP, d)[0], dn.train(n, d)[0], dn.train(CAP, d)[0]]
    ks = [ds.member_kernel(kernels, d, 0), ds.member_kernel(kernels, d, me), ds.member_kernel(kernels, d, 1)]
    diags = [ds.member_noise(CAP, d, 0), ds.member_noise(n, d, me), ds.member_noise(CAP, d, 1)]
    for _ in range(2):
        values = tinygp_amd.log_probability_datasets(ks, Xs, [ds.resid(CAP), ds.resid(n), ds.resid(CAP)], diags=diags)
        assert values[1] == alone[0]
        _assert_bar(values[0], ds.reference(CAP, d, 0).value, f"d={d} neighbour at the cap")


# ---- 4. ragged sets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
def test_ragged_sets_of_data_sets(d):
    ns = ds.RAGGED
    Xs = [dn.train(n, d)[0] for n in ns]
    ks = [ds.member_kernel(kernels, d, b) for b in range(len(ns))]
    ys = [ds.resid(n) for n in ns]
    diags = [ds.member_noise(n, d, b) for b, n in enumerate(ns)]
    values, info = tinygp_amd.log_probability_datasets(ks, Xs, ys, diags=diags, return_info=True)
    assert values.shape == (len(ns),) and values.dtype == np.float64 and not info.any()
    for b, n in enumerate(ns):
        _assert_bar(values[b], ds.reference(n, d, b).value, f"d={d} data set {b} (n={n})")
        shared, _ = _batch(n, d, [b])
        assert values[b] == shared[0], (b, n)  # the bits of the same member through the shared-X call
    # one kernel for all; a scalar diagonal and a scalar mean behave as their broadcast arrays
    scalar = tinygp_amd.log_probability_datasets(ks[0], Xs, ys, diags=[0.1 + 0.01 * b for b in range(len(ns))],
                                                 means=[None, 0.3, 0.0, -0.2, None, 1.5])
    arrays = tinygp_amd.log_probability_datasets([ks[0]] * len(ns), Xs, ys,
                                                 diags=[np.full(n, 0.1 + 0.01 * b) for b, n in enumerate(ns)],
                                                 means=[None, np.full(ns[1], 0.3), np.zeros(ns[2]), np.full(ns[3], -0.2),
                                                        None, np.full(ns[5], 1.5)])
    assert np.array_equal(scalar, arrays) and np.all(np.isfinite(scalar))
    plain = tinygp_amd.log_probability_datasets(ks[0], Xs, ys, diags=[0.1 + 0.01 * b for b in range(len(ns))])
    assert plain[0] == scalar[0] and plain[2] == scalar[2] and plain[1] != scalar[1]


# ---- 5. failure -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
@pytest.mark.parametrize("n,p", ds.FAIL_CASES)
def test_failed_pivot_is_reported_and_stays_in_its_member(n, p, d):
    members = [0, 1, 2]
    good = np.stack([ds.member_noise(n, d, b) for b in members])
    clean, info = _batch(n, d, members)
    assert not info.any()
    without, _ = _batch(n, d, [0, 2])
    assert np.array_equal(without, clean[[0, 2]])
    for bad_value in (-2.0, np.nan):
        noise = np.array(good)
        noise[1, p] = bad_value  # the leading minor is positive definite, K_pp + noise_p < 0: pivot p + 1 fails
        values, info = _batch(n, d, members, noise=noise)
        assert info.tolist() == [0, p + 1, 0], (bad_value, info)
        assert values[1] == -np.inf
        assert values[0] == clean[0] and values[2] == clean[2]
    resid = np.tile(ds.resid(n), (3, 1))
    resid[1, n // 2] = np.nan
    values, info = _batch(n, d, members, resid=resid)
    assert info.tolist() == [0, 0, 0] and values[1] == -np.inf
    assert values[0] == clean[0] and values[2] == clean[2]


# ---- 6. above the cap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
def test_above_the_cap_is_the_single_path(d):
    n = CAP + 1
    X, y = dn.train(n, d)[0], ds.resid(n)
    single = [GaussianProcess(ds.member_kernel(kernels, d, b), X, diag=ds.member_noise(n, d, b)).log_probability(y)
              for b in range(2)]
    values, info = _batch(n, d, [0, 1])
    assert not info.any()
    for b in range(2):
        assert values[b] == single[b]  # the same path: the same bits
        _assert_bar(values[b], ds.reference(n, d, b).value, f"d={d} n={n} member {b}")
    # one such member among small ones: the order of the results is the caller's
    ns = (17, n, 64)
    got = tinygp_amd.log_probability_datasets([ds.member_kernel(kernels, d, b) for b in (2, 1, 0)],
                                              [dn.train(m, d)[0] for m in ns], [ds.resid(m) for m in ns],
                                              diags=[ds.member_noise(m, d, b) for m, b in zip(ns, (2, 1, 0))])
    assert got[1] == single[1]
    _assert_bar(got[0], ds.reference(17, d, 2).value, f"d={d} data set 0 beside a large one")
    _assert_bar(got[2], ds.reference(64, d, 0).value, f"d={d} data set 2 beside a large one")


def test_the_raw_call_validates_its_arguments():
    ctx = _ffi.default_ctx()
    n, d = 5, 3
    good = small.pack_members([small.lower_member(ds.member_kernel(kernels, d, 0), dn.train(n, d)[0])
                               + (ds.member_noise(n, d, 0), ds.resid(n))])
    values, info = small.run_packed(ctx, good)
    _assert_bar(values[0], ds.reference(n, d, 0).value, "raw call")
    big = CAP + 1
    Xb = np.ascontiguousarray(dn.train(big, d)[0])
    over = good._replace(n=np.array([big], dtype=np.int32), X=Xb, noise=np.ones(big), resid=np.ones(big))
    with pytest.raises(ValueError, match=rf"member 0: n must be 1 \.\. {CAP}"):
        small.run_packed(ctx, over)
    for bad, match in ((good._replace(n=np.array([0], dtype=np.int32)), "member 0: n must be"),
                       (good._replace(d=0), "input dimension"), (good._replace(d=17), "input dimension"),
                       (good._replace(x_off=np.array([1], dtype=np.int64)), "member 0: rows .* outside X"),
                       (good._replace(x_off=np.array([-1], dtype=np.int64)), "member 0: rows .* outside X"),
                       (good._replace(vec_off=np.array([-1], dtype=np.int64)), "member 0: negative offset"),
                       (good._replace(prog_off=np.array([0, 0], dtype=np.int32)), "member 0: empty"),
                       (good._replace(progs=np.array([(16, 0, 0.0, 0.0)], dtype=small.KOP_DTYPE)), "member 0: ")):
        with pytest.raises(ValueError, match=match):
            small.run_packed(ctx, bad)
    lib = _ffi.lib()
    assert lib.tgp_small_logprob(ctx.handle, 0, None, None, None, None, 0, None, 0, None, None, None, None, None) == 0


# ---- 7. the GP surface ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ds.DS)
def test_the_gp_surface(d):
    n, B = 65, 3
    X, diag = dn.train(n, d)
    y = ds.resid(n) + 0.25
    ks = [ds.member_kernel(kernels, d, b) for b in range(B)]
    gp = GaussianProcess(ks[0], X, diag=diag)
    # (B,) forms: one noise value and one constant mean per member
    dvals, mvals = np.array([0.05, 0.1, 0.2]), np.array([0.25, 0.0, -0.5])
    got = gp.log_probability_batch(y, ks, diags=dvals, means=mvals)
    assert got.shape == (B,) and got.dtype == np.float64
    for b in range(B):
        K = ds.member_kernel(ds.o, d, b)(X, X) + dvals[b] * np.eye(n)
        _assert_bar(got[b], ds.loglik(K, y - mvals[b])[0], f"d={d} (B,) forms member {b}")
    # (B, N) forms
    dmat = np.stack([ds.member_noise(n, d, b) for b in range(B)])
    mmat = np.stack([np.full(n, 0.25), np.linspace(0.0, 0.5, n), np.zeros(n)])
    got = gp.log_probability_batch(y, ks, diags=dmat, means=mmat)
    for b in range(B):
        K = ds.member_kernel(ds.o, d, b)(X, X) + np.diag(dmat[b])
        _assert_bar(got[b], ds.loglik(K, y - mmat[b])[0], f"d={d} (B, N) forms member {b}")
    # the GP's own noise and mean
    got = gp.log_probability_batch(y, ks)
    for b in range(B):
        _assert_bar(got[b], ds.loglik(ds.member_kernel(ds.o, d, b)(X, X) + np.diag(diag), y)[0], f"d={d} defaults {b}")
    empty = gp.log_probability_batch(y, [])
    assert empty.shape == (0,) and empty.dtype == np.float64
    out, info = gp.solver.log_probability_batch([], y, return_info=True)
    assert out.shape == (0,) and info.shape == (0,) and info.dtype == np.int32
    with pytest.raises(ValueError, match="resid must have shape"):
        gp.solver.log_probability_batch(ks, np.zeros((2, n)))
    with pytest.raises(ValueError, match="noise must have shape"):
        gp.solver.log_probability_batch(ks, np.zeros(n), np.zeros((B, n - 1)))
    with pytest.raises(NotImplementedError, match="QuasisepSolver"):
        gp.log_probability_and_grad_batch(y, ks)


@pytest.mark.parametrize("d", ds.DS)
def test_fp32_inputs_are_computed_in_fp64_and_returned_as_fp32(d):
    n, B = 65, 3
    X32, y32 = dn.train(n, d, "float32")[0], ds.resid(n, "float32")
    ks = [ds.member_kernel(kernels, d, b) for b in range(B)]
    dmat = np.stack([ds.member_noise(n, d, b, "float32") for b in range(B)])
    gp = GaussianProcess(ks[0], X32, diag=dmat[0])
    assert gp.dtype == np.float32
    got = gp.log_probability_batch(y32, ks, diags=dmat)
    assert got.dtype == np.float32 and got.shape == (B,)
    empty = gp.log_probability_batch(y32, [])
    assert empty.shape == (0,) and empty.dtype == np.float32
    for b in range(B):
        want = ds.reference(n, d, b, dtype="float32").value  # float64, at the rounded inputs
        ulp = float(np.spacing(np.float32(abs(want))))
        print(f"d={d} member {b}: got {float(got[b])!r} want {want!r} ulp {ulp:.3g}")
        assert abs(float(got[b]) - want) <= ulp


def test_members_the_device_cannot_lower_take_the_single_path():
    n, d = 40, 3
    X, diag = dn.train(n, d)
    y = ds.resid(n)
    custom = kernels.Custom(lambda a, b: 0.9 * np.exp(-0.5 * np.sum(np.square(a - b)) / 2.5**2))
    ks = [ds.member_kernel(kernels, d, 0), custom, ds.member_kernel(kernels, d, 1)]
    gp = GaussianProcess(ks[0], X, diag=diag)
    got = gp.log_probability_batch(y, ks)
    for b, k in enumerate(ks):
        assert got[b] == GaussianProcess(k, X, diag=diag).log_probability(y), b  # bit for bit: the same path
    _assert_bar(got[1], ds.loglik(ds.member_kernel(ds.o, d, 0, other=True)(X, X) + np.diag(diag), y)[0], "Custom member")
    sets = tinygp_amd.log_probability_datasets(ks, [X, X, X], [y, y, y], diags=[diag, diag, diag])
    assert sets[1] == got[1]
    _assert_bar(sets[0], got[0], "lowerable data set beside a Custom one")
    # a noise model that is not Diagonal: every member on the single path, with that model
    N = np.diag(diag) + 0.01
    dense = GaussianProcess(ks[0], X, noise=Dense(N))
    got = dense.log_probability_batch(y, [ks[0], ks[2]])
    for b, k in enumerate((ks[0], ks[2])):
        assert got[b] == GaussianProcess(k, X, noise=Dense(N)).log_probability(y)


def test_quasisep_kernels_on_the_dense_solver_still_raise():
    t = np.sort(np.random.default_rng(3).uniform(0.0, 10.0, 30))
    ks = [quasisep.Matern32(1.0 + 0.1 * b) for b in range(2)]
    dense = GaussianProcess(ks[0], t, diag=0.1, solver=DirectSolver)
    with pytest.raises(NotImplementedError, match="QuasisepSolver"):
        dense.log_probability_batch(np.zeros(30), ks)
    with pytest.raises(NotImplementedError, match="QuasisepSolver"):
        dense.log_probability_batch(np.zeros(30), [kernels.Matern32(1.0), ks[1]])
    with pytest.raises(NotImplementedError, match="QuasisepSolver"):
        dense.log_probability_and_grad_batch(np.zeros(30), ks)
