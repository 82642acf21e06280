"""The conditions of the two-point probe's reference (``_kernel_derivs.py``), without a GPU: every member well posed,
every closed form pinned to central differences, every parameter's derivative carried by an off-diagonal term well
above its bar at some pair, and a table of deliberately wrong closed forms that the chosen pairs tell apart.  The GPU
file (``test_gpu_2_kernel_derivs.py``) only reads the cached reference."""
import numpy as np
import pytest

from oracle import grad_np
from oracle import kernel_derivs_np as kd
from oracle import tinygp_np as o

import _kernel_derivs as kv
import _nonstationary_np as ns

METRICS = (o.L1Distance, o.L2Distance)
LEAVES = (("Exp", {}), ("ExpSquared", {}), ("Matern32", {}), ("Matern52", {}), ("Cosine", {}),
          ("ExpSineSquared", dict(gamma=0.7)), ("RationalQuadratic", dict(alpha=1.3)))
PIN = dict(rtol=2e-7, atol=2e-8)  # tests/test_oracle.py's tolerance for the closed forms it pins


def _members(dtype="float64", pairs=None):
    for name, prog in kv.PROGRAMS.items():
        for D in kv.DS:
            for pair in kv.pairs_of(prog) if pairs is None else pairs:
                yield kv.reference(name, D, pair, dtype)


# ---- 1. the members are well posed ---------------------------------------------------------------------------------------
def test_every_member_is_well_posed():
    worst = 0.0
    count = 0
    for ref in _members():
        what = (ref.name, ref.D, ref.pair)
        assert ref.cond <= kv.COND_MAX, what + (ref.cond,)
        assert np.isfinite(ref.ll) and abs(ref.ll) >= 1e-2, what + (ref.ll,)
        assert np.all(np.isfinite(ref.g)) and np.all(np.isfinite(ref.noise)) and np.all(np.isfinite(ref.alpha)), what
        assert np.all(ref.noise_diag > 0), what
        worst = max(worst, ref.cond)
        count += 1
    for name in kv.FP32_PROGRAMS:
        for D in kv.DS:
            for pair in kv.FP32_PAIRS:
                ref = kv.reference(name, D, pair, "float32")
                assert ref.cond <= kv.COND_MAX and abs(ref.ll) >= 1e-2, (name, D, pair, ref.cond, ref.ll)
                assert ref.X.dtype == ref.y.dtype == ref.noise_diag.dtype == np.float32
    print(f"{count} members, worst cond(K) {worst:.3g}")


def test_the_degenerate_pairs_are_what_they_claim():
    for D in kv.DS:
        X = kv.pair_points("tiny", D)
        d = X[0] - X[1]
        assert np.sum(np.abs(d)) == 1e-200 and np.sum(d * d) == 0.0  # r2 underflows, r1 does not
        X = kv.pair_points("far", D)
        # the smallest argument any leaf sees (L2 at D = 1 .. 16, the largest scale 2.7): exp(-a) is zero in float64
        assert np.exp(-np.sqrt(np.sum((X[0] - X[1]) ** 2)) / 2.7) == 0.0
        X = kv.pair_points("close", D)
        assert np.allclose(np.abs(X[0] - X[1]), 1e-9, rtol=1e-6)
        X = kv.pair_points("one_coordinate", D)
        assert np.count_nonzero(X[0] - X[1]) == 1
        assert np.array_equal(*kv.pair_points("identical", D))
        assert np.count_nonzero(kv.pair_points("generic", D)[0] - kv.pair_points("generic", D)[1]) == D


def test_the_programs_reach_the_evaluators_limits():
    from tinygp_amd import kernels, transforms
    from tinygp_amd.kernels import base

    deep = kv.kernel("deep8", 3, kernels, transforms).program()
    assert base._stack_peak(deep) == base.KSTACK_MAX == 8 and len(deep) == 15
    assert [op for op, *_ in deep[:8]] == [base.K_EXP, base.K_EXPSQ, base.K_M32, base.K_M52, base.K_COS, base.K_ESS,
                                           base.K_RQ, base.K_CONST]
    assert len(kv.kernel("long32", 3, kernels, transforms).program()) == base.KPROG_MAX == 32
    # the reference's parameters are the product's, in its order
    for name, prog in kv.PROGRAMS.items():
        k = kv.kernel(name, 3, kernels, transforms)
        inner = k.kernel if prog.transform else k
        got = [getattr(obj, attr) for obj, attr in inner.parameters()]
        want = [d[key] for d, key in prog.tree.slots()]
        assert got == want, name
        assert kv.reference(name, 3, "generic").n_kernel == len(want), name
        assert (transforms.covering_transform(k) is not None) == (prog.transform is not None), name


# ---- 2. every closed form against central differences ---------------------------------------------------------------------
@pytest.mark.parametrize("d", (1, 3))
def test_log_scale_forms_match_central_differences_of_the_oracle(d):
    """d k / d log s_q of every stationary leaf under either metric: central differences of the oracle's kernel matrix
    on the scaled points (``grad_np.Scaled``) with respect to s_q, times s_q."""
    rng = np.random.default_rng(4)
    X1, X2 = rng.uniform(-2, 2, (6, d)), rng.uniform(-2, 2, (5, d))
    s = rng.uniform(0.6, 1.6, d)
    for kind, extra in LEAVES:
        for metric in METRICS:
            leaf = getattr(o, kind)(0.9, distance=metric(), **extra)
            got = kd.dleaf_dlogscale(leaf, X1 * s, X2 * s)
            assert got.shape == (d, 6, 5)
            for q in range(d):
                h = 1e-6
                sp, sm = s.copy(), s.copy()
                sp[q] += h
                sm[q] -= h
                want = s[q] * (grad_np.Scaled(sp, leaf)(X1, X2) - grad_np.Scaled(sm, leaf)(X1, X2)) / (2 * h)
                np.testing.assert_allclose(got[q], want, err_msg=f"{kind} {metric.__name__} d={d} q={q}", **PIN)
            # the weights sum to one: scaling every dimension is scaling 1 / l
            np.testing.assert_allclose(got.sum(axis=0), -0.9 * kd.dleaf(leaf, X1 * s, X2 * s), rtol=1e-12, atol=1e-14)


def test_log_scale_forms_at_coincident_points_are_zero():
    X = np.array([[0.3, -1.2, 0.7]])
    for kind, extra in LEAVES:
        for metric in METRICS:
            got = kd.dleaf_dlogscale(getattr(o, kind)(0.9, distance=metric(), **extra), X, X)
            assert np.array_equal(got, np.zeros((3, 1, 1))), (kind, metric.__name__)


@pytest.mark.parametrize("d", (1, 3))
def test_dot_product_forms_match_central_differences(d):
    """DotProduct's and Polynomial's derivatives (scale, sigma, order, log s_q) against central differences of the
    tests' own evaluator of the DOT / POW program (``_nonstationary_np.eval_prog``, from kernels/base.py:212-256)."""
    from tinygp_amd.kernels import base

    rng = np.random.default_rng(5)
    X1, X2 = rng.uniform(0.2, 1.5, (6, d)), rng.uniform(0.2, 1.5, (5, d))
    l, sg, P, h = 1.4, 0.8, 2.5, 1e-6

    def poly(l=l, sg=sg, P=P, s=np.ones(d)):
        return ns.eval_prog([(base.K_DOT, 0, l, sg), (base.K_POW, 0, P, 0.0)], X1 * s, X2 * s)

    u = kd.dot_value(X1, X2, l, sg)
    np.testing.assert_allclose(u**P, poly(), rtol=1e-14)
    np.testing.assert_allclose(kd.dot_value(X1, X2), ns.eval_prog([(base.K_DOT, 0, 1.0, 0.0)], X1, X2), rtol=1e-14)
    chain = P * u ** (P - 1)
    np.testing.assert_allclose(chain * kd.ddot(X1, X2, l, sg, "scale"), (poly(l=l + h) - poly(l=l - h)) / (2 * h), **PIN)
    np.testing.assert_allclose(chain * kd.ddot(X1, X2, l, sg, "sigma"), (poly(sg=sg + h) - poly(sg=sg - h)) / (2 * h), **PIN)
    np.testing.assert_allclose(u**P * np.log(u), (poly(P=P + h) - poly(P=P - h)) / (2 * h), **PIN)
    got = kd.ddot_dlogscale(X1, X2, l)
    for q in range(d):
        sp, sm = np.ones(d), np.ones(d)
        sp[q] += h
        sm[q] -= h
        np.testing.assert_allclose(chain * got[q], (poly(s=sp) - poly(s=sm)) / (2 * h), **PIN)


@pytest.mark.parametrize("D", (1, 3))
def test_every_programs_derivatives_match_central_differences_of_its_value(D):
    """The composition -- sum, product and power rules, the chain through ``Linear`` / ``Cholesky`` -- of every program:
    each dK against central differences of the program's own K (the oracle's leaves) in long double, step 1e-7
    (truncation ~1e-14, rounding ~1e-12 of K)."""
    for name, prog in kv.PROGRAMS.items():
        for pair in ("generic", "one_coordinate"):
            X = np.asarray(kv.pair_points(pair, D)).astype(kv.LD)
            dks, dts = prog.derivs(X)
            slots = prog.tree.slots()
            assert len(slots) == len(dks), name
            for (store, key), dK in zip(slots, dks):
                keep = store[key]
                h = kv.LD(1e-7)
                try:
                    store[key] = kv.LD(keep) + h
                    up = prog.value(X)
                    store[key] = kv.LD(keep) - h
                    down = prog.value(X)
                finally:
                    store[key] = keep
                np.testing.assert_allclose(np.float64(dK), np.float64((up - down) / (2 * h)), err_msg=f"{name} {key}", **PIN)
            assert len(dts) == (D if prog.transform else 0), name
            for q, dK in enumerate(dts):
                keep = prog.vectors[D]
                h = kv.LD(1e-7)
                try:
                    v = keep.astype(kv.LD)
                    v[q] += h
                    prog.vectors[D] = v
                    up = prog.value(X)
                    v = keep.astype(kv.LD)
                    v[q] -= h
                    prog.vectors[D] = v
                    down = prog.value(X)
                finally:
                    prog.vectors[D] = keep
                np.testing.assert_allclose(np.float64(dK), np.float64((up - down) / (2 * h)), err_msg=f"{name} q={q}", **PIN)


def test_the_two_by_two_closed_form_is_the_lapack_gradient():
    """det, K^-1, alpha and ll written out for 2 x 2 against the project's other analytic route (Cholesky, dpotri)."""
    import scipy.linalg as sla

    for name in ("amp*Matern52_L2", "deep8", "Linear(Polynomial)"):
        ref = kv.reference(name, 3, "generic")
        X = np.asarray(ref.X).astype(kv.LD)
        K = np.float64(kv.PROGRAMS[name].value(X)) + np.diag(ref.noise_diag)
        L = sla.cholesky(K, lower=True)
        alpha = sla.cho_solve((L, True), np.asarray(ref.y))
        ll = -0.5 * ref.y @ alpha - np.sum(np.log(np.diag(L))) - np.log(2 * np.pi)
        G = np.outer(alpha, alpha) - np.linalg.inv(K)
        dks, dts = kv.PROGRAMS[name].derivs(X)
        g = [0.5 * np.sum(G * np.float64(dK)) for dK in list(dks) + list(dts)]
        np.testing.assert_allclose(ref.ll, ll, rtol=1e-13)
        np.testing.assert_allclose(ref.g, g, rtol=1e-11, atol=1e-12 * np.abs(ref.g).max())
        np.testing.assert_allclose(ref.noise, 0.5 * np.diag(G), rtol=1e-11)
        np.testing.assert_allclose(ref.alpha, alpha, rtol=1e-12)


# ---- 3. no derivative passes on the atol term alone -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype,pairs", (("float64", kv.NONDEGENERATE), ("float32", ("generic", "one_coordinate"))))
def test_every_parameter_has_an_off_diagonal_term_of_100_bars(dtype, pairs):
    """For every (program, parameter, D) some non-degenerate pair has |G_10 dK_10| >= 100 of that parameter's bar.  (The
    float32 row: the programs and pairs the single path runs in float32, at that dtype's bars.)"""
    lightest = (np.inf, None)
    names = kv.PROGRAMS if dtype == "float64" else kv.FP32_PROGRAMS
    for name in names:
        for D in kv.DS:
            refs = [kv.reference(name, D, pair, dtype) for pair in pairs]
            for p in range(len(refs[0].g)):
                best = max(r.weight[p] for r in refs)
                assert best >= kv.WEIGHT_MIN, (name, D, p, [float(r.weight[p]) for r in refs])
                lightest = min(lightest, (best, (name, D, p)))
    print(f"{dtype}: the lightest parameter's best off-diagonal term is {lightest[0]:.3g} bars at {lightest[1]}")


# ---- 4. the pairs tell the formulas apart -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", kv.VARIANTS)
def test_a_wrong_closed_form_moves_the_reference_by_100_bars(variant):
    moved, where, changed = 0.0, None, 0
    try:
        for name in kv.PROGRAMS:
            for D in kv.DS:
                for pair in kv.NONDEGENERATE:
                    kv.WRONG.clear()
                    right = kv.reference(name, D, pair)
                    kv.WRONG.add(variant)
                    wrong = kv._compute(name, D, pair, "float64")
                    assert wrong.ll == right.ll and np.array_equal(wrong.alpha, right.alpha)  # (only dK moves)
                    if not len(right.g):
                        continue
                    with np.errstate(divide="ignore", invalid="ignore"):
                        by = np.where(wrong.g == right.g, 0.0, np.abs(wrong.g - right.g) / right.bars)
                    changed += bool(by.max() > 0)
                    if by.max() > moved:
                        moved, where = float(by.max()), (name, D, pair)
    finally:
        kv.WRONG.clear()
    print(f"{variant}: moves g by {moved:.3g} bars at {where}; {changed} members change")
    assert moved >= kv.WEIGHT_MIN, (variant, moved, where)
