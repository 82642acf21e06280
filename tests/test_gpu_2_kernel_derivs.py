"""Every kernel derivative the device evaluates, pair by pair, on both dense paths, against 2 x 2 closed forms.

The derivative evaluators (``leaf_deriv``, ``eval_kprog_deriv``, ``eval_kprog_deriv_dim``, ``pow_deriv`` of
``csrc/kprog_eval.h``; ``leaf_deriv_fast`` / ``FastEval`` of ``csrc/kmat.hip``) are hand-derived formulas.  A member
here is a GP on TWO points, whose gradient  g_p = 1/2 G_00 dK_00 + G_10 dK_10 + 1/2 G_11 dK_11  shows the device's
derivative at one chosen pair on its own; the reference is that closed form in long double with dK from
``oracle/kernel_derivs_np.py`` (``_kernel_derivs.py``; its conditions -- cond(K), every closed form pinned to central
differences, an off-diagonal term of at least 100 bars for every parameter, a table of wrong formulas that the pairs
tell apart -- are asserted by ``test_kernel_derivs_cpu.py``, and this file only reads the cached reference).

Programs: every stationary leaf under L1 and L2 as ``leaf``, ``amp * leaf`` and ``leaf * amp``; products of leaves of
different metrics and a sum of products; a right-nested program at stack depth 8 and one of 32 operations; DotProduct,
Polynomial and Polynomial * Matern32; every leaf, a product, DotProduct and Polynomial under ``transforms.Linear(vector)``,
three under ``transforms.Cholesky(vector)``.  Pairs, at D = 1, 2, 3, 16: two generic ones, one that differs in one
coordinate, identical points, separations of 1e-9 and of 1e-200 (r2 underflows), and one at which exp(-a) underflows.

Paths: ``log_probability_and_grad_datasets`` (``tgp_small_logprob_grad``: one call per group of programs and D, one
two-point member per program and pair) and ``GaussianProcess.log_probability_and_grad`` at n = 2 (float64 for every
program at every pair; float32 at three pairs for the eight FastEval forms, ``amp * Cosine`` and ``Polynomial * Matern32``).

Bars: ``_dense_grad_np.BARS`` -- float64 ll 1e-8, kernel and transform 2e-6, noise 1e-6, mean 1e-7; float32 ll 5e-4, the
rest 2e-3; each an rtol plus that fraction of the largest component as atol.  Every number must be finite.

Measured on an MI355X, the worst error over all members in units of its bar (1 936 members on the small batch, as many on
the single path in float64, 120 in float32):
  small batch, float64          ll 7.3e-4  kernel 1.3e-5 (under a transform 0.031)  noise 1.7e-5  mean 6.4e-5
  single path, float64          ll 7.3e-4  kernel 1.3e-5 (under a transform 0.031)  noise 1.7e-5  mean 6.4e-5
  single path, float32          ll 6.5e-4  kernel 7.5e-3                            noise 2.8e-4  mean 1.2e-4
The 0.031 is ``Cholesky(Exp_L2)`` at the separation of 1e-9: the host folds the transform into the coordinates in
float64 before the device differences them, which leaves dx with a relative error of ~1e-7 there (the same rounding
applied to the reference alone moves it by 0.027 bars); the whole file runs in 3 s.

What the probe found, fixed in ``csrc/kprog_eval.h`` with it: RationalQuadratic's alpha derivative took ``log(1 + q)``
of the rounded sum, which is zero below q = eps, and returned q where the derivative is -q^2 / 2 (``RationalQuadratic``
and ``ESS_L2*RQ_L1`` at the separation of 1e-9: an error of 0.43 of the largest component, now ``log1p``); and the
per-dimension weight dx^2 / r2 was zero where r2 underflows while r1 > 0, although every L2 leaf falls back to the
distance r1 there (``Linear(Exp_L2)`` and ``Cholesky(Exp_L2)`` at the separation of 1e-200, Exp being the one leaf
whose derivative is of first order in r: the transform's gradient in that dimension came back 0 where it is of the
size of the scale's; now the L1 weight).
"""
import numpy as np
import pytest

import tinygp_amd
from tinygp_amd import GaussianProcess, kernels, transforms
from tinygp_amd.solvers import small

import _kernel_derivs as kv

pytestmark = pytest.mark.gpu


def _worse(worst, errors):
    for key, v in errors.items():
        worst[key] = max(worst.get(key, 0.0), v)


def _judge(ref, got, worst, failed):
    """Add member ``ref``'s errors to ``worst`` and, where it misses a bar, its name and message to ``failed``: a test
    names every member that fails, not the first."""
    _worse(worst, kv.errors(ref, *got))
    try:
        kv.check(ref, *got)
    except AssertionError as e:
        failed.append(f"{ref.name} D={ref.D} {ref.pair} {ref.dtype}: " + " ".join(str(e).split())[:400])


def _report(what, worst, members, failed):
    print(f"{what}: {members} members, worst error in bars " + " ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    assert not failed, f"{len(failed)} of {members} members miss a bar:\n" + "\n".join(failed)


@pytest.mark.parametrize("D", kv.DS)
@pytest.mark.parametrize("group", kv.GROUPS)
def test_small_batch_pair_by_pair(group, D):
    refs = [kv.reference(name, D, pair) for name, prog in kv.GROUPS[group].items() for pair in kv.pairs_of(prog)]
    ks = [kv.kernel(ref.name, D, kernels, transforms) for ref in refs]
    for k, ref in zip(ks, refs):  # every member in the batched launch
        assert small.batched_route(2, small.lower_member(k, np.asarray(ref.X))), ref.name
    values, grads, info = tinygp_amd.log_probability_and_grad_datasets(
        ks, [np.asarray(ref.X) for ref in refs], [np.asarray(ref.y) for ref in refs],
        diags=[np.asarray(ref.noise_diag) for ref in refs], return_info=True)
    assert values.shape == (len(refs),) and not info.any()
    worst, failed = {}, []
    for m, ref in enumerate(refs):
        assert (grads["transform"][m] is not None) == (kv.PROGRAMS[ref.name].transform is not None), ref.name
        assert len(grads["kernel"][m]) == ref.n_kernel, ref.name
        got = (values[m], kv.full_gradient(grads["kernel"][m], grads["transform"][m]), grads["noise_diag"][m],
               grads["mean"][m])
        _judge(ref, got, worst, failed)
    _report(f"small batch {group} D={D}", worst, len(refs), failed)


def _single(ref):
    gp = GaussianProcess(kv.kernel(ref.name, ref.D, kernels, transforms), np.asarray(ref.X), diag=np.asarray(ref.noise_diag))
    try:
        ll, g = gp.log_probability_and_grad(np.asarray(ref.y))
        assert gp.solver.info == 0 and gp.solver.dtype == np.dtype(ref.dtype), ref.name
    finally:
        gp.solver.close()
    assert (g["transform"] is not None) == (kv.PROGRAMS[ref.name].transform is not None), ref.name
    assert len(g["kernel"]) == ref.n_kernel, ref.name
    return ll, kv.full_gradient(g["kernel"], g["transform"]), g["noise_diag"], g["mean"]


@pytest.mark.parametrize("D", kv.DS)
@pytest.mark.parametrize("group", kv.GROUPS)
def test_single_dense_path_pair_by_pair(group, D):
    worst, failed, members = {}, [], 0
    for name, prog in kv.GROUPS[group].items():
        for pair in kv.pairs_of(prog):
            ref = kv.reference(name, D, pair)
            _judge(ref, _single(ref), worst, failed)
            members += 1
    _report(f"single path {group} D={D}", worst, members, failed)


@pytest.mark.parametrize("D", kv.DS)
def test_single_dense_path_in_float32(D):
    worst, failed, members = {}, [], 0
    for name in kv.FP32_PROGRAMS:
        for pair in kv.FP32_PAIRS:
            ref = kv.reference(name, D, pair, "float32")
            got = _single(ref)
            assert got[2].dtype == got[3].dtype == np.float32
            _judge(ref, got, worst, failed)
            members += 1
    _report(f"single path float32 D={D}", worst, members, failed)
