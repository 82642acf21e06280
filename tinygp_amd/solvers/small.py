"""Batches of small dense GPs in one launch (``tgp_small_logprob``, ``tgp_small_logprob_grad``, ``tgp_small_predict``,
``tgp_small_condition``, ``csrc/small.hip``): one
workgroup owns a whole member -- it assembles ``K + diag(noise)`` in LDS, factors it there, solves and reduces, and for
the gradient inverts in place and weighs every derivative -- where the single dense path pays a handle, uploads, a
launch chain and a host join per evaluation.

This module is the host side: lowering of the members (:func:`lower_member`), the packing of programs, coordinates,
noise and residuals into the arrays of the C ABI (:func:`pack_members`), the choice between the batched launches and
the single path (:func:`batched_route`), and :func:`log_probability_datasets`, the entry point for sets of data sets
with points of their own.  ``DirectSolver.log_probability_batch`` is built on the same pieces.  The gradient's side:
:func:`run_packed_grad`, the mapping of the device's ``[2 i + q]`` layout onto ``kernel.parameters()``
(:func:`member_gradient`), :func:`log_probability_and_grad_datasets` and ``DirectSolver.log_probability_and_grad_batch``.  The prediction's side:
:func:`pack_predict` (test points, second programs and output offsets beside the members), :func:`predict_rows` and
:func:`predict_launch_bytes` (the table rows and the staging bytes the C side makes of them),
:func:`run_packed_predict`, :func:`predict_datasets` and ``DirectSolver.predict_batch``.  The joint posterior's side
(``tgp_small_condition``): :func:`pack_condition`, :func:`condition_launch_bytes`, :func:`run_packed_condition`,
:func:`condition_datasets`, :func:`sample_conditional_datasets` and ``DirectSolver.condition_batch``.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from tinygp_amd import _device, _ffi

__all__ = ["MAX_N", "KOP_DTYPE", "Packed", "lower_member", "pack_members", "batched_route", "batch_route", "run_packed",
           "run_packed_grad", "member_gradient", "failed_gradient", "log_probability_datasets",
           "log_probability_and_grad_datasets", "PRED_CHUNK", "PackedPredict", "pack_predict", "predict_rows",
           "predict_launch_bytes", "run_packed_predict", "predict_datasets", "PackedCondition", "condition_route",
           "pack_condition", "condition_launch_bytes", "run_packed_condition", "host_draws", "condition_datasets",
           "sample_conditional_datasets"]

MAX_N = _ffi.SMALL_MAX_N  # TGP_SMALL_MAX_N: the largest member a workgroup holds in LDS
PRED_CHUNK = _ffi.SMALL_PRED_CHUNK  # TGP_SMALL_PRED_CHUNK: the test points one workgroup takes
STAGE_BYTES = 1 << 30  # the staging cap of one launch (SMALL_STAGE_BYTES of small.hip)

# ``tgp_kop`` as a NumPy record: the programs of a batch are one contiguous array of these
KOP_DTYPE = np.dtype([("op", np.int32), ("metric", np.int32), ("p0", np.float64), ("p1", np.float64)], align=True)
assert KOP_DTYPE.itemsize == 24

_QUASISEP_MESSAGE = ("batches of kernels.quasisep models are evaluated by QuasisepSolver (log_probability_batch on sorted "
                     "1-D inputs, log_probability_series for series with time stamps of their own), not by the dense path")


class Packed(NamedTuple):
    """The host arrays of one ``tgp_small_logprob`` call."""

    progs: np.ndarray     # (total ops,) KOP_DTYPE
    prog_off: np.ndarray  # (B + 1,) int32
    x_off: np.ndarray     # (B,) int64, rows into X
    n: np.ndarray         # (B,) int32
    d: int
    X: np.ndarray         # (rows, d) float64
    vec_off: np.ndarray   # (B,) int64, into noise and resid
    noise: np.ndarray     # (sum n,) float64
    resid: np.ndarray     # (sum n,) float64


def lower_member(kernel, X):
    """``(program, points)`` of one member -- the postfix program and the float64 (n, D) coordinates the device reads,
    input transforms folded in -- or ``None`` when the device cannot evaluate it (``kernels.Custom``, more than 16
    dimensions, pytree inputs): such a member takes the single path."""
    if _device.is_tree(X):
        return None
    try:
        prog, Xdev = kernel._lower(X)
        if _device.is_tree(Xdev):
            return None
        P = _device.points(Xdev, np.float64)
    except NotImplementedError:
        return None
    if prog is None or len(prog) == 0:
        return None
    return prog, P


def batched_route(n: int, lowered) -> bool:
    """Whether a member of ``n`` points goes into the batched launches: it has a device program and fits a workgroup."""
    return lowered is not None and 1 <= n <= MAX_N


def batch_route(n: int, diagonal_noise: bool, lowered) -> bool:
    """Whether a batch over ONE set of n points runs in the batched launches: a diagonal noise model, and every member
    with a device program, n within the cap and one input dimension after the members' transforms.  Otherwise every
    member is evaluated on the single path, so that the interface does not change with N."""
    lowered = list(lowered)
    if not diagonal_noise or not all(batched_route(n, low) for low in lowered):
        return False
    return len({low[1].shape[1] for low in lowered}) == 1


def pack_members(members, labels=None) -> Packed:
    """Stack B members ``(program, points (n_b, D), noise (n_b,), resid (n_b,))`` into the arrays of
    ``tgp_small_logprob``.  Members whose points are ``np.array_equal`` to member 0's share its rows of ``X`` (one
    uploaded copy: the shared-coordinates batch); every other member ships its own.  A ``ValueError`` names the member
    whose input dimension, length or vectors do not fit (``labels[b]`` instead of ``"member b"`` when given)."""
    members = list(members)
    labels = [f"member {b}" for b in range(len(members))] if labels is None else list(labels)
    if not members:
        raise ValueError("a batch needs at least one member")
    P0 = np.asarray(members[0][1])
    d = int(P0.shape[1])
    ops, prog_off, x_off, ns, vec_off, Xs, noises, resids = [], [0], [], [], [], [], [], []
    rows = total = 0
    for b, (prog, P, noise, resid) in enumerate(members):
        P = np.asarray(P, dtype=np.float64)
        if P.ndim != 2 or P.shape[1] != d:
            raise ValueError(f"{labels[b]}: its points must have shape (n, {d}) like member 0's; got {P.shape}")
        n = int(P.shape[0])
        if not 1 <= n <= MAX_N:
            raise ValueError(f"{labels[b]}: the batched dense path holds 1 .. {MAX_N} points per member (got {n})")
        noise, resid = np.asarray(noise, dtype=np.float64), np.asarray(resid, dtype=np.float64)
        if noise.shape != (n,) or resid.shape != (n,):
            raise ValueError(f"{labels[b]}: noise and resid must have shape ({n},); got {noise.shape} and {resid.shape}")
        if not 1 <= len(prog) <= 32:
            raise ValueError(f"{labels[b]}: a kernel program holds 1 .. 32 operations (got {len(prog)})")
        ops.extend((int(op), int(metric), float(p0), float(p1)) for op, metric, p0, p1 in prog)
        prog_off.append(len(ops))
        if b > 0 and P.shape == P0.shape and np.array_equal(P, P0):
            x_off.append(0)
        else:
            x_off.append(rows)
            Xs.append(P)
            rows += n
        ns.append(n)
        vec_off.append(total)
        noises.append(noise)
        resids.append(resid)
        total += n
    return Packed(np.array(ops, dtype=KOP_DTYPE), np.array(prog_off, dtype=np.int32), np.array(x_off, dtype=np.int64),
                  np.array(ns, dtype=np.int32), d, np.ascontiguousarray(np.concatenate(Xs, axis=0)),
                  np.array(vec_off, dtype=np.int64), np.concatenate(noises), np.concatenate(resids))


def run_packed(ctx, packed: Packed):
    """One ``tgp_small_logprob`` call: ``(values (B,) float64 -- NaN where the factor failed --, info (B,) int32)``."""
    nb = len(packed.n)
    info, out = np.zeros(nb, dtype=np.int32), np.empty(nb)
    _ffi.check(_ffi.lib().tgp_small_logprob(
        ctx.handle, nb, _ffi.ptr(packed.progs), packed.prog_off.ctypes.data_as(_ffi._pi32),
        packed.x_off.ctypes.data_as(_ffi._pi64), packed.n.ctypes.data_as(_ffi._pi32), packed.d, _ffi.ptr(packed.X),
        packed.X.shape[0], packed.vec_off.ctypes.data_as(_ffi._pi64), _ffi.ptr(packed.noise), _ffi.ptr(packed.resid),
        info.ctypes.data_as(_ffi._pi32), out.ctypes.data_as(_ffi._pdbl)), "tgp_small_logprob")
    return out, info


def run_packed_grad(ctx, packed: Packed, want_dims=None, *, vectors: bool = True):
    """One ``tgp_small_logprob_grad`` call: ``(values (B,), info (B,), grad_params (2 x total ops,), grad_noise (sum n,),
    alpha (sum n,), grad_logscale (B, d))``, all float64.  Member b's parameter gradients start at
    ``2 * packed.prog_off[b]`` in the ``[2 i + q]`` layout of ``tgp_solver_grad``; its two vectors sit at
    ``packed.vec_off[b]``.  ``want_dims``: (B,) flags, the members that also get ``d ll / d log s_q`` per input
    dimension (zero for the others); ``None``: nobody, and no such output.  ``vectors=False``: the two vectors are
    ``None`` and are not copied back.  A failed member has NaN everywhere."""
    nb = len(packed.n)
    info, out = np.zeros(nb, dtype=np.int32), np.empty(nb)
    gparams = np.zeros(2 * len(packed.progs))
    total = int(packed.n.sum())
    gnoise, alpha = (np.empty(total), np.empty(total)) if vectors else (None, None)
    flags = None if want_dims is None else np.ascontiguousarray(want_dims, dtype=np.int32)
    if flags is not None and flags.shape != (nb,):
        raise ValueError(f"want_dims must hold one flag per member ({nb}); got {flags.shape}")
    glog = None if flags is None else np.zeros((nb, packed.d))

    def pdbl(a):
        return None if a is None else a.ctypes.data_as(_ffi._pdbl)

    _ffi.check(_ffi.lib().tgp_small_logprob_grad(
        ctx.handle, nb, _ffi.ptr(packed.progs), packed.prog_off.ctypes.data_as(_ffi._pi32),
        packed.x_off.ctypes.data_as(_ffi._pi64), packed.n.ctypes.data_as(_ffi._pi32), packed.d, _ffi.ptr(packed.X),
        packed.X.shape[0], packed.vec_off.ctypes.data_as(_ffi._pi64), _ffi.ptr(packed.noise), _ffi.ptr(packed.resid),
        None if flags is None else flags.ctypes.data_as(_ffi._pi32), info.ctypes.data_as(_ffi._pi32), pdbl(out),
        pdbl(gparams), pdbl(gnoise), pdbl(alpha), pdbl(glog)), "tgp_small_logprob_grad")
    return out, info, gparams, gnoise, alpha, glog


def dims_flags(kernels):
    """The ``want_dims`` flags of a batch: 1 for the members whose kernel sits under ONE input transform
    (``transforms.covering_transform``), whose per-dimension scales the device then differentiates; ``None`` when no
    member has one (the call then has no such output)."""
    from tinygp_amd.transforms import covering_transform

    flags = np.array([covering_transform(k) is not None for k in kernels], dtype=np.int32)
    return flags if flags.any() else None


def member_gradient(kernel, gparams, glog=None):
    """``(kernel gradient, transform gradient)`` of one member from the device's layout: ``gparams[2 i + q]`` is
    parameter q of op i, and the float64 array returned follows ``kernel.parameters()`` (the ``_slots`` mapping of
    ``DirectSolver.log_probability_and_grad``).  ``glog``: the member's ``d ll / d log s_q`` row, or ``None``; the
    transform gradient is what ``covering_transform(kernel)._logscale_gradient`` makes of it, ``None`` without one."""
    slots: list = []
    kernel._slots(slots)
    if 2 * len(slots) != len(gparams):
        raise ValueError(f"the kernel has {len(slots)} program ops, the gradient holds {len(gparams)} entries")
    kgrad = np.array([gparams[2 * i + q] for i, pair in enumerate(slots) for q in (0, 1) if pair[q] is not None],
                     dtype=np.float64)
    from tinygp_amd.transforms import covering_transform

    tgrad = None
    tf = None if glog is None else covering_transform(kernel)
    if tf is not None:
        try:
            tgrad = tf._logscale_gradient(np.array(glog, dtype=np.float64))
        except NotImplementedError:
            tgrad = None  # (Subspace, a Python callable, a full matrix: no per-dimension scale)
    return kgrad, tgrad


def failed_gradient(kgrad, tgrad):
    """The two of :func:`member_gradient` for a member whose value is ``-inf``: NaN in the same shapes."""
    kgrad = np.full(len(kgrad), np.nan)
    return kgrad, (None if tgrad is None else np.full_like(np.asarray(tgrad, dtype=np.float64), np.nan))


def unpack_gradients(kernels, packed: Packed, results, where, values, info, kgrads, tgrads, noise_rows, mean_rows, dtypes):
    """Scatter one ``run_packed_grad`` result (launch member m is member ``where[m]`` of the caller's batch, its vectors
    come back in ``dtypes[m]``) into the caller's arrays and lists; a failed or non-finite member gets NaN gradients
    (the device already wrote NaN where the factor failed)."""
    out, infos, gparams, gnoise, alpha, glog = results
    for m, b in enumerate(where):
        lo, hi = 2 * int(packed.prog_off[m]), 2 * int(packed.prog_off[m + 1])
        kg, tg = member_gradient(kernels[b], gparams[lo:hi], None if glog is None else glog[m])
        at, n = int(packed.vec_off[m]), int(packed.n[m])
        bad = infos[m] != 0 or not np.isfinite(out[m])
        if bad:
            kg, tg = failed_gradient(kg, tg)
        values[b], info[b], kgrads[b], tgrads[b] = out[m], infos[m], kg, tg
        if gnoise is not None:
            noise_rows[b] = np.full(n, np.nan, dtype=dtypes[m]) if bad else gnoise[at:at + n].astype(dtypes[m])
            mean_rows[b] = np.full(n, np.nan, dtype=dtypes[m]) if bad else alpha[at:at + n].astype(dtypes[m])


def reject_quasisep(kernels):
    """The dense batch does not take ``kernels.quasisep`` models: their batches are ``QuasisepSolver``'s."""
    from tinygp_amd.kernels.quasisep import Quasisep

    if any(isinstance(k, Quasisep) for k in kernels):
        raise NotImplementedError(_QUASISEP_MESSAGE)


def check_datasets(kernels, Xs, ys, diags, means=None):
    """The members of a set of data sets, validated: a list of ``(kernel, X, y (n,), diag (n,), mean (n,) or None)`` with
    the vectors in the dtype of that data set's coordinates.  ``kernels`` is one kernel or one per data set; ``Xs[b]``
    is (n_b,) or (n_b, D) with one D for the whole set (pytrees pass through to the single path); ``diags[b]`` a scalar
    or (n_b,); ``means[b]`` ``None``, a scalar or (n_b,).  A ``ValueError`` names the data set that does not fit."""
    from tinygp_amd.kernels.base import Kernel

    Xs = list(Xs)
    nb = len(Xs)
    if nb == 0:
        raise ValueError("a set of data sets needs at least one data set")
    if isinstance(kernels, Kernel):
        kernels = [kernels] * nb
    else:
        kernels = list(kernels)
        if len(kernels) != nb:
            raise ValueError(f"kernels must be one kernel or one per data set ({nb}); got {len(kernels)}")

    def entries(values, what):
        values = list(values)
        if len(values) != nb:
            raise ValueError(f"{what} must hold one entry per data set ({nb}); got {len(values)}")
        return values

    ys, diags = entries(ys, "ys"), entries(diags, "diags")
    means = [None] * nb if means is None else entries(means, "means")
    out, dim = [], None
    for b, X in enumerate(Xs):
        if _device.is_tree(X):
            n, dt = _device.num_points(X), _device.common_dtype(*_device.tree_leaves(X))
        else:
            try:
                P = _device.points(X, limit=False)
            except ValueError as e:
                raise ValueError(f"data set {b}: {e}") from e
            n, dt = P.shape[0], P.dtype
            if n == 0:
                raise ValueError(f"data set {b} is empty: every data set needs at least one data point")
            if dim is None:
                dim = P.shape[1]
            if P.shape[1] != dim:
                raise ValueError(f"data set {b}: its points have {P.shape[1]} input dimensions, the set's have {dim}")

        def vector(v, what, scalar_ok):
            v = np.asarray(v)
            if v.ndim == 2 and v.shape[1] == 1:
                v = v[:, 0]
            if not (v.shape == (n,) or (scalar_ok and v.shape == ())):
                raise ValueError(f"{what}[{b}] must have shape ({n},)" + (" or be a scalar" if scalar_ok else "")
                                 + f" for data set {b}; got {v.shape}")
            return np.broadcast_to(v.astype(dt, copy=False), (n,))

        y = vector(ys[b], "ys", False)
        diag = vector(diags[b], "diags", True)
        mean = None if means[b] is None else vector(means[b], "means", True)
        out.append((kernels[b], X, y, diag, mean))
    return out


def log_probability_datasets(kernels, Xs, ys, *, diags, means=None, return_info: bool = False, ctx=None):
    """The log-probabilities of B data sets under dense GPs, each with points, length and noise of its own, in one call
    (the reference's ``jax.vmap`` over the function that builds the GP, without its equal-length restriction): hundreds
    of short multi-band light curves, the inner loop of Bayesian optimisation.

    ``kernels``: one kernel or one per data set; the members may differ in structure.  ``Xs[b]``: (n_b,) or (n_b, D)
    with one D for the whole set.  ``ys[b]``: (n_b,).  ``diags[b]``: a scalar or (n_b,).  ``means[b]``: ``None``, a
    scalar or (n_b,).  Returns B float64 values in the caller's order; a failed or non-finite member gives ``-inf``.
    With ``return_info`` also the B ``info`` values (0, or the 1-based index of the first non-positive pivot).

    Data sets of up to ``TGP_SMALL_MAX_N`` points that the device can lower run in the batched launches
    (``tgp_small_logprob``: one workgroup per data set, fp64); each is held to the project's 1e-8 bar against
    ``GaussianProcess(kernels[b], Xs[b], diag=diags[b], mean=means[b]).log_probability(ys[b])``, not to its bits.
    Larger ones, and any the device cannot lower (``kernels.Custom``, more than 16 dimensions, pytree inputs), are that
    very call, one by one.  ``kernels.quasisep`` models belong to :func:`tinygp_amd.log_probability_series`."""
    members = check_datasets(kernels, Xs, ys, diags, means)
    reject_quasisep(m[0] for m in members)
    nb = len(members)
    out, info = np.empty(nb), np.zeros(nb, dtype=np.int32)
    batched, where = [], []
    for b, (kernel, X, y, diag, mean) in enumerate(members):
        lowered = lower_member(kernel, X)
        # (an input transform may change the dimension: the launches hold the first batched member's)
        if batched_route(len(y), lowered) and (not batched or lowered[1].shape[1] == batched[0][1].shape[1]):
            batched.append((lowered[0], lowered[1], diag, y if mean is None else y - mean))
            where.append(b)
        else:
            out[b], info[b] = _single(kernel, X, y, diag, mean, ctx)
    if batched:
        packed = pack_members(batched, labels=[f"data set {b}" for b in where])
        values, infos = run_packed(_ffi.default_ctx() if ctx is None else ctx, packed)
        out[where], info[where] = values, infos
    out[(info != 0) | ~np.isfinite(out)] = -np.inf
    return (out, info) if return_info else out


def log_probability_and_grad_datasets(kernels, Xs, ys, *, diags, means=None, vectors: bool = True,
                                      return_info: bool = False, ctx=None):
    """:func:`log_probability_datasets` with the gradients: ``(values (B,) float64, grads)`` of B data sets under dense
    GPs, each with points, length and noise of its own, in one call (the reference's ``jax.vmap`` over
    ``jax.value_and_grad`` of the function that builds the GP): the restarts of an optimiser, populations of HMC
    chains, many short light curves fitted at once.  Arguments as in :func:`log_probability_datasets`.

    ``grads`` has the keys of ``GaussianProcess.log_probability_and_grad``: ``"kernel"``, a list of B float64 arrays,
    member b's in the order of ``kernels[b].parameters()`` (the members may differ in structure); ``"noise_diag"`` and
    ``"mean"``, lists of (n_b,) arrays in the dtype of that data set's coordinates, or ``None`` with
    ``vectors=False`` (they are then not copied back); ``"transform"``, a list of B entries, each ``None`` or the
    gradient with respect to the ``scale`` / ``factor`` of the one ``transforms.Linear`` / ``Cholesky`` that covers the
    member's kernel.  A failed or non-finite member gives ``-inf`` and NaN gradients.  With ``return_info`` the B
    ``info`` values come third.

    Data sets of up to ``TGP_SMALL_MAX_N`` points that the device can lower run in the batched launches
    (``tgp_small_logprob_grad``: one workgroup per data set, fp64; the value has the bits of
    :func:`log_probability_datasets`); each is held to the project's bars against
    ``GaussianProcess(kernels[b], Xs[b], diag=diags[b], mean=means[b]).log_probability_and_grad(ys[b])``.  Larger ones,
    and any the device cannot lower, are that very call, one by one, repacked into the same shape (with its own answers:
    it raises ``NotImplementedError`` for a kernel without a device program, such as ``kernels.Custom``)."""
    members = check_datasets(kernels, Xs, ys, diags, means)
    reject_quasisep(m[0] for m in members)
    nb = len(members)
    ks = [m[0] for m in members]
    values, info = np.empty(nb), np.zeros(nb, dtype=np.int32)
    kgrads, tgrads, noise_rows, mean_rows = [None] * nb, [None] * nb, [None] * nb, [None] * nb
    batched, where = [], []
    for b, (kernel, X, y, diag, mean) in enumerate(members):
        lowered = lower_member(kernel, X)
        if batched_route(len(y), lowered) and (not batched or lowered[1].shape[1] == batched[0][1].shape[1]):
            batched.append((lowered[0], lowered[1], diag, y if mean is None else y - mean))
            where.append(b)
        else:
            values[b], info[b], kgrads[b], tgrads[b], noise_rows[b], mean_rows[b] = _single_grad(kernel, X, y, diag,
                                                                                                  mean, ctx, vectors)
    if batched:
        packed = pack_members(batched, labels=[f"data set {b}" for b in where])
        results = run_packed_grad(_ffi.default_ctx() if ctx is None else ctx, packed, dims_flags(ks[b] for b in where),
                                  vectors=vectors)
        unpack_gradients(ks, packed, results, where, values, info, kgrads, tgrads, noise_rows, mean_rows,
                         [members[b][2].dtype for b in where])  # (the vectors in the dtype of each data set)
    values[(info != 0) | ~np.isfinite(values)] = -np.inf
    grads = {"kernel": kgrads, "noise_diag": noise_rows if vectors else None, "mean": mean_rows if vectors else None,
             "transform": tgrads}
    return (values, grads, info) if return_info else (values, grads)


# ---- predictions ------------------------------------------------------------------------------------------------------
class PackedPredict(NamedTuple):
    """The host arrays of one ``tgp_small_predict`` call beside those of ``tgp_small_logprob``."""

    packed: Packed
    Xt: np.ndarray             # (test rows, d) float64
    xt_off: np.ndarray         # (B,) int64, rows into Xt
    m: np.ndarray              # (B,) int32
    pred_progs: np.ndarray | None     # (total second ops,) KOP_DTYPE, or None: every member predicts with its own
    pred_prog_off: np.ndarray | None  # (B + 1,) int32; an empty extent: the member's own program
    out_off: np.ndarray        # (B,) int64, into the means and variances


def pack_predict(members, tests, pred_progs=None, labels=None) -> PackedPredict:
    """:func:`pack_members` of ``members`` plus their test points: ``tests[b]`` is (m_b, D) float64, m_b = 0 allowed.
    Test points ``np.array_equal`` to the first member's share its rows of ``Xt`` (one uploaded copy: a shared grid of
    candidates); ``pred_progs[b]``: ``None`` or the postfix program of k* and k**.  The outputs of member b start at
    ``out_off[b] = m_0 + .. + m_{b-1}``.  A ``ValueError`` names the member whose test points do not fit."""
    members = list(members)
    packed = pack_members(members, labels)
    labels = [f"member {b}" for b in range(len(members))] if labels is None else list(labels)
    tests = list(tests)
    if len(tests) != len(members):
        raise ValueError(f"tests must hold one entry per member ({len(members)}); got {len(tests)}")
    xt_off, ms, out_off, Xts = [], [], [], []
    rows = total = 0
    T0 = None
    for b, T in enumerate(tests):
        T = np.asarray(T, dtype=np.float64)
        if T.ndim != 2 or T.shape[1] != packed.d:
            raise ValueError(f"{labels[b]}: its test points must have shape (m, {packed.d}) like its points; got {T.shape}")
        if b == 0:
            T0 = T
        if b > 0 and T.shape == T0.shape and np.array_equal(T, T0):
            xt_off.append(0)
        else:
            xt_off.append(rows)
            Xts.append(T)
            rows += T.shape[0]
        ms.append(T.shape[0])
        out_off.append(total)
        total += T.shape[0]
    pp = ppo = None
    if pred_progs is not None and any(q is not None for q in pred_progs):
        pred_progs = list(pred_progs)
        if len(pred_progs) != len(members):
            raise ValueError(f"pred_progs must hold one entry per member ({len(members)}); got {len(pred_progs)}")
        ops, ppo = [], [0]
        for b, prog in enumerate(pred_progs):
            if prog is not None:
                if not 1 <= len(prog) <= 32:
                    raise ValueError(f"{labels[b]}: a kernel program holds 1 .. 32 operations (got {len(prog)})")
                ops.extend((int(op), int(metric), float(p0), float(p1)) for op, metric, p0, p1 in prog)
            ppo.append(len(ops))
        pp, ppo = np.array(ops, dtype=KOP_DTYPE), np.array(ppo, dtype=np.int32)
    Xt = np.concatenate(Xts, axis=0) if Xts else np.empty((0, packed.d))
    return PackedPredict(packed, np.ascontiguousarray(Xt.reshape(-1, packed.d)), np.array(xt_off, dtype=np.int64),
                         np.array(ms, dtype=np.int32), pp, ppo, np.array(out_off, dtype=np.int64))


def predict_rows(m: int, chunk: int = PRED_CHUNK):
    """The table rows ``tgp_small_predict`` makes of a member with m test points: ``[(first point, points)]``, one per
    workgroup, each at most ``chunk`` points; every row factors the member again, the first alone writes the value.
    m = 0 is one row without points."""
    if m <= 0:
        return [(0, 0)]
    return [(at, min(chunk, m - at)) for at in range(0, m, chunk)]


def predict_launch_bytes(pp: PackedPredict, var: bool = True) -> int:
    """The staging bytes of ``pp`` as ONE launch (``pred_launch_bytes`` of small.hip): table rows of 64 bytes, the
    programs (``KPROG_BYTES`` each) with the second ones behind the members', coordinates, noise, residual, test points,
    values, info, means and variances.  The C side ends a launch before the member that would take this past
    ``STAGE_BYTES``."""
    nb, d = len(pp.packed.n), pp.packed.d
    rows = sum(len(predict_rows(int(m))) for m in pp.m)
    second = 0 if pp.pred_prog_off is None else int(np.count_nonzero(np.diff(pp.pred_prog_off)))
    # coordinates and test points are staged once per (offset, count)
    x_doubles = sum(n * d for _, n in {(int(o), int(n)) for o, n in zip(pp.packed.x_off, pp.packed.n)})
    xt_doubles = sum(m * d for _, m in {(int(o), int(m)) for o, m in zip(pp.xt_off, pp.m) if m > 0})
    vec, outs = int(pp.packed.n.sum()), int(pp.m.sum())
    return (rows * 64 + (nb + second) * _ffi.KPROG_BYTES + (x_doubles + 2 * vec + xt_doubles) * 8 + nb * 8
            + -(-nb * 4 // 8) * 8 + outs * (16 if var else 8))


def run_packed_predict(ctx, pp: PackedPredict, return_var: bool = True):
    """One ``tgp_small_predict`` call: ``(values (B,), info (B,) int32, means (sum m,), variances (sum m,) or None)``,
    float64; member b's predictions sit at ``pp.out_off[b]``.  The variances are ``k** - |L^-1 k*|^2``: no jitter.  A
    failed member has NaN in its value and predictions."""
    packed = pp.packed
    nb, total = len(packed.n), int(pp.m.sum())
    info, out = np.zeros(nb, dtype=np.int32), np.empty(nb)
    mean = np.empty(max(total, 1))
    var = np.empty(max(total, 1)) if return_var else None
    _ffi.check(_ffi.lib().tgp_small_predict(
        ctx.handle, nb, _ffi.ptr(packed.progs), packed.prog_off.ctypes.data_as(_ffi._pi32),
        packed.x_off.ctypes.data_as(_ffi._pi64), packed.n.ctypes.data_as(_ffi._pi32), packed.d, _ffi.ptr(packed.X),
        packed.X.shape[0], packed.vec_off.ctypes.data_as(_ffi._pi64), _ffi.ptr(packed.noise), _ffi.ptr(packed.resid),
        _ffi.ptr(pp.Xt) if pp.Xt.shape[0] else None, pp.Xt.shape[0], pp.xt_off.ctypes.data_as(_ffi._pi64),
        pp.m.ctypes.data_as(_ffi._pi32), None if pp.pred_progs is None else _ffi.ptr(pp.pred_progs),
        None if pp.pred_prog_off is None else pp.pred_prog_off.ctypes.data_as(_ffi._pi32),
        pp.out_off.ctypes.data_as(_ffi._pi64), info.ctypes.data_as(_ffi._pi32), out.ctypes.data_as(_ffi._pdbl),
        mean.ctypes.data_as(_ffi._pdbl), None if var is None else var.ctypes.data_as(_ffi._pdbl)), "tgp_small_predict")
    return out, info, mean[:total], None if var is None else var[:total]


def lower_test(kernel, predict_kernel, X, X_test, lowered):
    """``(test points (m, D) float64, second program or None)`` of a batched member, or ``None`` when it has to take the
    single path: the prediction kernel has no device program, or lowers the data points differently from the model
    kernel (another input transform), or the test points do not lower to the member's dimension."""
    pk = kernel if predict_kernel is None else predict_kernel
    try:
        if predict_kernel is not None:
            low = lower_member(predict_kernel, X)
            if low is None or low[1].shape != lowered[1].shape or not np.array_equal(low[1], lowered[1]):
                return None
        if X_test is None:
            return lowered[1], (None if predict_kernel is None else low[0])
        if _device.is_tree(X_test):
            return None
        Xt = pk._lower(X_test)[1]
        if _device.is_tree(Xt):
            return None
        Pt = _device.points(Xt, np.float64)
    except NotImplementedError:
        return None
    if Pt.shape[1] != lowered[1].shape[1]:
        return None
    return Pt, (None if predict_kernel is None else low[0])


def jitter(dtype):
    """What ``GaussianProcess.condition`` adds to the diagonal of a conditional covariance by default: sqrt(eps) of the
    data's dtype (``gp._default_diag``)."""
    return np.sqrt(np.finfo(np.dtype(dtype)).eps)


def added_means(members, raw_means, X_tests, test_means, include_mean):
    """What ``include_mean`` adds to member b's predictions, a list of (m_b,) float64 arrays: a scalar ``means[b]``
    itself; for a vector ``means[b]`` -- it enters the residual only -- ``test_means[b]``, a scalar or (m_b,), which
    ``include_mean`` then requires.  A ``ValueError`` names the data set."""
    added = [None] * len(members)
    for b, (kernel, X, y, diag, mean) in enumerate(members):
        m = len(y) if X_tests[b] is None else _device.num_points(X_tests[b])
        if mean is None or np.ndim(raw_means[b]) == 0:
            if test_means[b] is not None:
                raise ValueError(f"test_means[{b}] is given, but means[{b}] of data set {b} is not a vector: a scalar "
                                 "mean is added to the predictions by itself")
            added[b] = np.zeros(m) if mean is None else np.full(m, np.asarray(raw_means[b], dtype=np.float64))
        else:
            if test_means[b] is None:
                if include_mean:
                    raise ValueError(f"means[{b}] of data set {b} is a vector: the mean at its test points must be given "
                                     f"as test_means[{b}] (a scalar or ({m},)), or include_mean=False")
                added[b] = np.zeros(m)
            else:
                t = np.asarray(test_means[b], dtype=np.float64)
                if t.shape not in ((), (m,)):
                    raise ValueError(f"test_means[{b}] must have shape ({m},) or be a scalar for data set {b}; got {t.shape}")
                added[b] = np.broadcast_to(t, (m,))
    return added


def predict_datasets(kernels, Xs, ys, X_tests, *, diags, means=None, test_means=None, predict_kernels=None,
                     return_var: bool = True, include_mean: bool = True, return_info: bool = False, ctx=None):
    """Condition B dense GPs on their data and predict at test points, each with points, length, noise and test points
    of its own, in one call (the reference's ``jax.vmap`` over the function that builds the GP and calls ``predict``):
    the acquisition step of Bayesian optimisation, hundreds of short light curves interpolated after the fit, restarts
    compared on held-out points.

    Arguments as in :func:`log_probability_datasets`, and ``X_tests[b]``: (m_b,) or (m_b, D), m_b = 0 allowed, or
    ``None`` for the data set's own points (they are sent as test points: the mean is K alpha).  ``means[b]``: a
    scalar is added to the predicted mean when ``include_mean``; a vector (n_b,) enters the residual only and needs
    ``test_means[b]``, a scalar or (m_b,), which is then what ``include_mean`` adds.  ``predict_kernels[b]``: ``None``
    or the kernel of k* and k** (``predict(kernel=k1)``: the contribution of one term of a sum).

    Returns ``(values (B,) float64, means, variances)``: lists of B arrays (m_b,) in the dtype of that data set's
    coordinates, ``variances`` ``None`` without ``return_var`` (the triangular solve is then skipped); with
    ``return_info`` the B ``info`` values come fourth.  A failed or non-finite member gives ``-inf`` and NaN
    predictions.

    Member b is ``GaussianProcess(kernels[b], Xs[b], diag=diags[b], mean=means[b]).predict(ys[b], X_tests[b],
    kernel=predict_kernels[b], return_var=True)``, the default jitter of ``condition`` included in the variances, held
    to the project's posterior bar against that call.  Data sets of up to ``TGP_SMALL_MAX_N`` points that the device
    can lower run in the batched launches (``tgp_small_predict``: one workgroup per data set and per
    ``TGP_SMALL_PRED_CHUNK`` test points, fp64; the value has the bits of :func:`log_probability_datasets`, and a
    prediction's bits depend on its data set and its own test point alone).  Larger ones, any the device cannot lower
    (``kernels.Custom``, more than 16 dimensions, pytree inputs) and a ``predict_kernels[b]`` under another input
    transform than the model's are that very call, one by one.  ``kernels.quasisep`` models belong to
    ``QuasisepSolver``."""
    members = check_datasets(kernels, Xs, ys, diags, means)
    nb = len(members)

    def entries(values, what):
        values = [None] * nb if values is None else list(values)
        if len(values) != nb:
            raise ValueError(f"{what} must hold one entry per data set ({nb}); got {len(values)}")
        return values

    X_tests, test_means = entries(X_tests, "X_tests"), entries(test_means, "test_means")
    predict_kernels, raw_means = entries(predict_kernels, "predict_kernels"), entries(means, "means")
    reject_quasisep(m[0] for m in members)
    reject_quasisep(k for k in predict_kernels if k is not None)
    values, info = np.empty(nb), np.zeros(nb, dtype=np.int32)
    out_means, out_vars = [None] * nb, [None] * nb
    added = added_means(members, raw_means, X_tests, test_means, include_mean)
    batched, tests, seconds, where = [], [], [], []
    for b, (kernel, X, y, diag, mean) in enumerate(members):
        lowered = lower_member(kernel, X)
        test = None
        if batched_route(len(y), lowered) and (not batched or lowered[1].shape[1] == batched[0][1].shape[1]):
            test = lower_test(kernel, predict_kernels[b], X, X_tests[b], lowered)
        if test is not None:
            batched.append((lowered[0], lowered[1], diag, y if mean is None else y - mean))
            tests.append(test[0])
            seconds.append(test[1])
            where.append(b)
        else:
            values[b], info[b], out_means[b], out_vars[b] = _single_predict(
                kernel, X, y, diag, mean, X_tests[b], predict_kernels[b], return_var, ctx)
    if batched:
        pp = pack_predict(batched, tests, seconds, labels=[f"data set {b}" for b in where])
        vals, infos, mu, var = run_packed_predict(_ffi.default_ctx() if ctx is None else ctx, pp, return_var)
        for k, b in enumerate(where):
            at, m = int(pp.out_off[k]), int(pp.m[k])
            values[b], info[b] = vals[k], infos[k]
            out_means[b] = mu[at:at + m]
            if return_var:
                out_vars[b] = var[at:at + m] + jitter(members[b][2].dtype)
    bad = (info != 0) | ~np.isfinite(values)
    values[bad] = -np.inf
    for b in range(nb):
        dt = members[b][2].dtype
        mu = np.asarray(out_means[b], dtype=np.float64)
        mu = mu + added[b] if include_mean else mu
        out_means[b] = np.full(len(mu), np.nan, dtype=dt) if bad[b] else mu.astype(dt)
        if return_var:
            v = np.asarray(out_vars[b], dtype=np.float64)
            out_vars[b] = np.full(len(v), np.nan, dtype=dt) if bad[b] else v.astype(dt)
    out = (values, out_means, out_vars if return_var else None)
    return out + (info,) if return_info else out


def _single_predict(kernel, X, y, diag, mean, X_test, predict_kernel, return_var, ctx):
    """One data set on the single dense path: ``GaussianProcess(kernel, X, diag=diag).predict(y - mean, X_test,
    kernel=predict_kernel, return_var=True)`` itself -- the mean enters through the residual, the caller adds it to the
    predictions -- its solver closed behind it: ``(value, info, means, variances or None)``."""
    from tinygp_amd.gp import GaussianProcess
    from tinygp_amd.solvers.direct import DirectSolver

    kwargs = {} if ctx is None else {"ctx": ctx}
    gp = GaussianProcess(kernel, X, diag=diag, solver=DirectSolver, **({} if mean is None else {"mean_value": mean}),
                         **kwargs)
    try:
        value, cond = gp.condition(y, X if X_test is None else X_test, kernel=predict_kernel, include_mean=False)
        var = np.asarray(cond.variance) if return_var else None
        return float(value), int(gp.solver.info), np.asarray(cond.loc), var
    finally:
        gp.solver.close()


# ---- conditional covariance and joint draws ----------------------------------------------------------------------------
class PackedCondition(NamedTuple):
    """The host arrays of one ``tgp_small_condition`` call beside those of ``tgp_small_predict`` (``pp.out_off`` is where
    a member's means go, and its test diagonal comes from)."""

    pp: PackedPredict
    tdiag: np.ndarray    # (sum m,) float64, member b's at pp.out_off[b]
    cov_off: np.ndarray  # (B,) int64, into the covariances: m_0^2 + .. + m_{b-1}^2
    ndraw: np.ndarray    # (B,) int32, the draws S_b
    xi: np.ndarray       # (sum S m,) float64, member b's (S_b, m_b) draw-major at xi_off[b]
    xi_off: np.ndarray   # (B,) int64, into the normals and the samples


def condition_route(n: int, m: int, lowered) -> bool:
    """Whether a member of ``n`` points and ``m`` test points goes into the conditioning launches: the test points ride
    as columns of the member's matrix, so the cap of :func:`batched_route` holds for n + m."""
    return batched_route(n, lowered) and n + m <= MAX_N


def pack_condition(members, tests, tdiags, pred_progs=None, xis=None, labels=None) -> PackedCondition:
    """:func:`pack_predict` of ``members`` and ``tests`` plus ``tdiags[b]``, the (m_b,) values added to the diagonal
    of member b's conditional covariance, and ``xis[b]``, ``None`` or its (S_b, m_b) standard normals.  A
    ``ValueError`` names the member whose vectors do not fit or whose n + m is above the cap."""
    pp = pack_predict(members, tests, pred_progs, labels)
    nb = len(pp.m)
    labels = [f"member {b}" for b in range(nb)] if labels is None else list(labels)
    tdiags = list(tdiags)
    xis = [None] * nb if xis is None else list(xis)
    if len(tdiags) != nb or len(xis) != nb:
        raise ValueError(f"tdiags and xis must hold one entry per member ({nb}); got {len(tdiags)} and {len(xis)}")
    tds, zs, ndraw, xi_off = [], [], [], []
    total = 0
    for b in range(nb):
        n, m = int(pp.packed.n[b]), int(pp.m[b])
        if n + m > MAX_N:
            raise ValueError(f"{labels[b]}: the conditioning launches hold at most {MAX_N} data and test points per "
                             f"member (got {n} + {m})")
        t = np.asarray(tdiags[b], dtype=np.float64)
        if t.shape != (m,):
            raise ValueError(f"{labels[b]}: its test diagonal must have shape ({m},); got {t.shape}")
        tds.append(t)
        z = np.empty((0, m)) if xis[b] is None else np.asarray(xis[b], dtype=np.float64)
        if z.ndim != 2 or z.shape[1] != m:
            raise ValueError(f"{labels[b]}: its normals must have shape (S, {m}); got {z.shape}")
        ndraw.append(z.shape[0])
        xi_off.append(total)
        zs.append(z.reshape(-1))
        total += z.size
    cov_off = np.concatenate([[0], np.cumsum(pp.m.astype(np.int64) ** 2)[:-1]]).astype(np.int64)
    return PackedCondition(pp, np.concatenate(tds), cov_off, np.array(ndraw, dtype=np.int32), np.concatenate(zs),
                           np.array(xi_off, dtype=np.int64))


def condition_launch_bytes(pc: PackedCondition, cov: bool = True) -> int:
    """The staging bytes of ``pc`` as ONE launch (``cond_launch_bytes`` of small.hip): table rows of 80 bytes, one per
    member, the programs (``KPROG_BYTES`` each) with the second ones behind the members', coordinates, noise, residual,
    test points, test diagonal, normals, values, info, cond_info, means, covariances (when asked) and samples.  The C
    side ends a launch before the member that would take this past ``STAGE_BYTES``."""
    pp = pc.pp
    nb, d = len(pp.packed.n), pp.packed.d
    second = 0 if pp.pred_prog_off is None else int(np.count_nonzero(np.diff(pp.pred_prog_off)))
    x_doubles = sum(n * d for _, n in {(int(o), int(n)) for o, n in zip(pp.packed.x_off, pp.packed.n)})
    xt_doubles = sum(m * d for _, m in {(int(o), int(m)) for o, m in zip(pp.xt_off, pp.m) if m > 0})
    vec, outs = int(pp.packed.n.sum()), int(pp.m.sum())
    covs = int((pp.m.astype(np.int64) ** 2).sum()) if cov else 0
    draws = int((pc.ndraw.astype(np.int64) * pp.m).sum())
    return (nb * 80 + (nb + second) * _ffi.KPROG_BYTES + (x_doubles + 2 * vec + xt_doubles + 2 * outs + covs + 2 * draws) * 8
            + nb * 8 + 2 * (-(-nb * 4 // 8) * 8))


def run_packed_condition(ctx, pc: PackedCondition, return_cov: bool = True):
    """One ``tgp_small_condition`` call: ``(values (B,), info (B,) int32, cond_info (B,) int32, means (sum m,),
    covariances (sum m^2,) or None, samples (sum S m,))``, float64; member b's sit at ``pc.pp.out_off[b]``,
    ``pc.cov_off[b]`` and ``pc.xi_off[b]``.  Without ``return_cov`` no covariance is written or copied.  A member with
    ``info != 0`` has NaN everywhere, one with ``cond_info != 0`` NaN draws only."""
    pp, packed = pc.pp, pc.pp.packed
    nb, total = len(packed.n), int(pp.m.sum())
    info, cinfo, out = np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32), np.empty(nb)
    mean = np.empty(max(total, 1))
    ncov = int((pp.m.astype(np.int64) ** 2).sum())
    cov = np.empty(max(ncov, 1)) if return_cov else None
    draws = bool(pc.ndraw.any())
    xi = np.ascontiguousarray(pc.xi) if pc.xi.size else np.zeros(1)
    samples = np.empty(max(pc.xi.size, 1)) if draws else None
    tdiag = pc.tdiag if pc.tdiag.size else np.zeros(1)
    _ffi.check(_ffi.lib().tgp_small_condition(
        ctx.handle, nb, _ffi.ptr(packed.progs), packed.prog_off.ctypes.data_as(_ffi._pi32),
        packed.x_off.ctypes.data_as(_ffi._pi64), packed.n.ctypes.data_as(_ffi._pi32), packed.d, _ffi.ptr(packed.X),
        packed.X.shape[0], packed.vec_off.ctypes.data_as(_ffi._pi64), _ffi.ptr(packed.noise), _ffi.ptr(packed.resid),
        _ffi.ptr(pp.Xt) if pp.Xt.shape[0] else None, pp.Xt.shape[0], pp.xt_off.ctypes.data_as(_ffi._pi64),
        pp.m.ctypes.data_as(_ffi._pi32), None if pp.pred_progs is None else _ffi.ptr(pp.pred_progs),
        None if pp.pred_prog_off is None else pp.pred_prog_off.ctypes.data_as(_ffi._pi32), _ffi.ptr(tdiag),
        pp.out_off.ctypes.data_as(_ffi._pi64), pp.out_off.ctypes.data_as(_ffi._pi64), mean.ctypes.data_as(_ffi._pdbl),
        pc.cov_off.ctypes.data_as(_ffi._pi64) if return_cov else None,
        cov.ctypes.data_as(_ffi._pdbl) if return_cov else None, pc.ndraw.ctypes.data_as(_ffi._pi32),
        _ffi.ptr(xi) if draws else None, pc.xi_off.ctypes.data_as(_ffi._pi64),
        samples.ctypes.data_as(_ffi._pdbl) if draws else None, info.ctypes.data_as(_ffi._pi32),
        cinfo.ctypes.data_as(_ffi._pi32), out.ctypes.data_as(_ffi._pdbl)), "tgp_small_condition")
    return (out, info, cinfo, mean[:total], None if cov is None else cov[:ncov],
            samples[:pc.xi.size] if draws else np.empty(0))


def host_draws(loc, cov, xi):
    """``(loc + L xi_s for every row s of xi (S, m), cond_info)`` with L from LAPACK's ``dpotrf`` of ``cov`` on the
    host: the draws of a member on the single path.  ``cond_info``: 0, or the 1-based order of the first leading minor
    that is not positive definite; the draws are then NaN."""
    from scipy.linalg import lapack

    xi = np.asarray(xi, dtype=np.float64)
    if xi.shape[1] == 0 or xi.shape[0] == 0:
        return np.empty(xi.shape), 0
    cov = np.asarray(cov, dtype=np.float64)
    if not np.all(np.isfinite(cov)):
        return np.full(xi.shape, np.nan), 0
    L, bad = lapack.dpotrf(cov, lower=1, clean=1)
    if bad != 0:
        return np.full(xi.shape, np.nan), int(bad)
    return np.asarray(loc, dtype=np.float64) + xi @ L.T, 0


def _single_condition(kernel, X, y, diag, mean, X_test, test_diag, predict_kernel, xi, ctx):
    """One data set on the single dense path: ``GaussianProcess(kernel, X, diag=diag).condition(y - mean, X_test,
    diag=test_diag, kernel=predict_kernel)`` itself -- the mean enters through the residual, the caller adds it -- its
    solver closed behind it: ``(value, info, cond_info, means, covariance, draws (S, m) or None)``; the draws are
    :func:`host_draws` of that call's own mean and covariance."""
    from tinygp_amd.gp import GaussianProcess
    from tinygp_amd.solvers.direct import DirectSolver

    kwargs = {} if ctx is None else {"ctx": ctx}
    gp = GaussianProcess(kernel, X, diag=diag, solver=DirectSolver, **({} if mean is None else {"mean_value": mean}),
                         **kwargs)
    try:
        value, cond = gp.condition(y, X if X_test is None else X_test, diag=test_diag, kernel=predict_kernel,
                                   include_mean=False)
        loc = np.asarray(cond.loc)
        cov = np.asarray(cond.covariance) if len(loc) else np.empty((0, 0), dtype=loc.dtype)
        draws, cinfo = (None, 0) if xi is None else host_draws(loc, cov, xi)
        return float(value), int(gp.solver.info), cinfo, loc, cov, draws
    finally:
        gp.solver.close()


def _condition_sets(kernels, Xs, ys, X_tests, diags, means, test_means, test_diags, predict_kernels, include_mean,
                    xis, want_cov, ctx):
    """The body of :func:`condition_datasets` and :func:`sample_conditional_datasets`: ``(values, info, cond_info,
    means, covariances or None, draws or None)``; ``xis``: ``None`` or a callable ``(b, m_b) -> (S, m_b)`` asked
    member by member in the caller's order."""
    members = check_datasets(kernels, Xs, ys, diags, means)
    nb = len(members)

    def entries(values, what):
        values = [None] * nb if values is None else list(values)
        if len(values) != nb:
            raise ValueError(f"{what} must hold one entry per data set ({nb}); got {len(values)}")
        return values

    X_tests, test_means = entries(X_tests, "X_tests"), entries(test_means, "test_means")
    predict_kernels, raw_means = entries(predict_kernels, "predict_kernels"), entries(means, "means")
    test_diags = entries(test_diags, "test_diags")
    reject_quasisep(m[0] for m in members)
    reject_quasisep(k for k in predict_kernels if k is not None)
    added = added_means(members, raw_means, X_tests, test_means, include_mean)
    taus, draws_in = [None] * nb, [None] * nb
    for b, (kernel, X, y, diag, mean) in enumerate(members):
        m = len(added[b])
        t = np.asarray(jitter(y.dtype) if test_diags[b] is None else test_diags[b], dtype=np.float64)
        if t.shape not in ((), (m,)):
            raise ValueError(f"test_diags[{b}] must have shape ({m},) or be a scalar for data set {b}; got {t.shape}")
        taus[b] = np.broadcast_to(t.astype(y.dtype).astype(np.float64), (m,))  # (rounded as condition(diag=) rounds it)
        if xis is not None:
            z = np.asarray(xis(b, m), dtype=np.float64)
            if z.ndim != 2 or z.shape[1] != m:
                raise ValueError(f"xi[{b}] must have shape (R, {m}) for data set {b}; got {z.shape}")
            draws_in[b] = z
    values, info, cinfo = np.empty(nb), np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32)
    out_means, out_covs, out_draws = [None] * nb, [None] * nb, [None] * nb
    batched, tests, seconds, where = [], [], [], []
    for b, (kernel, X, y, diag, mean) in enumerate(members):
        lowered = lower_member(kernel, X)
        test = None
        if condition_route(len(y), len(added[b]), lowered) and (not batched
                                                               or lowered[1].shape[1] == batched[0][1].shape[1]):
            test = lower_test(kernel, predict_kernels[b], X, X_tests[b], lowered)
        if test is not None:
            batched.append((lowered[0], lowered[1], diag, y if mean is None else y - mean))
            tests.append(test[0])
            seconds.append(test[1])
            where.append(b)
        else:
            (values[b], info[b], cinfo[b], out_means[b], out_covs[b],
             out_draws[b]) = _single_condition(kernel, X, y, diag, mean, X_tests[b], taus[b], predict_kernels[b],
                                               draws_in[b], ctx)
    if batched:
        pc = pack_condition(batched, tests, [taus[b] for b in where], seconds, [draws_in[b] for b in where],
                            labels=[f"data set {b}" for b in where])
        vals, infos, cinfos, mu, cov, smp = run_packed_condition(_ffi.default_ctx() if ctx is None else ctx, pc,
                                                                 want_cov)
        for k, b in enumerate(where):
            at, m, s = int(pc.pp.out_off[k]), int(pc.pp.m[k]), int(pc.ndraw[k])
            values[b], info[b], cinfo[b] = vals[k], infos[k], cinfos[k]
            out_means[b] = mu[at:at + m]
            if want_cov:
                out_covs[b] = cov[int(pc.cov_off[k]):int(pc.cov_off[k]) + m * m].reshape(m, m)
            if xis is not None:
                out_draws[b] = smp[int(pc.xi_off[k]):int(pc.xi_off[k]) + s * m].reshape(s, m)
    bad = (info != 0) | ~np.isfinite(values)
    values[bad] = -np.inf
    for b in range(nb):
        dt = members[b][2].dtype
        shift = added[b] if include_mean else 0.0
        mu = np.asarray(out_means[b], dtype=np.float64) + shift
        out_means[b] = np.full(len(mu), np.nan, dtype=dt) if bad[b] else mu.astype(dt)
        if want_cov:
            c = np.asarray(out_covs[b], dtype=np.float64)
            out_covs[b] = np.full(c.shape, np.nan, dtype=dt) if bad[b] else c.astype(dt)
        if xis is not None:
            f = np.asarray(out_draws[b], dtype=np.float64) + shift
            out_draws[b] = np.full(f.shape, np.nan, dtype=dt) if bad[b] else f.astype(dt)
    return values, info, cinfo, out_means, (out_covs if want_cov else None), (out_draws if xis is not None else None)


def condition_datasets(kernels, Xs, ys, X_tests, *, diags, means=None, test_means=None, test_diags=None,
                       predict_kernels=None, include_mean: bool = True, return_info: bool = False, ctx=None):
    """Condition B dense GPs on their data and return the JOINT posterior at test points, each with points, length,
    noise and test points of its own, in one call (the reference's ``jax.vmap`` over the function that builds the GP
    and reads ``condition(y, X_test).gp``): batch acquisition in Bayesian optimisation, restarts compared on held-out
    points with their correlations.

    Arguments as in :func:`predict_datasets`, and ``test_diags[b]``: ``None``, a scalar or (m_b,), what is added to
    the diagonal of the covariance; ``None`` is the default jitter of ``condition``, :func:`jitter` of the data set's
    dtype.

    Returns ``(values (B,) float64, means, covariances)``: lists of B arrays (m_b,) and (m_b, m_b) in the dtype of
    that data set's coordinates, each covariance exactly symmetric; with ``return_info`` the B ``info`` values come
    fourth.  A failed or non-finite member gives ``-inf`` and NaN everywhere.

    Member b is ``GaussianProcess(kernels[b], Xs[b], diag=diags[b], mean=means[b]).condition(ys[b], X_tests[b],
    diag=test_diags[b], kernel=predict_kernels[b])``: its ``log_probability``, ``gp.loc`` and ``gp.covariance``, held
    to the project's posterior bar against that call.  Data sets whose data and test points TOGETHER number at most
    ``TGP_SMALL_MAX_N`` and that the device can lower run in the batched launches (``tgp_small_condition``: one
    workgroup per data set, fp64, the test points as further columns of the one elimination; the value has the bits of
    :func:`log_probability_datasets`, and a member's outputs depend on its own data alone).  Larger ones, any the
    device cannot lower (``kernels.Custom``, more than 16 dimensions, pytree inputs) and a ``predict_kernels[b]`` under
    another input transform than the model's are that very call, one by one.  ``kernels.quasisep`` models belong to
    ``QuasisepSolver``."""
    values, info, _, mu, cov, _ = _condition_sets(kernels, Xs, ys, X_tests, diags, means, test_means, test_diags,
                                                  predict_kernels, include_mean, None, True, ctx)
    return (values, mu, cov, info) if return_info else (values, mu, cov)


def sample_conditional_datasets(kernels, Xs, ys, X_tests, *, key, shape=None, diags, means=None, test_means=None,
                                test_diags=None, predict_kernels=None, include_mean: bool = True, xi=None,
                                return_info: bool = False, ctx=None):
    """Joint posterior draws of B dense GPs at test points of their own, in one call: what
    ``condition(ys[b], X_tests[b], diag=test_diags[b]).gp.sample(key, shape)`` draws from for every member (Thompson
    sampling over a candidate set, posterior draws of many short light curves after a fit).  Arguments as in
    :func:`condition_datasets`.

    ``key``: an int seed or a ``numpy.random.Generator``, as in ``GaussianProcess.sample``; member b's normals are
    ``rng.standard_normal((R, m_b))`` with R the product of ``shape``, drawn in member order.  ``xi``: a list of
    (R, m_b) arrays that replaces the draw (``key`` is then not used).  Returns ``(values (B,), samples)`` with
    ``samples[b]`` of shape ``shape + (m_b,)`` in that data set's dtype: ``mean + L xi_s`` with L the Cholesky factor
    of the conditional covariance, ``test_diags[b]`` included.  With ``return_info``, ``(info, cond_info)`` follow:
    ``cond_info[b]`` is 0, or the 1-based index of the first pivot of that factorisation that is not > 0 -- member b's
    draws are then NaN, its value stands.  A failed data block (``info != 0``) gives ``-inf`` and NaN draws.

    The routing is that of :func:`condition_datasets`; no covariance crosses the bus.  On the single path the draws are
    that call's ``gp.loc + L xi_s`` with L from LAPACK on the host (:func:`host_draws`).  A draw's bits depend on its
    data set and its own normals alone."""
    shape = () if shape is None else tuple(shape)
    R = int(np.prod(shape, dtype=np.int64))
    if xi is None:
        rng = key if isinstance(key, np.random.Generator) else np.random.default_rng(key)

        def normals(b, m):
            return rng.standard_normal((R, m))
    else:
        xi = list(xi)

        def normals(b, m):
            if b >= len(xi):
                raise ValueError(f"xi must hold one entry per data set; got {len(xi)}")
            z = np.asarray(xi[b])
            if z.shape != (R, m):
                raise ValueError(f"xi[{b}] must have shape ({R}, {m}) for data set {b}: R is the product of shape "
                                 f"{shape}; got {z.shape}")
            return z

    values, info, cinfo, _, _, draws = _condition_sets(kernels, Xs, ys, X_tests, diags, means, test_means, test_diags,
                                                       predict_kernels, include_mean, normals, False, ctx)
    samples = [f.reshape(shape + (f.shape[1],)) for f in draws]
    return (values, samples, info, cinfo) if return_info else (values, samples)


def single_gradient(solver, resid, vectors: bool):
    """``(value, info, kernel gradient, transform gradient, noise gradient, mean gradient)`` of one member on the
    single path, in the batch's shapes: ``DirectSolver.log_probability_and_grad`` itself."""
    value, g = solver.log_probability_and_grad(resid)
    kgrad = np.array(g["kernel"], dtype=np.float64)
    return (float(value), int(solver.info), kgrad, g["transform"], g["noise_diag"] if vectors else None,
            g["mean"] if vectors else None)


def _single_grad(kernel, X, y, diag, mean, ctx, vectors):
    """One data set on the single dense path: ``GaussianProcess(kernel, X, diag=diag,
    mean=mean).log_probability_and_grad(y)`` itself, its solver closed behind it."""
    from tinygp_amd.gp import GaussianProcess
    from tinygp_amd.solvers.direct import DirectSolver

    kwargs = {} if ctx is None else {"ctx": ctx}
    gp = GaussianProcess(kernel, X, diag=diag, solver=DirectSolver, **({} if mean is None else {"mean_value": mean}),
                         **kwargs)
    try:
        return single_gradient(gp.solver, gp._residual(y), vectors)
    finally:
        gp.solver.close()


def _single(kernel, X, y, diag, mean, ctx):
    """One data set on the single dense path: ``GaussianProcess(kernel, X, diag=diag, mean=mean).log_probability(y)``
    itself, its solver closed behind it."""
    from tinygp_amd.gp import GaussianProcess
    from tinygp_amd.solvers.direct import DirectSolver

    kwargs = {} if ctx is None else {"ctx": ctx}
    gp = GaussianProcess(kernel, X, diag=diag, solver=DirectSolver, **({} if mean is None else {"mean_value": mean}),
                         **kwargs)
    try:
        return float(gp.log_probability(y)), int(gp.solver.info)
    finally:
        gp.solver.close()
