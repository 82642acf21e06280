"""``QuasisepSolver`` on MI355X (mirror of reference ``solvers/quasisep/solver.py``).

For a :class:`tinygp_amd.kernels.quasisep.Quasisep` kernel on sorted 1-D inputs, ``K + diag(noise)`` has a Cholesky
factor described by O(N J) numbers (``c_n``, ``w_n``; ``tests/_quasisep_np.py`` states the recursion).  A
``tgp_qsep`` handle (C ABI, ``include/tgp_hip.h``) keeps t, the noise and that factor resident on the device; the
factorisation, both triangular solves and ``L @ z`` are chunked reduce-then-scan recurrences in
``csrc/qsep.hip``, and so are the conditional mean and variance at M test points (``predict_mean_var``; O(N + M),
nothing of size N x M), the same for every term of a sum at once (``predict_terms``; also at the data themselves),
posterior draws by Matheron's rule (``sample_conditional``; O(N + M) per draw),
the gradient of the log-probability (``value_and_grad``; O(N) per parameter) and the log-probabilities of many
hyper-parameter sets over the one series in one launch chain (``log_probability_batch``; with their gradients:
``value_and_grad_batch``).  :class:`QuasisepSeriesSet` evaluates many series, each on coordinates of its own, in one
launch chain (``tgp_qsep_series_logprob``; with their gradients: ``tgp_qsep_series_grad``; with predictions at test
points of their own: ``tgp_qsep_series_predict``; with posterior draws there and at the data:
``tgp_qsep_series_sample``).  Nothing
of size N x N is ever formed, except by ``covariance()`` (host, O(N^2), as in the
reference); the full conditional covariance and conditioning on another kernel keep the reference's dense route.

dtypes: the device computes in fp64 whatever the inputs are; with fp32 inputs the results are returned as fp32
(the Riccati recursion loses positivity quickly in fp32 arithmetic).

Numerical failure never raises (as :class:`~tinygp_amd.solvers.DirectSolver`): a non-positive pivot sets
``self.info`` to its 1-based step, ``log_probability`` returns ``-inf`` and the affected outputs are NaN.
"""

from __future__ import annotations

import ctypes as C
from typing import Any

import numpy as np

from tinygp_amd import _device, _ffi
from tinygp_amd.noise import Diagonal, Noise
from tinygp_amd.solvers.solver import Solver

__all__ = ["QuasisepSolver", "QuasisepSeriesSet"]


def _check_sorted(t):
    if np.any(np.diff(t) < 0):
        raise ValueError(
            "Input coordinates must be sorted in order to use the QuasisepSolver")


def _f64(a, shape=None):
    a = np.asarray(a, dtype=np.float64)
    if shape is not None:
        a = np.broadcast_to(a, shape)
    return np.ascontiguousarray(a)


class QuasisepSolver(Solver):
    """O(N J^2) solver for quasiseparable kernels on sorted 1-D inputs.

    Args:
        kernel: a :class:`tinygp_amd.kernels.quasisep.Quasisep` kernel (state dimension J <= 8 on the device).
        X: sorted coordinates, shape (N,) or (N, 1).
        noise: a :class:`tinygp_amd.noise.Diagonal` noise model.
        covariance: not supported (a dense matrix defeats the purpose; pass the kernel instead).
        assume_sorted: skip the host check that X is sorted.
        parallel: accepted for compatibility with the reference and ignored: the device always scans.
        ctx: optional :class:`tinygp_amd._ffi.Ctx`.
    """

    def __init__(self, kernel, X, noise: Noise, *, covariance: Any | None = None, assume_sorted: bool = False,
                 parallel: bool = False, ctx=None):
        from tinygp_amd.kernels.quasisep import Quasisep, _coords

        del parallel
        if covariance is not None:
            raise TypeError("QuasisepSolver takes no covariance=: it works from the quasiseparable kernel itself")
        if not isinstance(noise, Diagonal):
            raise TypeError(f"QuasisepSolver supports noise.Diagonal only (got {type(noise).__name__}); use "
                            "DirectSolver for dense noise")
        if not isinstance(kernel, Quasisep):
            raise TypeError("QuasisepSolver needs a kernels.quasisep.Quasisep kernel")
        self.kernel, self.X, self.noise = kernel, X, noise
        t = _coords(X)
        noise_diag = np.asarray(noise.diagonal())
        self.dtype = _device.common_dtype(t, noise_diag)
        self.n = t.shape[0]
        if noise_diag.shape != (self.n,):
            raise ValueError("the noise model must have one entry per data point")
        if not assume_sorted:
            _check_sorted(t)
        self._t = _f64(t)
        self._noise = _f64(noise_diag)
        self._ssm = kernel._lower_ssm()
        self._ctx = _ffi.default_ctx() if ctx is None else ctx
        self._handle = None
        h = C.c_void_p()
        _ffi.check(_ffi.lib().tgp_qsep_create(self._ctx.handle, self.n, _ffi.ptr(self._t), C.byref(h)),
                   "tgp_qsep_create")
        self._handle = h
        self._info = 0
        self._factored = False

    # -- factorisation -------------------------------------------------------------
    def _model_args(self):
        s = self._ssm
        self._margs = (_f64(s.leaves), np.ascontiguousarray(s.state_map, dtype=np.int32), _f64(s.h), _f64(s.Pinf))
        lv, sm, h, P = self._margs
        return (_ffi.ptr(lv), len(lv), _ffi.ptr(sm), len(h), _ffi.ptr(h), _ffi.ptr(P), _ffi.ptr(self._noise))

    def refactor(self, kernel=None) -> int:
        """(Re-)factor in place, optionally with a new kernel of the same coordinates."""
        if kernel is not None:
            self._ssm, self.kernel = kernel._lower_ssm(), kernel
        info = C.c_int32(0)
        _ffi.check(_ffi.lib().tgp_qsep_factor(self._handle, *self._model_args(), C.byref(info)), "tgp_qsep_factor")
        self._info, self._factored = int(info.value), True
        return self._info

    def _ensure_factor(self):
        if not self._factored:
            self.refactor()

    @property
    def info(self) -> int:
        """0, or the 1-based step of the first non-positive pivot."""
        self._ensure_factor()
        return self._info

    def factor_data(self):
        """``(c, w)``: the factor's diagonal squares (N,) and its state vectors (N, J), as float64 host arrays."""
        self._ensure_factor()
        c = np.empty(self.n)
        w = np.empty((self.n, self._ssm.J))
        _ffi.check(_ffi.lib().tgp_qsep_factor_data(self._handle, _ffi.ptr(c), _ffi.ptr(w)), "tgp_qsep_factor_data")
        return c, w

    # -- Solver protocol -------------------------------------------------------------
    def variance(self):
        return (self.kernel(self.X) + self._noise).astype(self.dtype, copy=False)

    def covariance(self):
        """Dense, on the host, O(N^2) memory (reference ``solver.py`` makes the same caveat)."""
        K = np.asarray(self.kernel(self.X, self.X), dtype=np.float64)
        K[np.diag_indices(self.n)] += self._noise
        return K.astype(self.dtype, copy=False)

    def normalization(self):
        self._ensure_factor()
        out = C.c_double()
        _ffi.check(_ffi.lib().tgp_qsep_normalization(self._handle, C.byref(out)), "tgp_qsep_normalization")
        return self.dtype.type(np.nan if self._info else out.value)

    def _affine(self, fn, y, *args):
        self._ensure_factor()
        y = np.asarray(y)
        if y.ndim < 1 or y.shape[0] != self.n:
            raise ValueError(f"y must have leading dimension {self.n}; got {y.shape}")
        dt = np.result_type(self.dtype, y.dtype) if y.dtype.kind == "f" else self.dtype
        yy = _f64(y.reshape(self.n, -1))
        out = np.empty_like(yy)
        if yy.shape[1]:
            _ffi.check(fn(self._handle, *args, yy.shape[1], _ffi.ptr(yy), _ffi.ptr(out)), "tgp_qsep")
        if self._info:
            out[:] = np.nan
        return out.reshape(y.shape).astype(dt, copy=False)

    def solve_triangular(self, y, *, transpose: bool = False):
        """``L x = y`` or ``L^T x = y``; y (N,) or (N, R)."""
        return self._affine(_ffi.lib().tgp_qsep_solve_tri, y, int(bool(transpose)))

    def dot_triangular(self, y):
        """``L @ y``."""
        return self._affine(_ffi.lib().tgp_qsep_dot_tri, y)

    def _cond(self, kernel, X_test, var_only: bool):
        """``Kss - A^T A`` with ``A = L^-1 Ks``: Ks and Kss on the host, the M-column solve on the device
        (the reference's own fallback, ``solvers/quasisep/solver.py:130-139``)."""
        Xt = self.X if X_test is None else X_test
        A = self.solve_triangular(np.asarray(kernel(self.X, Xt), dtype=np.float64))
        if var_only:
            return np.asarray(kernel(Xt), dtype=np.float64) - np.sum(A * A, axis=0)
        return np.asarray(kernel(Xt, Xt), dtype=np.float64) - A.T @ A

    def condition(self, kernel, X_test, noise):
        out = self._cond(kernel, X_test, False)
        if isinstance(noise, Diagonal):
            out[np.diag_indices(out.shape[0])] += np.asarray(noise.diagonal())
        else:
            out = out + noise
        return out.astype(self.dtype, copy=False)

    def condition_variance(self, kernel, X_test):
        if kernel is self.kernel and X_test is not None and X_test is not self.X:  # O(N + M) on the device
            return self._predict(None, False, X_test, False, True)[1]
        return self._cond(kernel, X_test, True).astype(self.dtype, copy=False)

    def conditional_mean(self, kernel, X_out, alpha):
        """``k(X_out, X) @ alpha`` (the hook of ``GaussianProcess._kernel_matvec``): on the device in O(N + M) for
        the solver's own kernel at test points, on the host otherwise."""
        if kernel is self.kernel and X_out is not self.X and np.ndim(alpha) == 1:
            return self._predict(alpha, True, X_out, True, False)[0]
        if kernel is self.kernel and X_out is not self.X and np.ndim(alpha) == 2:
            return self._predict_mean_cols(alpha, True, X_out)
        return kernel.matmul(X_out, self.X, alpha)

    # -- prediction at test points -------------------------------------------------------
    def _predict(self, v, is_alpha, X_test, want_mean, want_var):
        from tinygp_amd.kernels.quasisep import _coords

        self._ensure_factor()
        x = _f64(_coords(X_test))
        m = x.shape[0]
        vv = _f64(v, (self.n,)) if want_mean else None
        mean = np.empty(m) if want_mean else None
        var = np.empty(m) if want_var else None
        if m:
            _ffi.check(_ffi.lib().tgp_qsep_predict(self._handle, _ffi.ptr(vv), int(bool(is_alpha)), m, _ffi.ptr(x),
                                                   _ffi.ptr(mean), _ffi.ptr(var)), "tgp_qsep_predict")
        cast = lambda a: None if a is None else a.astype(self.dtype, copy=False)  # noqa: E731
        return cast(mean), cast(var)

    def _predict_mean_cols(self, v, is_alpha, X_test):
        """The conditional mean for the R columns of ``v`` (N, R) at once (``tgp_qsep_predict_mean``): (M, R)."""
        from tinygp_amd.kernels.quasisep import _coords

        x = _f64(_coords(X_test))
        v = np.asarray(v)
        if v.ndim != 2 or v.shape[0] != self.n:
            raise ValueError(f"a block of residuals must have shape ({self.n}, R); got {v.shape}")
        self._ensure_factor()
        vv = _f64(v)
        mean = np.empty((x.shape[0], vv.shape[1]))
        _ffi.check(_ffi.lib().tgp_qsep_predict_mean(self._handle, vv.shape[1], _ffi.ptr(vv), int(bool(is_alpha)),
                                                    x.shape[0], _ffi.ptr(x), _ffi.ptr(mean)), "tgp_qsep_predict_mean")
        return mean.astype(self.dtype, copy=False)

    def predict_mean_var(self, resid, X_test, *, return_var: bool = True):
        """Conditional mean ``k(X_test, X) K^-1 resid`` and variance ``k(x, x) - k(x, X) K^-1 k(X, x)`` (no noise
        added) at M test points, in O((N + M) J^2 + M log N) on the device (``csrc/qsep.hip``, ``qs_pred_*``).

        ``X_test``: shape (M,) or (M, 1), in any order and anywhere relative to the data; M = 0 is allowed.
        Returns ``(mean, var)``, or the mean alone with ``return_var=False``.  After a failed factor both are NaN.
        With ``return_var=False`` ``resid`` may also hold R residuals as the columns of an (N, R) array: the means come
        back as (M, R) from one pair of scans per 8 columns (``qs_cm_*``).
        """
        if np.ndim(resid) == 2 and not return_var:
            return self._predict_mean_cols(resid, False, X_test)
        mean, var = self._predict(resid, False, X_test, True, return_var)
        return (mean, var) if return_var else mean

    def predict_terms(self, resid, X_test=None, kernels=None, *, return_var: bool = True):
        """What each term of a sum contributes: for every kernel ``k_j`` of ``kernels`` the conditional mean
        ``k_j(X_test, X) K^-1 resid`` and variance ``k_j(x, x) - k_j(x, X) K^-1 k_j(X, x)`` (no noise added), with
        ``K`` the whole model's.  All terms share one pair of device scans (``tgp_qsep_predict_terms``): O(N + K M).

        ``kernels``: terms of the solver's kernel in the sense of :meth:`Quasisep._term_vector`; ``None`` means its
        flattened top-level addends, in order (a kernel that is no sum gives one row).  More than 8 are served in
        batches of 8.  ``X_test``: as in :meth:`predict_mean_var`; ``None`` predicts at the data without uploading or
        sorting anything.  Returns ``(means, vars)`` of shape (K, M), or the means alone with ``return_var=False``;
        after a failed factor both are NaN."""
        from tinygp_amd.kernels.quasisep import MAX_STATE, _coords

        terms = self.kernel._addends() if kernels is None else list(kernels)
        gs = []
        for k in terms:
            g = self.kernel._term_vector(k)
            if g is None:
                raise ValueError(
                    f"{k!r} is not a term of the solver's kernel: a term is that kernel itself, one of the addends or "
                    "partial sums reached from it through Sum nodes (the same object, not an equal copy), or a Sum of "
                    "such addends; a factor of a Product and the kernel inside a Scale are not terms")
            gs.append(g)
        self._ensure_factor()
        x = None if X_test is None else _f64(_coords(X_test))
        m = self.n if x is None else x.shape[0]
        vv = _f64(resid, (self.n,))
        means = np.empty((len(gs), m))
        vars_ = np.empty((len(gs), m)) if return_var else None
        for b in range(0, len(gs) if m else 0, MAX_STATE):
            g = _f64(np.stack(gs[b:b + MAX_STATE]))
            mean = np.empty((len(g), m))
            var = np.empty((len(g), m)) if return_var else None
            _ffi.check(_ffi.lib().tgp_qsep_predict_terms(self._handle, _ffi.ptr(vv), 0, m, _ffi.ptr(x), len(g),
                                                         _ffi.ptr(g), _ffi.ptr(mean), _ffi.ptr(var)),
                       "tgp_qsep_predict_terms")
            means[b:b + len(g)] = mean
            if return_var:
                vars_[b:b + len(g)] = var
        means = means.astype(self.dtype, copy=False)
        return (means, vars_.astype(self.dtype, copy=False)) if return_var else means

    # -- posterior samples ------------------------------------------------------------------
    @property
    def state_dimension(self) -> int:
        """J: the number of standard normals a sample takes per point."""
        return self._ssm.J

    def sample_conditional(self, resid, X_test=None, *, xi, eps, return_data: bool = False):
        """Draws of the latent process conditioned on ``resid``, at M test points and at the data, in O((N + M) J^3) per
        draw on the device (``tgp_qsep_sample``; Matheron's rule: a prior draw over the merged grid of data and test
        points by the state-space recurrence, then the conditional mean of what the data say about it).  Nothing of
        size N x M or M x M is formed.  No noise or jitter is added: the result is the latent process.

        The draw is a function of the standard normals passed in: ``xi`` of shape (N + M, J, R), row p for point p of
        ``[X; X_test]``, and ``eps`` of shape (N, R); ``xi`` (N + M, J) and ``eps`` (N,) give 1-D results.  Column c does
        not depend on R or on the other columns, bit for bit.  ``X_test``: (M,) or (M, 1), any order, anywhere relative
        to the data, finite.  Returns the samples at the test points (M, R), or ``(data (N, R), test (M, R))`` with
        ``return_data``; ``X_test=None`` returns the (N, R) samples at the data.  After a failed factor the result is
        NaN.  fp32 inputs are computed in fp64 and returned as fp32."""
        from tinygp_amd.kernels.quasisep import _coords

        x = None if X_test is None else _f64(_coords(X_test))
        n, m, J = self.n, 0 if x is None else x.shape[0], self._ssm.J
        xi, eps = np.asarray(xi), np.asarray(eps)
        one = xi.ndim == 2
        R = 1 if one else (xi.shape[2] if xi.ndim == 3 else -1)
        if xi.ndim not in (2, 3) or xi.shape[:2] != (n + m, J):
            raise ValueError(f"xi must have shape ({n + m}, {J}) or ({n + m}, {J}, R); got {xi.shape}")
        if eps.shape != ((n,) if one else (n, R)):
            raise ValueError(f"eps must have shape {(n,) if one else (n, R)} beside xi of shape {xi.shape}; got "
                             f"{eps.shape}")
        if x is not None and not np.all(np.isfinite(x)):
            raise ValueError("X_test must be finite: a sample is a recurrence over all points")
        r = _f64(resid, (n,))
        self._ensure_factor()
        xi, eps = _f64(xi.reshape(n + m, J, R)), _f64(eps.reshape(n, R))
        want_data = return_data or x is None
        data = np.empty((n, R)) if want_data else None
        test = None if x is None else np.empty((m, R))
        passes = C.c_int32(0)
        _ffi.check(_ffi.lib().tgp_qsep_sample(self._handle, _ffi.ptr(r), m, _ffi.ptr(x), R, _ffi.ptr(xi), _ffi.ptr(eps),
                                              _ffi.ptr(data), _ffi.ptr(test), C.byref(passes)), "tgp_qsep_sample")
        self.sample_passes = int(passes.value)  # passes of columns the last call took
        shape = lambda a: None if a is None else (a[:, 0] if one else a).astype(self.dtype, copy=False)  # noqa: E731
        data, test = shape(data), shape(test)
        if x is None:
            return data
        return (data, test) if return_data else test

    # -- fused entry points used by GaussianProcess ------------------------------------
    def log_probability(self, resid):
        """Factor + forward solve + sums in one call; non-finite or a failed factor -> ``-inf``."""
        r = _f64(resid, (self.n,))
        info, out = C.c_int32(0), C.c_double()
        _ffi.check(_ffi.lib().tgp_qsep_factor_logprob(self._handle, *self._model_args(), _ffi.ptr(r),
                                                      C.byref(info), C.byref(out)), "tgp_qsep_factor_logprob")
        self._info, self._factored = int(info.value), True
        v = out.value
        if self._info or not np.isfinite(v):
            v = -np.inf
        return self.dtype.type(v)

    def log_probability_batch(self, kernels, resid, noise=None, *, return_info: bool = False):
        """The log-probabilities of B models over this solver's coordinates, evaluated together on the device
        (``tgp_qsep_logprob_batch``: one model per grid row, so that a short series still fills the card).

        ``kernels``: a sequence of B :class:`~tinygp_amd.kernels.quasisep.Quasisep` kernels of one structure
        (:func:`tinygp_amd.kernels.quasisep.pack_batch`).  ``resid``: (N,) shared or (B, N).  ``noise``: ``None`` (the
        solver's own diagonal), (N,) shared or (B, N) diagonals.  Returns B values, each with the bits of
        :meth:`log_probability` of a solver built with that member's kernel and noise; a failed or non-finite member
        gives ``-inf``.  With ``return_info`` also the B ``info`` values.  fp32 inputs are computed in fp64 and
        returned as fp32.  The solver's own kernel and factor are neither used nor changed."""
        from tinygp_amd.kernels.quasisep import pack_batch

        kernels = list(kernels)
        nb = len(kernels)
        if nb == 0:
            out = np.empty(0, dtype=self.dtype)
            return (out, np.empty(0, dtype=np.int32)) if return_info else out
        leaves, smap, h, P = pack_batch(kernels)

        def rows(a, what):  # (N,) -> shared, (B, N) -> one per member
            a = np.asarray(a)
            if a.shape == (self.n,):
                return _f64(a), 0
            if a.shape == (nb, self.n):
                return _f64(a), self.n
            raise ValueError(f"{what} must have shape ({self.n},) or ({nb}, {self.n}); got {a.shape}")

        r, r_stride = rows(resid, "resid")
        d, d_stride = (self._noise, 0) if noise is None else rows(noise, "noise")
        info, out = np.zeros(nb, dtype=np.int32), np.empty(nb)
        _ffi.check(_ffi.lib().tgp_qsep_logprob_batch(self._handle, nb, _ffi.ptr(leaves), leaves.shape[1],
                                                     _ffi.ptr(smap), h.shape[1], _ffi.ptr(h), _ffi.ptr(P),
                                                     _ffi.ptr(d), d_stride, _ffi.ptr(r), r_stride, _ffi.ptr(info),
                                                     _ffi.ptr(out), None), "tgp_qsep_logprob_batch")
        out[(info != 0) | ~np.isfinite(out)] = -np.inf
        out = out.astype(self.dtype, copy=False)
        return (out, info) if return_info else out

    def alpha(self, resid):
        """``(K^-1 r, log_probability)``."""
        self._ensure_factor()
        z = self.solve_triangular(_f64(resid, (self.n,)))
        a = self.solve_triangular(z, transpose=True)
        v = -0.5 * float(np.sum(np.square(z, dtype=np.float64))) - float(self.normalization())
        if self._info or not np.isfinite(v):
            v = -np.inf
        return a.astype(self.dtype, copy=False), self.dtype.type(v)

    def value_and_grad(self, resid):
        """``(log_probability, grads)`` with ``grads = {"kernel": [...], "noise_diag": (N,), "mean": (N,),
        "transform": None}``, the dictionary of :meth:`DirectSolver.log_probability_and_grad`: derivatives with
        respect to ``kernel.parameters()`` (same order), to every noise variance and to every entry of the mean
        vector (``K^-1 r``).  Exact, forward mode, O(N J^3) per parameter on the device (``csrc/qsep.hip``,
        ``tgp_qsep_grad``): the tangents of the factor and of the forward solve are two more scans per parameter,
        the noise gradient one backward scan; nothing of size N x N or N x P x N is formed.

        A failed factor gives ``-inf`` and NaN gradients; fp32 inputs are computed in fp64 and returned as fp32.  A
        critically damped ``SHO`` has no derivative with respect to ``quality``: that entry is NaN."""
        tangents = self.kernel._ssm_tangents()
        s = self._ssm
        ndir, L, J = len(tangents), len(s.leaves), s.J
        dleaves, dh, dP = np.zeros((ndir, L, 4)), np.zeros((ndir, J)), np.zeros((ndir, J, J))
        undefined = []
        for i, t in enumerate(tangents):
            if np.all(np.isfinite(t.dleaves)) and np.all(np.isfinite(t.dh)) and np.all(np.isfinite(t.dPinf)):
                dleaves[i], dh[i], dP[i] = t.dleaves, t.dh, t.dPinf
            else:
                undefined.append(i)
        v, kgrad, gnoise, alpha = self._grad_call(resid, dleaves, dh, dP)
        kgrad[undefined] = np.nan
        if self._info or not np.isfinite(v):
            v = -np.inf
            kgrad[:] = np.nan
            gnoise[:] = np.nan
            alpha[:] = np.nan
        return self.dtype.type(v), {"kernel": [float(g) for g in kgrad],
                                    "noise_diag": gnoise.astype(self.dtype, copy=False),
                                    "mean": alpha.astype(self.dtype, copy=False), "transform": None}

    def value_and_grad_batch(self, kernels, resid, noise=None, *, vectors: bool = True, return_info: bool = False):
        """:meth:`value_and_grad` of B models over this solver's coordinates, evaluated together on the device
        (``tgp_qsep_grad_batch``: one model per grid layer of the gradient's kernels): the starts of an optimiser, a
        population of HMC chains, many stars observed at one cadence (one residual per member).

        ``kernels``, ``resid`` and ``noise`` as in :meth:`log_probability_batch`; every member must have the same
        number of parameters (:func:`tinygp_amd.kernels.quasisep.pack_batch_tangents`).  Returns ``(values (B,),
        grads)`` with ``grads = {"kernel": (B, P), "noise_diag": (B, N), "mean": (B, N), "transform": None}``; row b
        has the bits of :meth:`value_and_grad` of a solver built with that member's kernel and noise.  With
        ``vectors=False`` the two (B, N) entries are ``None`` and their scans are skipped.  A failed or non-finite
        member gives ``-inf`` and NaN gradients, an undefined derivative (the quality of a critically damped ``SHO``)
        NaN.  With ``return_info`` also the B ``info`` values.  fp32 inputs are computed in fp64 and returned as fp32
        (the ``"kernel"`` rows stay float64, as the floats of :meth:`value_and_grad` do).  The solver's own kernel and
        factor are neither used nor changed."""
        from tinygp_amd.kernels.quasisep import pack_batch, pack_batch_tangents

        kernels = list(kernels)
        nb = len(kernels)
        if nb == 0:
            npar = len(self.kernel.parameters())
            vec = (lambda: np.empty((0, self.n), dtype=self.dtype)) if vectors else (lambda: None)
            out = np.empty(0, dtype=self.dtype), {"kernel": np.empty((0, npar)),
                                                  "noise_diag": vec(), "mean": vec(), "transform": None}
            return out + (np.empty(0, dtype=np.int32),) if return_info else out
        leaves, smap, h, P = pack_batch(kernels)
        dleaves, dh, dP, undefined = pack_batch_tangents(kernels)
        ndir = dh.shape[1]

        def rows(a, what):  # (N,) -> shared, (B, N) -> one per member
            a = np.asarray(a)
            if a.shape == (self.n,):
                return _f64(a), 0
            if a.shape == (nb, self.n):
                return _f64(a), self.n
            raise ValueError(f"{what} must have shape ({self.n},) or ({nb}, {self.n}); got {a.shape}")

        r, r_stride = rows(resid, "resid")
        d, d_stride = (self._noise, 0) if noise is None else rows(noise, "noise")
        info, out, kgrad = np.zeros(nb, dtype=np.int32), np.empty(nb), np.zeros((nb, ndir))
        gnoise, alpha = (np.empty((nb, self.n)), np.empty((nb, self.n))) if vectors else (None, None)
        _ffi.check(_ffi.lib().tgp_qsep_grad_batch(self._handle, nb, _ffi.ptr(leaves), leaves.shape[1], _ffi.ptr(smap),
                                                  h.shape[1], _ffi.ptr(h), _ffi.ptr(P), _ffi.ptr(d), d_stride,
                                                  _ffi.ptr(r), r_stride, ndir, _ffi.ptr(dleaves), _ffi.ptr(dh),
                                                  _ffi.ptr(dP), _ffi.ptr(info), _ffi.ptr(out), _ffi.ptr(kgrad),
                                                  _ffi.ptr(gnoise), _ffi.ptr(alpha), None, None),
                   "tgp_qsep_grad_batch")
        kgrad[undefined] = np.nan
        failed = (info != 0) | ~np.isfinite(out)
        out[failed] = -np.inf
        kgrad[failed] = np.nan
        if vectors:
            gnoise[failed] = np.nan
            alpha[failed] = np.nan
        cast = lambda a: None if a is None else a.astype(self.dtype, copy=False)  # noqa: E731
        result = cast(out), {"kernel": kgrad, "noise_diag": cast(gnoise), "mean": cast(alpha),
                             "transform": None}
        return result + (info,) if return_info else result

    def _grad_call(self, resid, dleaves, dh, dP, vectors: bool = True):
        """One ``tgp_qsep_grad``: the value, the derivatives along the given directions (``dleaves`` (P, L, 4), ``dh``
        (P, J), ``dP`` (P, J, J)) and, with ``vectors``, the noise gradient and alpha (else ``None``)."""
        r = _f64(resid, (self.n,))
        dleaves, dh, dP = _f64(dleaves), _f64(dh), _f64(dP)
        ndir = dh.shape[0]
        info, out = C.c_int32(0), C.c_double()
        kgrad = np.zeros(ndir)
        gnoise, alpha = (np.empty(self.n), np.empty(self.n)) if vectors else (None, None)
        _ffi.check(_ffi.lib().tgp_qsep_grad(self._handle, *self._model_args(), _ffi.ptr(r), ndir, _ffi.ptr(dleaves),
                                            _ffi.ptr(dh), _ffi.ptr(dP), C.byref(info), C.byref(out),
                                            _ffi.ptr(kgrad), _ffi.ptr(gnoise), _ffi.ptr(alpha)), "tgp_qsep_grad")
        self._info, self._factored = int(info.value), True
        return out.value, kgrad, gnoise, alpha

    def log_probability_and_grad(self, resid):
        raise NotImplementedError("the gradient of the quasiseparable log-probability is not yet implemented")

    # -- lifetime ----------------------------------------------------------------------
    def close(self):
        if getattr(self, "_handle", None):
            _ffi.lib().tgp_qsep_destroy(self._handle)
            self._handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def check_series(Xs, assume_sorted: bool = False):
    """The coordinates of a set of series as float64 vectors: each (N_b,) or (N_b, 1) with N_b >= 1 and, unless
    ``assume_sorted``, sorted; a ``ValueError`` names the member that is not."""
    from tinygp_amd.kernels.quasisep import _coords

    ts = []
    for b, X in enumerate(Xs):
        try:
            t = _coords(X)
        except ValueError as e:
            raise ValueError(f"series {b}: {e}") from e
        if t.shape[0] == 0:
            raise ValueError(f"series {b} is empty: every series needs at least one data point")
        if not assume_sorted and np.any(np.diff(t) < 0):
            raise ValueError(f"series {b}: input coordinates must be sorted in order to use the QuasisepSeriesSet")
        ts.append(_f64(t))
    if not ts:
        raise ValueError("a set of series needs at least one series")
    return ts


def pack_series(lengths, kernels, ys, diags, means=None):
    """The host arrays of ``tgp_qsep_series_logprob`` for series of the given lengths: ``(leaves, state_map, h, Pinf,
    noise, resid)``, the models stacked as by :func:`tinygp_amd.kernels.quasisep.pack_batch` (one shared kernel is
    lowered once and repeated), noise and residual concatenated.  A wrong count or length raises ``ValueError`` naming
    the member."""
    from tinygp_amd.kernels.quasisep import Quasisep, pack_batch

    lengths = np.asarray(lengths, dtype=np.int64)
    nb = len(lengths)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    if isinstance(kernels, Quasisep):
        leaves, smap, h, P = pack_batch([kernels])
        leaves, h, P = (np.ascontiguousarray(np.repeat(a, nb, axis=0)) for a in (leaves, h, P))
    else:
        kernels = list(kernels)
        if len(kernels) != nb:
            raise ValueError(f"kernels must be one kernel or one per series ({nb}); got {len(kernels)}")
        leaves, smap, h, P = pack_batch(kernels)

    def concat(values, what, scalars_ok):
        values = list(values)
        if len(values) != nb:
            raise ValueError(f"{what} must hold one entry per series ({nb}); got {len(values)}")
        out = np.empty(offsets[-1])
        for b, v in enumerate(values):
            v = np.asarray(v)
            if v.ndim == 2 and v.shape[1] == 1:
                v = v[:, 0]
            if not (v.shape == (lengths[b],) or (scalars_ok and v.shape == ())):
                raise ValueError(f"{what}[{b}] must have shape ({lengths[b]},)" + (" or be a scalar" if scalars_ok else "")
                                 + f" for series {b}; got {v.shape}")
            out[offsets[b]:offsets[b + 1]] = v
        return out

    resid = concat(ys, "ys", False)
    if means is not None:
        resid -= concat(means, "means", True)
    return leaves, smap, h, P, concat(diags, "diags", True), resid


def pack_series_tangents(lengths, kernels):
    """The parameter tangents of ``tgp_qsep_series_grad`` for series of the given lengths: ``(dleaves (B, P, L, 4), dh
    (B, P, J), dPinf (B, P, J, J), undefined (B, P) bool)`` as :func:`tinygp_amd.kernels.quasisep.pack_batch_tangents`
    makes them (a non-finite tangent -- the quality of a critically damped ``SHO`` -- is zeroed and flagged).  One
    shared kernel is lowered once and repeated, B kernels of one structure are stacked; a member whose parameter count
    differs raises ``ValueError`` naming it, and so does a wrong number of kernels."""
    from tinygp_amd.kernels.quasisep import Quasisep, pack_batch_tangents

    nb = len(lengths)
    if isinstance(kernels, Quasisep):
        return tuple(np.ascontiguousarray(np.repeat(a, nb, axis=0)) for a in pack_batch_tangents([kernels]))
    kernels = list(kernels)
    if len(kernels) != nb:
        raise ValueError(f"kernels must be one kernel or one per series ({nb}); got {len(kernels)}")
    return pack_batch_tangents(kernels)


def pack_series_tests(lengths, X_tests):
    """The test points of ``tgp_qsep_series_predict`` for series of the given lengths: ``(test_offsets (B + 1,) int64,
    xtest (sum m_b,) float64, at_data (B,) int32)``.  ``X_tests[b]``: (m_b,) or (m_b, 1), in any order, m_b = 0
    allowed; ``None`` predicts at the series' own points: its flag is set, its count is N_b and its part of ``xtest``
    stays zero (the device reads the resident coordinates instead).  A wrong count or shape raises ``ValueError``
    naming the series."""
    from tinygp_amd.kernels.quasisep import _coords

    nb = len(lengths)
    X_tests = list(X_tests)
    if len(X_tests) != nb:
        raise ValueError(f"X_tests must hold one entry per series ({nb}); got {len(X_tests)}")
    points, at_data = [], np.zeros(nb, dtype=np.int32)
    for b, X in enumerate(X_tests):
        if X is None:
            at_data[b] = 1
            points.append(np.zeros(int(lengths[b])))
            continue
        try:
            points.append(_f64(_coords(X)))
        except ValueError as e:
            raise ValueError(f"X_tests[{b}] of series {b}: {e}") from e
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in points])]).astype(np.int64)
    xtest = np.concatenate(points) if points else np.empty(0)
    return offsets, np.ascontiguousarray(xtest, dtype=np.float64), at_data


def series_added_means(means, test_offsets, test_means, include_mean: bool):
    """What ``include_mean`` adds to series b's predictions, a list of (m_b,) float64 arrays -- the convention of
    :func:`tinygp_amd.predict_datasets`: a scalar ``means[b]`` itself; for a vector ``means[b]`` -- it enters the
    residual only -- ``test_means[b]``, a scalar or (m_b,), which ``include_mean`` then requires.  A ``ValueError`` names
    the series."""
    nb = len(test_offsets) - 1
    counts = np.diff(test_offsets)

    def entries(values, what):
        values = [None] * nb if values is None else list(values)
        if len(values) != nb:
            raise ValueError(f"{what} must hold one entry per series ({nb}); got {len(values)}")
        return values

    means, test_means = entries(means, "means"), entries(test_means, "test_means")
    added = []
    for b, (mean, tmean) in enumerate(zip(means, test_means)):
        m = int(counts[b])
        if mean is None or np.ndim(mean) == 0:
            if tmean is not None:
                raise ValueError(f"test_means[{b}] is given, but means[{b}] of series {b} is not a vector: a scalar mean "
                                 "is added to the predictions by itself")
            added.append(np.zeros(m) if mean is None else np.full(m, np.asarray(mean, dtype=np.float64)))
        elif tmean is None:
            if include_mean:
                raise ValueError(f"means[{b}] of series {b} is a vector: the mean at its test points must be given as "
                                 f"test_means[{b}] (a scalar or ({m},)), or include_mean=False")
            added.append(np.zeros(m))
        else:
            t = np.asarray(tmean, dtype=np.float64)
            if t.ndim == 2 and t.shape[1] == 1:
                t = t[:, 0]
            if t.shape not in ((), (m,)):
                raise ValueError(f"test_means[{b}] must have shape ({m},) or be a scalar for series {b}; got {t.shape}")
            added.append(np.array(np.broadcast_to(t, (m,))))
    return added


def pack_series_sample_tests(lengths, X_tests):
    """The test points of ``tgp_qsep_series_sample``: as :func:`pack_series_tests`, but a ``None`` entry -- the series'
    own points -- counts 0 beside its flag (its draws at the data are an output already), and every test point must be
    finite: a ``ValueError`` names the series whose are not."""
    X_tests = list(X_tests)
    offsets, xtest, at_data = pack_series_tests(lengths, [np.empty(0) if X is None else X for X in X_tests])
    for b, X in enumerate(X_tests):
        at_data[b] = X is None
        if not np.all(np.isfinite(xtest[offsets[b]:offsets[b + 1]])):
            raise ValueError(f"X_tests[{b}] of series {b} must be finite: a sample is a recurrence over all points")
    return offsets, xtest, at_data


def pack_series_normals(lengths, counts, J, xi, eps):
    """The standard normals of ``tgp_qsep_series_sample`` for series of the given lengths and test-point counts:
    ``(xi_concat (sum (N_b + M_b) J, R), eps_concat (sum N_b, R), R, one)``, member b's rows after member b - 1's.
    ``xi[b]``: (N_b + M_b, J, R), ``eps[b]``: (N_b, R), one R for all; or every ``xi[b]`` (N_b + M_b, J) with ``eps[b]``
    (N_b,): ``one``, R = 1.  A wrong count or shape raises ``ValueError`` naming the member."""
    nb = len(lengths)
    xi, eps = [np.asarray(a) for a in xi], [np.asarray(a) for a in eps]
    if len(xi) != nb or len(eps) != nb:
        raise ValueError(f"xi and eps must hold one entry per series ({nb}); got {len(xi)} and {len(eps)}")
    one = xi[0].ndim == 2
    R = 1 if one else (xi[0].shape[2] if xi[0].ndim == 3 else -1)
    for b in range(nb):
        n, g = int(lengths[b]), int(lengths[b] + counts[b])
        want = (g, J) if one else (g, J, R)
        if xi[b].shape != want:
            raise ValueError(f"xi[{b}] must have shape {want} for series {b}"
                             + ("" if b == 0 else f" (as xi[0] has {xi[0].ndim} dimensions)") + f"; got {xi[b].shape}")
        if eps[b].shape != ((n,) if one else (n, R)):
            raise ValueError(f"eps[{b}] must have shape {(n,) if one else (n, R)} for series {b} beside xi[{b}] of shape "
                             f"{xi[b].shape}; got {eps[b].shape}")
    if R < 1:
        raise ValueError(f"xi[0] must have shape (N + M, J) or (N + M, J, R) with R >= 1; got {xi[0].shape}")
    xi_c = np.concatenate([_f64(a).reshape(-1, R) for a in xi])
    eps_c = np.concatenate([_f64(a).reshape(-1, R) for a in eps])
    return np.ascontiguousarray(xi_c), np.ascontiguousarray(eps_c), R, one


class QuasisepSeriesSet:
    """B series on coordinates of their own -- the light curves of a survey, each with its gaps, masks and length --
    evaluated together on the device: one series per grid row of every kernel (``tgp_qsep_series_logprob``), where a
    loop over :class:`QuasisepSolver` pays a handle and a launch chain per series and fills the card with none of them.

    Args:
        Xs: a sequence of B sorted coordinate arrays, each of shape (N_b,) or (N_b, 1) with N_b >= 1; the lengths may
            differ freely.
        assume_sorted: skip the host check that every member is sorted.
        ctx: optional :class:`tinygp_amd._ffi.Ctx`.

    The handle keeps the concatenated coordinates and the table of the series' extents resident; :meth:`close` frees it.
    """

    def __init__(self, Xs, *, assume_sorted: bool = False, ctx=None):
        self._handle = None
        ts = check_series(Xs, assume_sorted)
        self.lengths = np.array([len(t) for t in ts], dtype=np.int64)
        self._offsets = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self._t = np.concatenate(ts)
        self._ctx = _ffi.default_ctx() if ctx is None else ctx
        h = C.c_void_p()
        _ffi.check(_ffi.lib().tgp_qsep_series_create(self._ctx.handle, len(ts), _ffi.ptr(self._offsets),
                                                     _ffi.ptr(self._t), C.byref(h)), "tgp_qsep_series_create")
        self._handle = h

    def __len__(self):
        return len(self.lengths)

    def log_probability(self, kernels, ys, diags, *, means=None, return_info: bool = False):
        """The log-probabilities of the B series, float64, shape (B,).

        ``kernels``: one :class:`~tinygp_amd.kernels.quasisep.Quasisep` kernel shared by all series, or B of one
        structure (:func:`tinygp_amd.kernels.quasisep.pack_batch`).  ``ys``: B arrays, (N_b,) each.  ``diags``: B
        noise diagonals, each (N_b,) or a scalar.  ``means``: ``None``, or B means, each a scalar or (N_b,).  Member b
        has the bits of ``QuasisepSolver(kernels[b], Xs[b], Diagonal(diags[b])).log_probability(ys[b] - means[b])``
        on a fresh solver, whatever B, its position and the other members' lengths; a failed or non-finite member
        gives ``-inf`` and touches no other.  With ``return_info`` also the B ``info`` values (0, or the 1-based step
        of the first non-positive pivot within that series)."""
        if self._handle is None:
            raise ValueError("this QuasisepSeriesSet has been closed")
        leaves, smap, h, P, noise, resid = pack_series(self.lengths, kernels, ys, diags, means)
        nb = len(self)
        info, out = np.zeros(nb, dtype=np.int32), np.empty(nb)
        _ffi.check(_ffi.lib().tgp_qsep_series_logprob(self._handle, _ffi.ptr(leaves), leaves.shape[1], _ffi.ptr(smap),
                                                      h.shape[1], _ffi.ptr(h), _ffi.ptr(P), _ffi.ptr(noise),
                                                      _ffi.ptr(resid), _ffi.ptr(info), _ffi.ptr(out), None),
                   "tgp_qsep_series_logprob")
        out[(info != 0) | ~np.isfinite(out)] = -np.inf
        return (out, info) if return_info else out

    def value_and_grad(self, kernels, ys, diags, *, means=None, vectors: bool = True, return_info: bool = False):
        """Value and gradient of the B series in one launch chain (``tgp_qsep_series_grad``): what a population fit by
        L-BFGS or HMC needs per step.  Arguments as in :meth:`log_probability`; every member must have the same number
        of parameters (:func:`pack_series_tangents`).  Returns ``(values (B,), grads)`` with ``grads = {"kernel":
        (B, P) float64, "noise_diag": list of B arrays (N_b,), "mean": list of B arrays (N_b,), "transform": None}``;
        with ``vectors=False`` the two lists are ``None`` and their scans are skipped.  Member b has the bits of
        ``QuasisepSolver(kernels[b], Xs[b], Diagonal(diags[b])).value_and_grad(ys[b] - means[b])`` on a fresh solver,
        whatever B, its position, the other members' lengths and the split into chains and direction passes.  A failed
        or non-finite member gives ``-inf`` and NaN gradients and touches no other; an undefined derivative (the
        quality of a critically damped ``SHO``) is NaN in that entry only.  With ``return_info`` also the B ``info``
        values."""
        if self._handle is None:
            raise ValueError("this QuasisepSeriesSet has been closed")
        leaves, smap, h, P, noise, resid = pack_series(self.lengths, kernels, ys, diags, means)
        dleaves, dh, dP, undefined = pack_series_tangents(self.lengths, kernels)
        nb, ndir, total = len(self), dh.shape[1], int(self._offsets[-1])
        info, out, kgrad = np.zeros(nb, dtype=np.int32), np.empty(nb), np.zeros((nb, ndir))
        gnoise, alpha = (np.empty(total), np.empty(total)) if vectors else (None, None)
        _ffi.check(_ffi.lib().tgp_qsep_series_grad(self._handle, _ffi.ptr(leaves), leaves.shape[1], _ffi.ptr(smap),
                                                   h.shape[1], _ffi.ptr(h), _ffi.ptr(P), _ffi.ptr(noise),
                                                   _ffi.ptr(resid), ndir, _ffi.ptr(dleaves), _ffi.ptr(dh), _ffi.ptr(dP),
                                                   _ffi.ptr(info), _ffi.ptr(out), _ffi.ptr(kgrad), _ffi.ptr(gnoise),
                                                   _ffi.ptr(alpha), None, None), "tgp_qsep_series_grad")
        kgrad[undefined] = np.nan
        failed = (info != 0) | ~np.isfinite(out)
        out[failed] = -np.inf
        kgrad[failed] = np.nan
        split = lambda a: [a[lo:hi] for lo, hi in zip(self._offsets[:-1], self._offsets[1:])]  # noqa: E731
        gnoise, alpha = (split(gnoise), split(alpha)) if vectors else (None, None)
        for b in np.flatnonzero(failed) if vectors else ():
            gnoise[b][:] = np.nan
            alpha[b][:] = np.nan
        result = out, {"kernel": kgrad, "noise_diag": gnoise, "mean": alpha, "transform": None}
        return result + (info,) if return_info else result

    def predict(self, kernels, ys, diags, X_tests, *, means=None, test_means=None, return_var: bool = True,
                include_mean: bool = True, return_info: bool = False):
        """Value and prediction of the B series in one launch chain (``tgp_qsep_series_predict``): every light curve of
        a survey interpolated, detrended or scored on held-out points after the fit, where a loop of
        :meth:`QuasisepSolver.predict_mean_var` pays a handle, an upload, a launch chain and a stream synchronisation
        per series.

        ``kernels``, ``ys``, ``diags`` as in :meth:`log_probability`.  ``X_tests[b]``: (m_b,) or (m_b, 1), unsorted,
        with duplicates, anywhere relative to the data, m_b = 0 allowed; ``None`` predicts at the series' own points
        (nothing is uploaded for it).  ``means[b]``: a scalar is added to the predicted mean when ``include_mean``; a
        vector (N_b,) enters the residual only and needs ``test_means[b]``, a scalar or (m_b,), which is then what
        ``include_mean`` adds (the convention of :func:`tinygp_amd.predict_datasets`).

        Returns ``(values (B,), means, variances)``, float64: ``means`` and ``variances`` are lists of B arrays (m_b,)
        in the caller's order, ``variances`` (of the latent process: no noise added, as
        :meth:`QuasisepSolver.predict_mean_var`) ``None`` without ``return_var``, whose half of the device work is then
        skipped; with ``return_info`` the B ``info`` values come fourth.  Member b's value, mean and variance have the
        bits of ``QuasisepSolver(kernels[b], Xs[b], Diagonal(diags[b]))`` with ``.log_probability(r)`` and
        ``.predict_mean_var(r, X_tests[b])``, r = ``ys[b] - means[b]``, on a fresh solver, whatever B, its position, the
        other members' lengths and test points and the split into chains.  A failed or non-finite member gives ``-inf``
        and NaN predictions and touches no other."""
        if self._handle is None:
            raise ValueError("this QuasisepSeriesSet has been closed")
        leaves, smap, h, P, noise, resid = pack_series(self.lengths, kernels, ys, diags, means)
        test_offsets, xtest, at_data = pack_series_tests(self.lengths, X_tests)
        added = series_added_means(means, test_offsets, test_means, include_mean)
        nb, total = len(self), int(test_offsets[-1])
        info, out = np.zeros(nb, dtype=np.int32), np.empty(nb)
        mean = np.empty(max(total, 1))
        var = np.empty(max(total, 1)) if return_var else None
        _ffi.check(_ffi.lib().tgp_qsep_series_predict(self._handle, _ffi.ptr(leaves), leaves.shape[1], _ffi.ptr(smap),
                                                      h.shape[1], _ffi.ptr(h), _ffi.ptr(P), _ffi.ptr(noise),
                                                      _ffi.ptr(resid), _ffi.ptr(test_offsets),
                                                      _ffi.ptr(xtest) if total else None, _ffi.ptr(at_data),
                                                      _ffi.ptr(info), _ffi.ptr(out), _ffi.ptr(mean), _ffi.ptr(var),
                                                      None), "tgp_qsep_series_predict")
        failed = (info != 0) | ~np.isfinite(out)
        out[failed] = -np.inf
        split = lambda a: [a[lo:hi] for lo, hi in zip(test_offsets[:-1], test_offsets[1:])]  # noqa: E731
        mus = split(mean)
        variances = split(var) if return_var else None
        for b in range(nb):
            if failed[b]:
                mus[b] = np.full(len(mus[b]), np.nan)
                if return_var:
                    variances[b] = np.full(len(variances[b]), np.nan)
            elif include_mean:
                mus[b] = mus[b] + added[b]
        result = out, mus, variances
        return result + (info,) if return_info else result

    def sample_conditional(self, kernels, ys, diags, X_tests, *, xi, eps, means=None, return_data: bool = False,
                           return_info: bool = False):
        """Value and posterior draws of the B series in one launch chain (``tgp_qsep_series_sample``): draws of every
        fitted light curve of a survey, where a loop of :meth:`QuasisepSolver.sample_conditional` pays a handle, an
        upload, a launch chain and a stream synchronisation per series.

        ``kernels``, ``ys``, ``diags``, ``means`` as in :meth:`log_probability`; ``X_tests`` as in :meth:`predict`
        (finite; ``None``: the series' own points, whose test-side entry is then its data-side draw).  The draws are a
        function of the standard normals passed in, as :meth:`QuasisepSolver.sample_conditional` takes them: ``xi``, a
        list of B arrays (N_b + M_b, J, R), row p for point p of ``[Xs[b]; X_tests[b]]`` (M_b = 0 for ``None``), and
        ``eps``, a list of B arrays (N_b, R); all ``xi[b]`` (N_b + M_b, J) with ``eps[b]`` (N_b,) give 1-D results.

        Returns ``(values (B,), tests)``, ``tests`` a list of B arrays (M_b, R), float64; with ``return_data`` the list
        of the draws at the data (N_b, R) comes third, with ``return_info`` the B ``info`` values come last.  No noise
        is added: the draws are of the latent process, without any mean.  Member b's value and column c of its draws
        have the bits of ``QuasisepSolver(kernels[b], Xs[b], Diagonal(diags[b]))`` with ``.log_probability(r)`` and
        ``.sample_conditional(r, X_tests[b], xi=xi[b][..., c], eps=eps[b][:, c], return_data=True)``, r = ``ys[b] -
        means[b]``, on a fresh solver, whatever B, its position, the other members, R and the split into chains and
        passes (``self.sample_chains``, ``self.sample_passes``: what the last call took).  A failed or non-finite
        member gives ``-inf`` and NaN draws and touches no other."""
        if self._handle is None:
            raise ValueError("this QuasisepSeriesSet has been closed")
        leaves, smap, h, P, noise, resid = pack_series(self.lengths, kernels, ys, diags, means)
        test_offsets, xtest, at_data = pack_series_sample_tests(self.lengths, X_tests)
        J = h.shape[1]
        xi_c, eps_c, R, one = pack_series_normals(self.lengths, np.diff(test_offsets), J, xi, eps)
        nb, total, ntest = len(self), int(self._offsets[-1]), int(test_offsets[-1])
        info, out = np.zeros(nb, dtype=np.int32), np.empty(nb)
        want_data = return_data or bool(at_data.any())
        data = np.empty((total, R)) if want_data else None
        test = np.empty((max(ntest, 1), R))
        chains, passes = C.c_int32(0), C.c_int32(0)
        _ffi.check(_ffi.lib().tgp_qsep_series_sample(self._handle, _ffi.ptr(leaves), leaves.shape[1], _ffi.ptr(smap), J,
                                                     _ffi.ptr(h), _ffi.ptr(P), _ffi.ptr(noise), _ffi.ptr(resid),
                                                     _ffi.ptr(test_offsets), _ffi.ptr(xtest) if ntest else None,
                                                     _ffi.ptr(at_data), R, _ffi.ptr(xi_c), _ffi.ptr(eps_c),
                                                     _ffi.ptr(info), _ffi.ptr(out), _ffi.ptr(data), _ffi.ptr(test),
                                                     C.byref(chains), C.byref(passes)), "tgp_qsep_series_sample")
        self.sample_chains, self.sample_passes = int(chains.value), int(passes.value)
        failed = (info != 0) | ~np.isfinite(out)
        out[failed] = -np.inf
        shape = (lambda a: a[:, 0]) if one else (lambda a: a)
        cut = lambda a, offs: [shape(a[lo:hi]) for lo, hi in zip(offs[:-1], offs[1:])]  # noqa: E731
        datas = cut(data, self._offsets) if want_data else None
        tests = cut(test, test_offsets)
        for b in range(nb):
            if at_data[b]:
                tests[b] = datas[b]
        for b in np.flatnonzero(failed):
            tests[b] = np.full(tests[b].shape, np.nan)
            if want_data:
                datas[b] = np.full(datas[b].shape, np.nan)
        result = (out, tests) + ((datas,) if return_data else ())
        return result + (info,) if return_info else result

    def close(self):
        if getattr(self, "_handle", None):
            _ffi.lib().tgp_qsep_series_destroy(self._handle)
            self._handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def log_probability_series(kernels, Xs, ys, *, diags, means=None):
    """The log-probabilities of B series, each on coordinates of its own, under quasiseparable GPs: builds a
    :class:`QuasisepSeriesSet` on ``Xs``, evaluates it and closes it.  Member b equals
    ``GaussianProcess(kernels[b], Xs[b], diag=diags[b], mean=means[b]).log_probability(ys[b])`` for float64 inputs.
    Arguments as in :meth:`QuasisepSeriesSet.log_probability`; keep the set yourself to evaluate it more than once."""
    series = QuasisepSeriesSet(Xs)
    try:
        return series.log_probability(kernels, ys, diags, means=means)
    finally:
        series.close()


def predict_series(kernels, Xs, ys, X_tests, *, diags, means=None, test_means=None, return_var: bool = True,
                   include_mean: bool = True, return_info: bool = False):
    """Condition B quasiseparable GPs on series with coordinates of their own and predict at test points of their own:
    builds a :class:`QuasisepSeriesSet` on ``Xs``, calls its :meth:`~QuasisepSeriesSet.predict` and closes it.  Member
    b equals ``QuasisepSolver(kernels[b], Xs[b], Diagonal(diags[b]))`` with ``log_probability`` and
    ``predict_mean_var`` of ``ys[b] - means[b]`` at ``X_tests[b]`` bit for bit for float64 inputs.  Arguments and result
    as in :meth:`QuasisepSeriesSet.predict`; keep the set yourself to predict more than once."""
    series = QuasisepSeriesSet(Xs)
    try:
        return series.predict(kernels, ys, diags, X_tests, means=means, test_means=test_means, return_var=return_var,
                              include_mean=include_mean, return_info=return_info)
    finally:
        series.close()


def log_probability_and_grad_series(kernels, Xs, ys, *, diags, means=None, vectors: bool = True):
    """Value and gradient of B series, each on coordinates of its own, under quasiseparable GPs: builds a
    :class:`QuasisepSeriesSet` on ``Xs``, evaluates it and closes it.  Member b equals ``GaussianProcess(kernels[b],
    Xs[b], diag=diags[b], mean=means[b]).log_probability_and_grad(ys[b])`` for float64 inputs.  Arguments and result as
    in :meth:`QuasisepSeriesSet.value_and_grad`; keep the set yourself to evaluate it more than once."""
    series = QuasisepSeriesSet(Xs)
    try:
        return series.value_and_grad(kernels, ys, diags, means=means, vectors=vectors)
    finally:
        series.close()


def sample_conditional_series(kernels, Xs, ys, X_tests, *, diags, key, shape=None, means=None, test_means=None,
                              include_mean: bool = True, normals=None):
    """Posterior draws of the latent process of B quasiseparable GPs, each conditioned on a series with coordinates of
    its own, at test points of its own: builds a :class:`QuasisepSeriesSet` on ``Xs``, calls its
    :meth:`~QuasisepSeriesSet.sample_conditional` and closes it.

    ``key``: an ``int`` seed or a ``numpy.random.Generator``.  With R the product of ``shape``, it draws per member, in
    member order, ``xi_b = rng.standard_normal((N_b + M_b, J, R))``, then ``eps_b = rng.standard_normal((N_b, R))`` (M_b
    = 0 for ``X_tests[b] = None``), the order of :meth:`tinygp_amd.GaussianProcess.sample_conditional`: member 0 of a
    set, drawn with a fresh generator, equals ``GaussianProcess(kernels[0], Xs[0], diag=diags[0],
    mean=means[0]).sample_conditional(ys[0], X_tests[0], key=key, shape=shape)`` bit for bit for float64 inputs.
    ``normals``: a list of B pairs ``(xi_b, eps_b)`` of those shapes, which replaces the draw (``key`` is then not
    used).

    Returns ``(values (B,), samples)``: ``samples[b]`` has shape ``shape + (M_b,)``, or ``shape + (N_b,)`` for a member
    drawn at its own points.  ``means``, ``test_means``, ``include_mean``: as in :meth:`QuasisepSeriesSet.predict`
    (:func:`series_added_means`; a member at its own points counts its N_b outputs).  A failed or non-finite member
    gives ``-inf`` and NaN draws."""
    from tinygp_amd.kernels.quasisep import Quasisep, _coords

    shape = () if shape is None else tuple(shape)
    R = int(np.prod(shape, dtype=np.int64))
    series = QuasisepSeriesSet(Xs)
    try:
        nb = len(series)
        X_tests = list(X_tests)
        if len(X_tests) != nb:
            raise ValueError(f"X_tests must hold one entry per series ({nb}); got {len(X_tests)}")
        counts = [0 if X is None else len(_coords(X)) for X in X_tests]
        outs = [int(n) if X is None else m for n, X, m in zip(series.lengths, X_tests, counts)]
        added = series_added_means(means, np.concatenate([[0], np.cumsum(outs)]), test_means, include_mean)
        if normals is None:
            first = kernels if isinstance(kernels, Quasisep) else list(kernels)[0]
            J = first._lower_ssm().J
            rng = key if isinstance(key, np.random.Generator) else np.random.default_rng(key)
            normals = []
            for n, m in zip(series.lengths, counts):
                xi = rng.standard_normal((int(n) + m, J, R))
                normals.append((xi, rng.standard_normal((int(n), R))))
        else:
            normals = list(normals)
            if len(normals) != nb:
                raise ValueError(f"normals must hold one (xi, eps) pair per series ({nb}); got {len(normals)}")
        values, tests = series.sample_conditional(kernels, ys, diags, X_tests, xi=[p[0] for p in normals],
                                                  eps=[p[1] for p in normals], means=means)
    finally:
        series.close()
    samples = []
    for b, out in enumerate(tests):
        out = np.moveaxis(out, 0, -1).reshape(shape + (out.shape[0],))
        samples.append(out + added[b] if include_mean else out)
    return values, samples
