"""``GaussianProcess`` front-end (mirror of reference ``gp.py:30-393`` for the dense path).

Same constructor, properties, ``log_probability`` / ``condition`` / ``predict`` and error
conventions as the reference; every O(N^2) / O(N^3) step is delegated to the solver, which
runs it on the MI355X.  Two deliberate departures, both invisible in the results:

* ``log_probability`` uses the solver's fused solve+reduce entry point when it has one
  (the reference's two ``@jax.jit`` stages ``gp.py:313-320``);
* the GP returned by ``condition`` builds its covariance / M x M factor lazily -- the
  reference computes them eagerly (``gp.py:201-221``) and relies on XLA dead-code
  elimination when the caller only reads ``.loc``.

``sample`` draws its standard normals with NumPy on the host (JAX's threefry stream cannot be
reproduced bit for bit; moments match) and multiplies by L on the device;
``numpyro_dist`` is adjacent to the hot path and not provided.
"""

from __future__ import annotations

from collections.abc import Callable
from typing import Any, NamedTuple

import numpy as np

from tinygp_amd import _device, kernels, means
from tinygp_amd.noise import Diagonal, Noise
from tinygp_amd.solvers import DirectSolver, QuasisepSolver

__all__ = ["GaussianProcess", "ConditionResult"]


def _eval_mean(mean_function, X, n, dtype):
    return means.evaluate_mean(mean_function, X, n, dtype)  # (methods below take an argument named ``means``)


def _default_diag(reference: np.ndarray):
    """sqrt(eps) of the mean's dtype (reference ``gp.py:388-393``)."""
    return np.sqrt(np.finfo(np.asarray(reference).dtype).eps)


class GaussianProcess:
    """Interface for designing a Gaussian Process regression model.

    Args:
        kernel: the kernel function.
        X: input coordinates, shape (N,) or (N, D).
        diag: value(s) added to the diagonal of the covariance (scalar or (N,)); defaults to
            ``sqrt(eps)`` like the reference.
        noise: a :mod:`tinygp_amd.noise` model (overrides ``diag``).
        mean: a scalar, a callable of one coordinate, or a :class:`means.MeanBase`.
        solver: the solver class, default :class:`solvers.QuasisepSolver` for a
            ``kernels.quasisep.Quasisep`` kernel and :class:`solvers.DirectSolver` otherwise.
        mean_value / covariance_value: pre-computed mean vector / covariance matrix.
        **solver_kwargs: forwarded to the solver constructor (e.g. ``ctx=``).
    """

    def __init__(self, kernel: kernels.Kernel, X, *, diag=None, noise: Noise | None = None,
                 mean: means.MeanBase | Callable | Any | None = None, solver: Any | None = None,
                 mean_value=None, covariance_value: Any | None = None, _lazy: bool = False,
                 **solver_kwargs: Any):
        self.kernel = kernel
        self.X = X

        if isinstance(mean, means.MeanBase):
            self.mean_function = mean
        elif mean is None:
            self.mean_function = means.Mean(np.zeros(()))
        else:
            self.mean_function = means.Mean(mean)

        if mean_value is None:
            if _device.is_tree(X):  # pytree input (gp.py:64-112): host-evaluated kernels only
                n_pts = _device.num_points(X)
                dt = _device.common_dtype(*_device.tree_leaves(X))
            else:
                P = _device.points(X, limit=False)
                n_pts, dt = P.shape[0], P.dtype
            mean_value = means.evaluate_mean(self.mean_function, X, n_pts, dt)
        mean_value = np.asarray(mean_value)
        if mean_value.dtype.kind != "f":
            mean_value = mean_value.astype(np.float64)
        self.num_data = mean_value.shape[0] if mean_value.ndim else 0
        self.dtype = mean_value.dtype
        self.mean = mean_value
        if self.mean.ndim != 1:
            raise ValueError(f"Invalid mean shape: expected ndim = 1, got ndim={self.mean.ndim}")

        if noise is None:
            diag = _default_diag(self.mean) if diag is None else diag
            noise = Diagonal(diag=np.broadcast_to(np.asarray(diag, dtype=self.dtype),
                                                  self.mean.shape))
        self.noise = noise

        if solver is None:  # reference gp.py:101-105
            solver = QuasisepSolver if isinstance(kernel, kernels.quasisep.Quasisep) else DirectSolver
        self._solver_cls = solver
        self._solver_args = (covariance_value, solver_kwargs)
        self._solver = None
        if not _lazy:
            _ = self.solver

    @property
    def solver(self):
        if self._solver is None:
            covariance_value, solver_kwargs = self._solver_args
            if callable(covariance_value):  # lazy conditional covariance
                covariance_value = covariance_value()
            self._solver = self._solver_cls(self.kernel, self.X, self.noise,
                                            covariance=covariance_value, **solver_kwargs)
        return self._solver

    # -- reference gp.py:114-124 ------------------------------------------------------
    @property
    def loc(self):
        return self.mean

    @property
    def variance(self):
        if self._solver is None and isinstance(self.kernel, kernels.Conditioned):
            # conditioned GP: diag(Kss - A^T A) + noise without the M x M factorisation
            return self.kernel(self.X) + np.asarray(self.noise.diagonal())
        return self.solver.variance()

    @property
    def covariance(self):
        if self._solver is None and callable(self._solver_args[0]):
            cov = self._solver_args[0]()
            self._solver_args = (cov, self._solver_args[1])
            return cov
        return self.solver.covariance()

    # -- reference gp.py:273-311 ---------------------------------------------------------
    def sample(self, key, shape=None):
        """Draw samples from the prior: ``mean + L z`` (reference ``gp.py:273-311``).

        ``key``: an ``int`` seed or a ``numpy.random.Generator`` (the reference takes a JAX
        PRNG key; the random stream necessarily differs, the distribution does not).
        Returns shape ``shape + (N,)`` like the reference.
        """
        rng = key if isinstance(key, np.random.Generator) else np.random.default_rng(key)
        full = (self.num_data,) if shape is None else (self.num_data,) + tuple(shape)
        z = rng.standard_normal(full).astype(self.dtype, copy=False)
        out = self.solver.dot_triangular(z)
        return self.mean + np.moveaxis(out, 0, -1)

    def sample_conditional(self, y, X_test=None, *, key, shape=None, include_mean: bool = True):
        """Draw samples of the latent process from the posterior given ``y``, at ``X_test`` (``None``: at the data), in
        O(N + M) per draw: what ``condition(y, X_test).gp.sample(key)`` draws from, without the M x M covariance and
        its factorisation, and without the noise or jitter that route adds.

        ``key``: an ``int`` seed or a ``numpy.random.Generator``, as in :meth:`sample`; the standard normals ``xi``
        (N + M, J, R), then ``eps`` (N, R), are drawn from it.  Returns shape ``shape + (M,)``, the mean function at
        the output points added when ``include_mean``.  Needs a solver with ``sample_conditional``
        (:class:`solvers.QuasisepSolver`)."""
        fused = getattr(self.solver, "sample_conditional", None)
        if fused is None:
            raise TypeError(f"{type(self.solver).__name__} has no sample_conditional: posterior samples in O(N + M) "
                            "are drawn by QuasisepSolver (a kernels.quasisep kernel on sorted 1-D inputs)")
        rng = key if isinstance(key, np.random.Generator) else np.random.default_rng(key)
        shape = () if shape is None else tuple(shape)
        R = int(np.prod(shape, dtype=np.int64))
        n, m = self.num_data, 0 if X_test is None else _device.num_points(X_test)
        resid = self._residual(y)
        xi = rng.standard_normal((n + m, self.solver.state_dimension, R))
        eps = rng.standard_normal((n, R))
        out = np.asarray(fused(resid, X_test, xi=xi, eps=eps), dtype=self.dtype)
        out = np.moveaxis(out, 0, -1).reshape(shape + (out.shape[0],))
        if include_mean:
            out = out + (self.loc if X_test is None else means.evaluate_mean(self.mean_function, X_test, m, self.dtype))
        return out.astype(self.dtype, copy=False)

    # -- reference gp.py:126-138, 313-320 ---------------------------------------------
    def log_probability(self, y):
        """Marginal log-probability of ``y`` under this multivariate normal."""
        resid = self._residual(y)
        fused = getattr(self.solver, "log_probability", None)
        if fused is not None:
            return fused(resid)
        return self._compute_log_prob(self.solver.solve_triangular(resid))

    def log_probability_batch(self, y, kernels, *, diags=None, means=None):
        """The log-probabilities of ``y`` under B models that share this GP's coordinates, evaluated together
        (the reference's ``jax.vmap`` over the function that builds the GP): the walkers of an ensemble sampler, the
        starts of an optimiser, a grid over a period.

        ``kernels``: B kernels.  ``diags``: ``None`` (this GP's noise), (B,) one value per member or (B, N) diagonals.
        ``means``: ``None`` (this GP's mean vector), (B,) constants or (B, N) vectors.  Returns B values; member b is
        ``GaussianProcess(kernels[b], X, diag=diags[b], mean=means[b]).log_probability(y)``.

        On a :class:`tinygp_amd.solvers.QuasisepSolver` the kernels are ``kernels.quasisep`` models of one structure
        and every member equals that call to the bit.  On a :class:`tinygp_amd.solvers.DirectSolver` (the dense path)
        the members may differ in structure -- leaves, sums, products, metrics, input transforms -- and each is held to
        the project's 1e-8 bar against that call, not to the bits of a single call: up to ``TGP_SMALL_MAX_N`` points a
        workgroup evaluates a whole member in LDS (``csrc/small.hip``), above it the members are evaluated one by one.
        Needs a solver with ``log_probability_batch``."""
        fused = getattr(self.solver, "log_probability_batch", None)
        if fused is None:
            raise NotImplementedError(f"{type(self.solver).__name__} has no log_probability_batch: batches of models "
                                      "are evaluated by QuasisepSolver (a kernels.quasisep kernel on sorted 1-D "
                                      "inputs) and by DirectSolver (any other kernel)")
        kernels = list(kernels)
        return fused(kernels, *self._batch_inputs(y, len(kernels), diags, means))

    def log_probability_and_grad_batch(self, y, kernels, *, diags=None, means=None):
        """:meth:`log_probability_and_grad` of ``y`` under B models that share this GP's coordinates, evaluated
        together: ``(values (B,), grads)`` with ``grads = {"kernel": (B, P), "noise_diag": (B, N), "mean": (B, N),
        "transform": None}``.  Arguments as in :meth:`log_probability_batch`; row b equals
        ``GaussianProcess(kernels[b], X, diag=diags[b], mean=means[b]).log_probability_and_grad(y)`` to the bit.
        Needs a solver with ``value_and_grad_batch`` (:class:`tinygp_amd.solvers.QuasisepSolver`).  The dense path's
        batches of gradients have another return shape (its members may differ in structure) and entry points of their
        own: ``DirectSolver.log_probability_and_grad_batch`` over this GP's coordinates, and
        :func:`tinygp_amd.log_probability_and_grad_datasets` for data sets with points of their own."""
        fused = getattr(self.solver, "value_and_grad_batch", None)
        if fused is None:
            raise NotImplementedError(f"{type(self.solver).__name__} has no value_and_grad_batch: batches of gradients "
                                      "through this method are evaluated by QuasisepSolver (a kernels.quasisep kernel "
                                      "on sorted 1-D inputs); on the dense path use "
                                      "DirectSolver.log_probability_and_grad_batch or "
                                      "tinygp_amd.log_probability_and_grad_datasets")
        kernels = list(kernels)
        return fused(kernels, *self._batch_inputs(y, len(kernels), diags, means))

    def predict_batch(self, y, kernels, X_test=None, *, diags=None, means=None, return_var: bool = True,
                      include_mean: bool = True):
        """:meth:`predict` of ``y`` under B models that share this GP's coordinates, at one shared set of test points,
        evaluated together (the reference's ``jax.vmap`` over the function that builds the GP and predicts): the
        candidates of an acquisition function under every member of an ensemble, restarts compared on held-out points.

        ``kernels``, ``diags`` and ``means`` as in :meth:`log_probability_batch`; ``X_test``: ``None`` for this GP's
        points.  Returns the (B, M) means, or ``(means, variances)`` with ``return_var``; row b is
        ``GaussianProcess(kernels[b], X, diag=diags[b], mean=means[b]).predict(y, X_test, return_var=True)`` with the
        default jitter of :meth:`condition` in the variances, held to the project's posterior bar against that call.
        With ``include_mean`` the constant ``means[b]`` -- or, with ``means=None``, this GP's mean function at the
        test points -- is added to row b; (B, N) mean vectors enter the residual only.  Needs a solver with
        ``predict_batch`` (:class:`tinygp_amd.solvers.DirectSolver`: up to ``TGP_SMALL_MAX_N`` points a workgroup
        conditions and predicts a whole member in LDS, ``csrc/small.hip``; above it the members are evaluated one by
        one).  Data sets with points of their own: :func:`tinygp_amd.predict_datasets`."""
        fused = getattr(self.solver, "predict_batch", None)
        if fused is None:
            raise NotImplementedError(f"{type(self.solver).__name__} has no predict_batch: batches of predictions are "
                                      "evaluated by DirectSolver (the dense path); a kernels.quasisep model predicts "
                                      "through QuasisepSolver's predict and predict_terms")
        kernels = list(kernels)
        nb = len(kernels)
        resid, noise = self._batch_inputs(y, nb, diags, means)
        _, mu, var = fused(kernels, resid, X_test, noise, return_var=return_var)
        if include_mean:
            if means is None:
                mu = mu + (self.loc if X_test is None else
                           _eval_mean(self.mean_function, X_test, _device.num_points(X_test), self.dtype))
            elif np.ndim(means) == 1:
                mu = mu + np.asarray(means, dtype=self.dtype)[:, None]
        mu = np.asarray(mu, dtype=self.dtype)
        if not return_var:
            return mu
        return mu, np.asarray(var + _default_diag(self.mean), dtype=self.dtype)

    def _condition_batch(self, y, kernels, X_test, diags, means, diag, include_mean, xi, return_cov):
        """``(means, covariances or None, draws (B, R, M) or None)`` of B models at one set of test points, the mean
        function and the default jitter added: the body of :meth:`condition_batch` and
        :meth:`sample_conditional_batch`."""
        fused = getattr(self.solver, "condition_batch", None)
        if fused is None:
            raise NotImplementedError(f"{type(self.solver).__name__} has no condition_batch: batches of joint "
                                      "posteriors are evaluated by DirectSolver (the dense path); a kernels.quasisep "
                                      "model draws through QuasisepSolver's sample_conditional")
        kernels = list(kernels)
        nb = len(kernels)
        resid, noise = self._batch_inputs(y, nb, diags, means)
        tau = _default_diag(self.mean) if diag is None else diag
        _, mu, cov, draws = fused(kernels, resid, X_test, noise, test_diag=tau, xi=xi, return_cov=return_cov)
        if include_mean:
            shift = None
            if means is None:
                shift = (self.loc if X_test is None else
                         _eval_mean(self.mean_function, X_test, _device.num_points(X_test), self.dtype))
            elif np.ndim(means) == 1:
                shift = np.asarray(means, dtype=self.dtype)[:, None]
            if shift is not None:
                mu = mu + shift
                if draws is not None:  # (B, R, M): a member's constant, or the mean function at the M points
                    draws = draws + (shift[:, None] if np.ndim(shift) == 2 else shift)
        return (np.asarray(mu, dtype=self.dtype), None if cov is None else np.asarray(cov, dtype=self.dtype),
                None if draws is None else np.asarray(draws, dtype=self.dtype))

    def condition_batch(self, y, kernels, X_test=None, *, diags=None, means=None, diag=None, include_mean: bool = True):
        """:meth:`condition` of ``y`` under B models that share this GP's coordinates, at one shared set of test
        points, evaluated together: ``(means (B, M), covariances (B, M, M))``; row b is the ``gp.loc`` and
        ``gp.covariance`` of ``GaussianProcess(kernels[b], X, diag=diags[b], mean=means[b]).condition(y, X_test,
        diag=diag)``, held to the project's posterior bar against that call.  ``kernels``, ``diags``, ``means`` and
        ``include_mean`` as in :meth:`predict_batch`; ``diag``: what is added to the diagonal of every covariance, a
        scalar or (M,), ``None`` for the default jitter of :meth:`condition`.  Needs a solver with ``condition_batch``
        (:class:`tinygp_amd.solvers.DirectSolver`: with N + M up to ``TGP_SMALL_MAX_N`` a workgroup conditions a whole
        member in LDS, ``csrc/small.hip``; above it the members are evaluated one by one).  Data sets with points of
        their own: :func:`tinygp_amd.condition_datasets`."""
        mu, cov, _ = self._condition_batch(y, kernels, X_test, diags, means, diag, include_mean, None, True)
        return mu, cov

    def sample_conditional_batch(self, y, kernels, X_test=None, *, key, shape=None, diags=None, means=None, diag=None,
                                 include_mean: bool = True):
        """Joint posterior draws under B models that share this GP's coordinates, at one shared set of test points,
        evaluated together: what ``condition(y, X_test, diag=diag).gp.sample(key, shape)`` draws from for every member
        (Thompson sampling over a candidate set under every member of an ensemble).  Arguments as in
        :meth:`condition_batch`; ``key``: an int seed or a ``numpy.random.Generator``, as in :meth:`sample` -- the
        standard normals (B, R, M), R the product of ``shape``, are drawn from it.  Returns (B,) + shape + (M,); no
        covariance crosses the bus.  A member whose covariance does not factor has NaN draws.  Needs a solver with
        ``condition_batch``.  Data sets with points of their own: :func:`tinygp_amd.sample_conditional_datasets`."""
        rng = key if isinstance(key, np.random.Generator) else np.random.default_rng(key)
        shape = () if shape is None else tuple(shape)
        kernels = list(kernels)
        M = self.num_data if X_test is None else _device.num_points(X_test)
        xi = rng.standard_normal((len(kernels), int(np.prod(shape, dtype=np.int64)), M))
        _, _, draws = self._condition_batch(y, kernels, X_test, diags, means, diag, include_mean, xi, False)
        return draws.reshape((len(kernels),) + shape + (M,))

    def _batch_inputs(self, y, nb, diags, means):
        """``(resid, noise)`` of a batch of nb models: the arguments of the solver's batch methods."""
        n = self.num_data

        def per_member(a, what):  # (B,) -> (B, N) of this GP's dtype, (B, N) kept
            a = np.asarray(a)
            if a.shape not in ((nb,), (nb, n)):
                raise ValueError(f"{what} must have shape ({nb},) or ({nb}, {n}); got {a.shape}")
            a = a.astype(self.dtype, copy=False)
            return np.broadcast_to(a[:, None], (nb, n)) if a.ndim == 1 else a

        if means is None:
            resid = self._residual(y)
        else:
            resid = (np.asarray(y) - per_member(means, "means")).astype(self.dtype, copy=False)
            if resid.shape != (nb, n):
                raise ValueError(f"y must broadcast against the means of shape ({nb}, {n})")
        noise = None if diags is None else per_member(diags, "diags")
        return resid, noise

    def log_probability_and_grad(self, y):
        """``(log_probability, grads)``; see :meth:`solvers.DirectSolver.log_probability_and_grad`.
        ``grads["kernel"]`` follows ``self.kernel.parameters()``.  A solver with a ``value_and_grad`` of its own
        (:class:`solvers.QuasisepSolver`) is differentiated through that."""
        fused = getattr(self.solver, "value_and_grad", None)
        if fused is not None:
            return fused(self._residual(y))
        return self.solver.log_probability_and_grad(self._residual(y))

    def _residual(self, y):
        y = np.asarray(y)
        try:
            return np.broadcast_to(y - self.loc, self.loc.shape).astype(self.dtype, copy=False)
        except ValueError as e:
            raise ValueError(f"y must broadcast against the mean of shape {self.loc.shape}") from e

    def _get_alpha(self, y):
        return self.solver.solve_triangular(self._residual(y))

    def _compute_log_prob(self, alpha):
        loglike = -0.5 * np.sum(np.square(alpha)) - self.solver.normalization()
        return self.dtype.type(loglike if np.isfinite(loglike) else -np.inf)

    # -- reference gp.py:140-223, 322-361 ---------------------------------------------
    def _condition(self, y, X_test, include_mean: bool, kernel=None):
        resid = self._residual(y)
        two_solves = getattr(self.solver, "alpha", None)
        if two_solves is not None:
            alpha, log_prob = two_solves(resid)
        else:
            a = self.solver.solve_triangular(resid)
            log_prob = self._compute_log_prob(a)
            alpha = self.solver.solve_triangular(a, transpose=True)

        if X_test is None:
            if kernel is None:
                # predicting at the data with the original kernel: O(N) (gp.py:342-346)
                delta = self.noise @ alpha
                mean_value = np.asarray(y) - delta
                if not include_mean:
                    mean_value = mean_value - self.loc
            else:
                mean_value = self._kernel_matvec(kernel, self.X, alpha)
                if include_mean:
                    mean_value = mean_value + self.loc
        else:
            if kernel is None:
                kernel = self.kernel
            mean_value = self._kernel_matvec(kernel, X_test, alpha)
            if include_mean:
                mean_value = mean_value + means.evaluate_mean(self.mean_function, X_test,
                                                              _device.num_points(X_test), self.dtype)
        return alpha, log_prob, np.asarray(mean_value, dtype=self.dtype)

    def _kernel_matvec(self, kernel, X_out, alpha):
        fused = getattr(self.solver, "conditional_mean", None)
        if fused is not None:
            return fused(kernel, X_out, alpha)  # X resident on the device
        return kernel.matmul(X_out, self.X, alpha)

    def condition(self, y, X_test=None, *, diag=None, noise: Noise | None = None,
                  include_mean: bool = True, kernel: kernels.Kernel | None = None):
        """Condition the model on observed data ``y``; returns ``ConditionResult``."""
        if X_test is not None:
            if _device.is_tree(self.X) or _device.is_tree(X_test):
                same = _device.tree_structure(self.X) == _device.tree_structure(X_test)
            else:
                a, b = np.asarray(self.X), np.asarray(X_test)
                same = a.ndim == b.ndim and a.shape[1:] == b.shape[1:]
            if not same:
                raise ValueError(
                    "`X_test` must have the same tree structure as the input `X`, "
                    "and all but the leading dimension must have matching sizes")

        alpha, log_prob, mean_value = self._condition(y, X_test, include_mean, kernel)
        if kernel is None:
            kernel = self.kernel

        if noise is None:
            diag = _default_diag(mean_value) if diag is None else diag
            noise = Diagonal(diag=np.broadcast_to(np.asarray(diag, dtype=self.dtype),
                                                  mean_value.shape))

        solver, Xt = self.solver, X_test
        covariance_value = lambda: solver.condition(kernel, Xt, noise)  # noqa: E731 (lazy)
        if X_test is None:
            X_test = self.X

        gp = GaussianProcess(
            kernels.Conditioned(self.X, self.solver, kernel), X_test, noise=noise,
            mean=means.Conditioned(self.X, alpha, kernel, include_mean=include_mean,
                                   mean_function=self.mean_function),
            mean_value=mean_value, covariance_value=covariance_value, _lazy=True)
        return ConditionResult(log_prob, gp)

    def predict(self, y, X_test=None, *, kernel: kernels.Kernel | None = None,
                include_mean: bool = True, return_var: bool = False, return_cov: bool = False):
        """Reference ``gp.py:225-271``."""
        _, cond = self.condition(y, X_test, kernel=kernel, include_mean=include_mean)
        if return_var:
            return cond.loc, cond.variance
        if return_cov:
            return cond.loc, cond.covariance
        return cond.loc

    def predict_terms(self, y, X_test=None, *, kernels=None, return_var: bool = False):
        """The contribution of each term of a sum kernel to the prediction (the reference's
        ``condition(y, X_test, kernel=k1)`` for every ``k1`` at once): ``means`` of shape (K, M), or ``(means, vars)``
        with ``return_var``.  ``kernels=None`` means the top-level addends of the kernel; ``X_test=None`` the data.
        The mean function enters through the residual only and is added to no term; no jitter is added to the
        variances.  Needs a solver with ``predict_terms`` (:class:`tinygp_amd.solvers.QuasisepSolver`)."""
        fused = getattr(self.solver, "predict_terms", None)
        if fused is None:
            raise TypeError(f"{type(self.solver).__name__} has no predict_terms: the terms of a sum are predicted by "
                            "QuasisepSolver (a kernels.quasisep kernel on sorted 1-D inputs)")
        return fused(self._residual(y), X_test, kernels, return_var=return_var)


class ConditionResult(NamedTuple):
    """``(log_probability, gp)`` (reference ``gp.py:364-385``)."""

    log_probability: Any
    gp: GaussianProcess
