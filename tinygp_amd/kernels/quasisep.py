"""Quasiseparable (state-space) kernels for 1-D inputs (mirror of ``tinygp.kernels.quasisep``).

Every kernel here is the covariance of a linear stationary SDE observed through a design vector:

    k(t_i, t_j) = h^T A(|t_i - t_j|) P h,      A(dt) = expm(F dt),

with state dimension ``J = len(h)``, stationary covariance ``P`` (``stationary_covariance()``) and the
closed-form forward transition ``A``.  (The reference's ``transition_matrix(X1, X2)`` returns ``A^T``; the method
of the same name here keeps that convention, ``_phi`` returns ``A`` itself.)  Used with
:class:`tinygp_amd.solvers.QuasisepSolver` the likelihood, solves and samples cost O(N J^2) on the device.

Algebra: a :class:`Sum` is block-diagonal, a :class:`Product` is the Kronecker product of ``A``, ``P`` and ``h``
(``np.kron`` order: the second operand's index runs fastest), a :class:`Scale` multiplies ``P``.  Mixed with a dense
kernel the result is the ordinary :class:`tinygp_amd.kernels.Sum` / ``Product``.

Called directly (``k(X1, X2)``, ``matmul``) a quasiseparable kernel is evaluated on the host from the formula above,
in blocks of rows.  For the dense solvers, ``Exp``, ``Matern32``, ``Matern52`` and ``Cosine`` (sigma^2 times the
stationary leaves of the same name) and their sums / products lower to the device kernel program; ``Celerite`` and
``SHO`` have no program and reach :class:`~tinygp_amd.solvers.DirectSolver` through ``covariance=``.

:meth:`Quasisep._lower_ssm` is the compact description the device recursions read (``include/tgp_hip.h``,
``tgp_qsep_*``): a leaf table, a state map, ``h`` and ``P``.  The device holds ``J <= 8``.
"""

from __future__ import annotations

from typing import Any, NamedTuple

import numpy as np

from tinygp_amd import _device
from tinygp_amd.kernels import base
from tinygp_amd.kernels.distance import L1Distance

__all__ = ["Quasisep", "Sum", "Product", "Scale", "Celerite", "SHO", "Exp", "Matern32", "Matern52", "Cosine",
           "MAX_STATE", "MAX_LEAVES", "SSMTangent", "leaf_phi", "leaf_dphi", "model_dphi", "pack_batch",
           "pack_batch_tangents"]

MAX_STATE = 8   # TGP_QSEP_MAX_J of include/tgp_hip.h
MAX_LEAVES = 8  # TGP_QSEP_MAX_LEAVES

# leaf kinds of include/tgp_hip.h (TGP_QS_*)
QS_EXP, QS_M32, QS_M52, QS_COS, QS_CELERITE, QS_SHO_UNDER, QS_SHO_CRIT, QS_SHO_OVER = range(8)


class SSM(NamedTuple):
    """What the device reads.  ``leaves``: (L, 5) float64 rows ``(kind, p0, p1, p2, p3)``; ``state_map``: (J, L)
    int32, the index into leaf ``l``'s own state of global state ``r``, or -1 when leaf ``l`` is not a factor of
    the term ``r`` belongs to; ``h``: (J,); ``Pinf``: (J, J)."""

    leaves: np.ndarray
    state_map: np.ndarray
    h: np.ndarray
    Pinf: np.ndarray

    @property
    def J(self) -> int:
        return len(self.h)


class SSMTangent(NamedTuple):
    """The derivative of an :class:`SSM` with respect to one parameter: ``dleaves`` (L, 4), one tangent per stored
    leaf parameter (the dependent third parameter of an ``SHO`` included), ``dh`` (J,), ``dPinf`` (J, J)."""

    dleaves: np.ndarray
    dh: np.ndarray
    dPinf: np.ndarray


def _coords(X) -> np.ndarray:
    if _device.is_tree(X):
        raise NotImplementedError("quasiseparable kernels take 1-D coordinates, not pytrees")
    X = np.asarray(X)
    if X.ndim == 2 and X.shape[1] == 1:
        X = X[:, 0]
    if X.ndim != 1:
        raise ValueError(f"quasiseparable kernels take coordinates of shape (N,) or (N, 1); got {X.shape}")
    return X


def pack_batch(kernels):
    """Lower B kernels of one structure for ``tgp_qsep_logprob_batch``: ``(leaves (B, L, 5), state_map (J, L) int32,
    h (B, J), Pinf (B, J, J))``, float64 and contiguous.  Every member must have the first one's state dimension, leaf
    count and ``state_map``; leaf kinds may differ (an ``SHO`` in another damping regime).  A mismatch raises
    ``ValueError`` naming the member and what differs; J > 8 raises :class:`tinygp_amd._device.DeviceLimit`."""
    kernels = list(kernels)
    if not kernels:
        raise ValueError("pack_batch needs at least one kernel")
    for i, k in enumerate(kernels):
        if not isinstance(k, Quasisep):
            raise TypeError(f"kernel {i} of the batch is no kernels.quasisep.Quasisep kernel ({type(k).__name__})")
    ssms = [k._lower_ssm() for k in kernels]
    first = ssms[0]
    smap = np.ascontiguousarray(first.state_map, dtype=np.int32)
    for i, s in enumerate(ssms[1:], start=1):
        if s.J != first.J:
            raise ValueError(f"kernel {i} of the batch has state dimension J = {s.J}, kernel 0 has J = {first.J}")
        if len(s.leaves) != len(first.leaves):
            raise ValueError(f"kernel {i} of the batch has {len(s.leaves)} leaf kernels, kernel 0 has "
                             f"{len(first.leaves)}")
        if not np.array_equal(np.asarray(s.state_map, dtype=np.int32), smap):
            raise ValueError(f"kernel {i} of the batch has another state_map than kernel 0: the sums and products "
                             "must be nested alike")
    stack = lambda field: np.ascontiguousarray(  # noqa: E731
        np.stack([np.asarray(getattr(s, field), dtype=np.float64) for s in ssms]))
    return stack("leaves"), smap, stack("h"), stack("Pinf")


def pack_batch_tangents(kernels):
    """The parameter tangents of B kernels for ``tgp_qsep_grad_batch``: ``(dleaves (B, P, L, 4), dh (B, P, J), dPinf
    (B, P, J, J), undefined (B, P) bool)`` from each member's ``_ssm_tangents()``, float64 and contiguous.  A tangent
    with a non-finite entry (the quality of a critically damped ``SHO``) is zeroed and flagged in ``undefined``, as
    ``QuasisepSolver.value_and_grad`` does for one model.  Every member must have the first one's number of parameters;
    a mismatch raises ``ValueError`` naming the member.  The structure itself is checked by :func:`pack_batch`."""
    kernels = list(kernels)
    if not kernels:
        raise ValueError("pack_batch_tangents needs at least one kernel")
    for i, k in enumerate(kernels):
        if not isinstance(k, Quasisep):
            raise TypeError(f"kernel {i} of the batch is no kernels.quasisep.Quasisep kernel ({type(k).__name__})")
    tangents = [k._ssm_tangents() for k in kernels]
    nb, npar = len(kernels), len(tangents[0])
    for i, ts in enumerate(tangents):
        if len(ts) != npar:
            raise ValueError(f"kernel {i} of the batch has {len(ts)} parameters, kernel 0 has {npar}")
    ssm = kernels[0]._lower_ssm()
    L, J = len(ssm.leaves), ssm.J
    dleaves, dh, dP = np.zeros((nb, npar, L, 4)), np.zeros((nb, npar, J)), np.zeros((nb, npar, J, J))
    undefined = np.zeros((nb, npar), dtype=bool)
    for b, ts in enumerate(tangents):
        for i, t in enumerate(ts):
            if np.all(np.isfinite(t.dleaves)) and np.all(np.isfinite(t.dh)) and np.all(np.isfinite(t.dPinf)):
                dleaves[b, i], dh[b, i], dP[b, i] = t.dleaves, t.dh, t.dPinf
            else:
                undefined[b, i] = True
    return dleaves, dh, dP, undefined


class Quasisep(base.Kernel):
    """Base class of the quasiseparable kernels (reference ``kernels/quasisep.py:50-215``)."""

    # -- state-space description --------------------------------------------------
    def _ssm(self) -> SSM:
        raise NotImplementedError

    def _phi(self, dt) -> np.ndarray:
        """A(dt) for an array of lags: shape ``dt.shape + (J, J)``."""
        raise NotImplementedError

    def stationary_covariance(self) -> np.ndarray:
        return self._ssm().Pinf

    def observation_model(self, X=None) -> np.ndarray:
        del X
        return self._ssm().h

    def transition_matrix(self, X1, X2) -> np.ndarray:
        """The reference's convention: ``A(X2 - X1)^T``."""
        return np.swapaxes(self._phi(np.asarray(X2, dtype=np.float64) - np.asarray(X1, dtype=np.float64)), -1, -2)

    def coord_to_sortable(self, X):
        return X

    # -- parameters and their tangents (the gradient of QuasisepSolver.value_and_grad) --
    def parameters(self) -> list[tuple[Any, str]]:
        """The scalar hyper-parameters as ``(object, attribute)`` pairs in constructor order, depth first: the order
        of the ``"kernel"`` entry of :meth:`tinygp_amd.solvers.QuasisepSolver.value_and_grad`."""
        raise NotImplementedError

    def _ssm_tangents(self) -> list[SSMTangent]:
        """Per entry of :meth:`parameters`, the analytic derivative of :meth:`_ssm` with respect to it."""
        raise NotImplementedError

    def _lower_ssm(self) -> SSM:
        """The device description; raises :class:`tinygp_amd._device.DeviceLimit` beyond J = 8 or 8 leaves."""
        s = self._ssm()
        if s.J > MAX_STATE:
            raise _device.DeviceLimit(
                f"the quasiseparable device path holds state dimension J <= {MAX_STATE}; this kernel has J = {s.J}")
        if len(s.leaves) > MAX_LEAVES:
            raise _device.DeviceLimit(
                f"the quasiseparable device path holds at most {MAX_LEAVES} leaf kernels; this one has "
                f"{len(s.leaves)}")
        if not (np.all(np.isfinite(s.leaves)) and np.all(np.isfinite(s.h)) and np.all(np.isfinite(s.Pinf))):
            raise ValueError("non-finite quasiseparable kernel parameters")
        return s

    # -- terms of a sum (QuasisepSolver.predict_terms) ------------------------------
    def _addends(self) -> list:
        """The flattened addends: the leaves of the tree of ``Sum`` nodes rooted here, in state order."""
        if isinstance(self, Sum):
            return self.kernel1._addends() + self.kernel2._addends()
        return [self]

    def _term_vector(self, term):
        """The test-side observation vector ``g`` of ``term``, or ``None`` when ``term`` is not a term of this kernel.

        A sum's state is block-diagonal, so the covariance between one addend at x and the whole model at the data is
        the model's own with ``h`` masked to that addend's states.  Terms are found by object identity, walking from
        this kernel through ``Sum`` nodes only: this kernel itself (``g = h``), any addend or partial ``Sum`` of the
        tree, and a ``Sum`` built elsewhere whose flattened addends are all found that way (their union).  A factor
        of a ``Product``, the kernel inside a ``Scale`` and an equal-valued copy are not terms."""
        nodes = []  # (node, first state, one past its last), every node reachable through Sum nodes

        def walk(k, lo):
            nodes.append((k, lo, lo + k._ssm().J))
            if isinstance(k, Sum):
                walk(k.kernel1, lo)
                walk(k.kernel2, lo + k.kernel1._ssm().J)

        def find(k):
            for node, lo, hi in nodes:
                if node is k:
                    return [(lo, hi)]
            if isinstance(k, Sum):
                a, b = find(k.kernel1), find(k.kernel2)
                if a is not None and b is not None:
                    return a + b
            return None

        walk(self, 0)
        ranges = find(term)
        if ranges is None:
            return None
        h = self._ssm().h
        g = np.zeros_like(h)
        for lo, hi in ranges:
            g[lo:hi] = h[lo:hi]
        return g

    # -- dense value on the host ---------------------------------------------------
    def _k_of_lag(self, tau) -> np.ndarray:
        """k as a function of the lag ``tau >= 0`` (any shape)."""
        s = self._ssm()
        Ph = s.Pinf @ s.h
        return np.einsum("...ij,i,j->...", self._phi(tau), s.h, Ph)

    def _host_matrix(self, X1, X2):
        a, b = _coords(X1), _coords(X2)
        dt = _device.common_dtype(a, b)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        out = np.empty((a.shape[0], b.shape[0]), dtype=dt)
        step = max(1, (1 << 20) // max(1, b.shape[0] * self._ssm().J ** 2))
        for i0 in range(0, a.shape[0], step):
            out[i0:i0 + step] = self._k_of_lag(np.abs(a64[i0:i0 + step, None] - b64[None, :]))
        return out

    def _host_diag(self, X):
        a = _coords(X)
        s = self._ssm()
        return np.full(a.shape, s.h @ s.Pinf @ s.h, dtype=_device.common_dtype(a))

    def __call__(self, X1, X2=None):
        return self._host_diag(X1) if X2 is None else self._host_matrix(X1, X2)

    def evaluate(self, X1, X2):
        return self._host_matrix(np.reshape(X1, (1,)), np.reshape(X2, (1,)))[0, 0]

    def evaluate_diag(self, X):
        return self._host_diag(np.reshape(X, (1,)))[0]

    def matmul(self, X1, X2=None, y=None):
        """``k(X1, X2) @ y`` on the host, a bounded slab of rows of ``X1`` at a time."""
        if y is None:
            assert X2 is not None
            y = X2
            X2 = None
        if X2 is None:
            X2 = X1
        a, b = _coords(X1), _coords(X2)
        y = np.asarray(y)
        if y.shape[0] != b.shape[0]:
            raise ValueError("dimension mismatch between X2 and y in Kernel.matmul")
        rows = max(1, (1 << 22) // max(1, b.shape[0]))
        parts = [self._host_matrix(a[i0:i0 + rows], b) @ y for i0 in range(0, a.shape[0], rows)]
        if not parts:
            return np.zeros((0,) + y.shape[1:], dtype=np.result_type(y, _device.common_dtype(b)))
        return np.concatenate(parts, axis=0)

    # -- dense device program (Exp / Matern / Cosine trees only) --------------------
    def _lower(self, X):
        prog = self.program()
        return prog, _coords(X)

    # -- algebra (reference quasisep.py:164-199) ------------------------------------
    def __add__(self, other: Any):
        if isinstance(other, Quasisep):
            return Sum(self, other)
        return super().__add__(other)

    def __radd__(self, other: Any):
        if isinstance(other, Quasisep):
            return Sum(other, self)
        return super().__radd__(other)

    def __mul__(self, other: Any):
        if isinstance(other, Quasisep):
            return Product(self, other)
        if isinstance(other, base.Kernel) or np.ndim(other) != 0:
            return super().__mul__(other)
        return Scale(kernel=self, scale=other)

    def __rmul__(self, other: Any):
        if isinstance(other, Quasisep):
            return Product(other, self)
        if isinstance(other, base.Kernel) or np.ndim(other) != 0:
            return super().__rmul__(other)
        return Scale(kernel=self, scale=other)


def _leaf_ssm(kind, params, h, P) -> SSM:
    p = np.zeros(4)
    p[:len(params)] = params
    J = len(h)
    return SSM(np.array([[kind, *p]], dtype=np.float64), np.arange(J, dtype=np.int32)[:, None],
               np.asarray(h, dtype=np.float64), np.asarray(P, dtype=np.float64))


def _block_diag(a, b):
    out = np.zeros((a.shape[0] + b.shape[0], a.shape[1] + b.shape[1]), dtype=np.result_type(a, b))
    out[:a.shape[0], :a.shape[1]] = a
    out[a.shape[0]:, a.shape[1]:] = b
    return out


class Sum(Quasisep):
    """k1 + k2: block-diagonal state (reference ``quasisep.py:241-295``)."""

    def __init__(self, kernel1: Quasisep, kernel2: Quasisep, use_block: bool = True):
        self.kernel1, self.kernel2, self.use_block = kernel1, kernel2, use_block

    def _ssm(self):
        s1, s2 = self.kernel1._ssm(), self.kernel2._ssm()
        m = np.full((s1.J + s2.J, len(s1.leaves) + len(s2.leaves)), -1, dtype=np.int32)
        m[:s1.J, :len(s1.leaves)] = s1.state_map
        m[s1.J:, len(s1.leaves):] = s2.state_map
        return SSM(np.concatenate([s1.leaves, s2.leaves]), m, np.concatenate([s1.h, s2.h]),
                   _block_diag(s1.Pinf, s2.Pinf))

    def parameters(self):
        return self.kernel1.parameters() + self.kernel2.parameters()

    def _ssm_tangents(self):
        s1, s2 = self.kernel1._ssm(), self.kernel2._ssm()
        z1, z2 = SSMTangent(np.zeros((len(s1.leaves), 4)), np.zeros(s1.J), np.zeros((s1.J, s1.J))), \
            SSMTangent(np.zeros((len(s2.leaves), 4)), np.zeros(s2.J), np.zeros((s2.J, s2.J)))
        join = lambda a, b: SSMTangent(np.concatenate([a.dleaves, b.dleaves]), np.concatenate([a.dh, b.dh]),  # noqa: E731
                                       _block_diag(a.dPinf, b.dPinf))
        return ([join(d, z2) for d in self.kernel1._ssm_tangents()]
                + [join(z1, d) for d in self.kernel2._ssm_tangents()])

    def _phi(self, dt):
        a1, a2 = self.kernel1._phi(dt), self.kernel2._phi(dt)
        j1, j2 = a1.shape[-1], a2.shape[-1]
        out = np.zeros(np.shape(dt) + (j1 + j2, j1 + j2))
        out[..., :j1, :j1] = a1
        out[..., j1:, j1:] = a2
        return out

    def _k_of_lag(self, tau):
        return self.kernel1._k_of_lag(tau) + self.kernel2._k_of_lag(tau)

    def _emit(self, ops):
        self.kernel1._emit(ops)
        self.kernel2._emit(ops)
        ops.append((base.K_ADD, 0, 0.0, 0.0))

    def __repr__(self):
        return f"quasisep.Sum({self.kernel1!r}, {self.kernel2!r})"


class Product(Quasisep):
    """k1 * k2: Kronecker-product state (reference ``quasisep.py:298-331``)."""

    def __init__(self, kernel1: Quasisep, kernel2: Quasisep):
        self.kernel1, self.kernel2 = kernel1, kernel2

    def _ssm(self):
        s1, s2 = self.kernel1._ssm(), self.kernel2._ssm()
        m = np.concatenate([np.repeat(s1.state_map, s2.J, axis=0), np.tile(s2.state_map, (s1.J, 1))], axis=1)
        return SSM(np.concatenate([s1.leaves, s2.leaves]), m.astype(np.int32), np.kron(s1.h, s2.h),
                   np.kron(s1.Pinf, s2.Pinf))

    def parameters(self):
        return self.kernel1.parameters() + self.kernel2.parameters()

    def _ssm_tangents(self):
        s1, s2 = self.kernel1._ssm(), self.kernel2._ssm()
        z1, z2 = np.zeros((len(s1.leaves), 4)), np.zeros((len(s2.leaves), 4))
        return ([SSMTangent(np.concatenate([d.dleaves, z2]), np.kron(d.dh, s2.h), np.kron(d.dPinf, s2.Pinf))
                 for d in self.kernel1._ssm_tangents()]
                + [SSMTangent(np.concatenate([z1, d.dleaves]), np.kron(s1.h, d.dh), np.kron(s1.Pinf, d.dPinf))
                   for d in self.kernel2._ssm_tangents()])

    def _phi(self, dt):
        a1, a2 = self.kernel1._phi(dt), self.kernel2._phi(dt)
        j1, j2 = a1.shape[-1], a2.shape[-1]
        return np.einsum("...ik,...jl->...ijkl", a1, a2).reshape(np.shape(dt) + (j1 * j2, j1 * j2))

    def _k_of_lag(self, tau):
        return self.kernel1._k_of_lag(tau) * self.kernel2._k_of_lag(tau)

    def _emit(self, ops):
        self.kernel1._emit(ops)
        self.kernel2._emit(ops)
        ops.append((base.K_MUL, 0, 0.0, 0.0))

    def __repr__(self):
        return f"quasisep.Product({self.kernel1!r}, {self.kernel2!r})"


class Scale(Quasisep):
    """``scale * kernel`` (reference ``quasisep.py:334-340``): multiplies the stationary covariance."""

    def __init__(self, kernel: Quasisep, scale):
        self.kernel, self.scale = kernel, scale

    def _ssm(self):
        s = self.kernel._ssm()
        return SSM(s.leaves, s.state_map, s.h, float(self.scale) * s.Pinf)

    def parameters(self):
        return self.kernel.parameters() + [(self, "scale")]

    def _ssm_tangents(self):
        s = self.kernel._ssm()
        inner = [SSMTangent(d.dleaves, d.dh, float(self.scale) * d.dPinf) for d in self.kernel._ssm_tangents()]
        return inner + [SSMTangent(np.zeros((len(s.leaves), 4)), np.zeros(s.J), s.Pinf.copy())]

    def _phi(self, dt):
        return self.kernel._phi(dt)

    def _k_of_lag(self, tau):
        return float(self.scale) * self.kernel._k_of_lag(tau)

    def _emit(self, ops):
        if np.ndim(self.scale) != 0:
            raise ValueError("Quasisep kernels can only be multiplied by scalars and other Quasisep kernels")
        self.kernel._emit(ops)
        ops.append((base.K_CONST, 0, float(self.scale), 0.0))
        ops.append((base.K_MUL, 0, 0.0, 0.0))

    def __repr__(self):
        return f"quasisep.Scale({self.kernel!r}, scale={self.scale!r})"


def _damped(decay, m):
    """``exp(-decay) * m`` with m (..., J, J) built from a list of rows of arrays."""
    return np.exp(-decay)[..., None, None] * np.moveaxis(np.asarray(m, dtype=np.float64), (0, 1), (-2, -1))


def _leaf_tangent(dparams, dh, dP) -> SSMTangent:
    p = np.zeros((1, 4))
    p[0, :len(dparams)] = dparams
    return SSMTangent(p, np.asarray(dh, dtype=np.float64), np.asarray(dP, dtype=np.float64))


class _Leaf(Quasisep):
    _stationary: type | None = None  # the dense leaf this kernel equals sigma^2 times, if any
    _params: tuple = ("scale", "sigma")

    def parameters(self):
        return [(self, name) for name in self._params]

    def _emit(self, ops):
        if self._stationary is None:
            raise NotImplementedError(
                f"quasisep.{type(self).__name__} has no dense device program: use QuasisepSolver, or pass its matrix "
                "through covariance=")
        for name in ("scale", "sigma"):
            if np.ndim(getattr(self, name)) != 0:
                raise ValueError(f"the {name} of a quasiseparable kernel must be a scalar")
        ops.append((self._stationary._op, L1Distance.metric_code, float(self.scale), 0.0))
        ops.append((base.K_CONST, 0, float(self.sigma) ** 2, 0.0))
        ops.append((base.K_MUL, 0, 0.0, 0.0))

    def __repr__(self):
        args = ", ".join(f"{k}={v!r}" for k, v in vars(self).items())
        return f"quasisep.{type(self).__name__}({args})"


class Exp(_Leaf):
    """sigma^2 exp(-tau / scale) (reference ``quasisep.py:491-525``); J = 1."""

    def __init__(self, scale, sigma=1.0):
        self.scale, self.sigma = scale, sigma

    @property
    def _stationary(self):
        from tinygp_amd.kernels.stationary import Exp as E
        return E

    def design_matrix(self):
        return np.array([[-1.0 / self.scale]])

    def _ssm(self):
        return _leaf_ssm(QS_EXP, [1.0 / float(self.scale)], [float(self.sigma)], [[1.0]])

    def _ssm_tangents(self):
        return [_leaf_tangent([-1.0 / float(self.scale) ** 2], [0.0], [[0.0]]),
                _leaf_tangent([0.0], [1.0], [[0.0]])]

    def _phi(self, dt):
        return np.exp(-np.asarray(dt, dtype=np.float64) / float(self.scale))[..., None, None]


class Matern32(_Leaf):
    """sigma^2 (1 + f tau) exp(-f tau), f = sqrt(3)/scale (reference ``quasisep.py:528-569``); J = 2."""

    def __init__(self, scale, sigma=1.0):
        self.scale, self.sigma = scale, sigma

    @property
    def _stationary(self):
        from tinygp_amd.kernels.stationary import Matern32 as M
        return M

    def noise(self):
        f = np.sqrt(3) / self.scale
        return 4 * f ** 3

    def design_matrix(self):
        f = np.sqrt(3) / self.scale
        return np.array([[0.0, 1.0], [-f * f, -2 * f]])

    def _ssm(self):
        f = np.sqrt(3) / float(self.scale)
        return _leaf_ssm(QS_M32, [f], [float(self.sigma), 0.0], np.diag([1.0, 3.0 / float(self.scale) ** 2]))

    def _ssm_tangents(self):
        sc = float(self.scale)
        return [_leaf_tangent([-np.sqrt(3) / sc ** 2], [0.0, 0.0], np.diag([0.0, -6.0 / sc ** 3])),
                _leaf_tangent([0.0], [1.0, 0.0], np.zeros((2, 2)))]

    def _phi(self, dt):
        dt = np.asarray(dt, dtype=np.float64)
        f = np.sqrt(3) / float(self.scale)
        fd = f * dt
        return _damped(fd, [[1 + fd, dt], [-f * fd, 1 - fd]])


class Matern52(_Leaf):
    """sigma^2 (1 + f tau + f^2 tau^2 / 3) exp(-f tau), f = sqrt(5)/scale (reference ``quasisep.py:572-633``)."""

    def __init__(self, scale, sigma=1.0):
        self.scale, self.sigma = scale, sigma

    @property
    def _stationary(self):
        from tinygp_amd.kernels.stationary import Matern52 as M
        return M

    def design_matrix(self):
        f = np.sqrt(5) / self.scale
        return np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-f ** 3, -3 * f ** 2, -3 * f]])

    def _ssm(self):
        f = np.sqrt(5) / float(self.scale)
        f2 = f * f
        P = np.array([[1.0, 0.0, -f2 / 3], [0.0, f2 / 3, 0.0], [-f2 / 3, 0.0, f2 * f2]])
        return _leaf_ssm(QS_M52, [f], [float(self.sigma), 0.0, 0.0], P)

    def _ssm_tangents(self):
        f = np.sqrt(5) / float(self.scale)
        df = -f / float(self.scale)
        dP = df * np.array([[0.0, 0.0, -2 * f / 3], [0.0, 2 * f / 3, 0.0], [-2 * f / 3, 0.0, 4 * f ** 3]])
        return [_leaf_tangent([df], np.zeros(3), dP), _leaf_tangent([0.0], [1.0, 0.0, 0.0], np.zeros((3, 3)))]

    def _phi(self, dt):
        d = np.asarray(dt, dtype=np.float64)
        f = np.sqrt(5) / float(self.scale)
        f2, fd, d2 = f * f, f * d, d * d
        return _damped(fd, [
            [0.5 * f2 * d2 + fd + 1, d * (fd + 1), 0.5 * d2],
            [-0.5 * f * f2 * d2, -f2 * d2 + fd + 1, 0.5 * d * (2 - fd)],
            [0.5 * f2 * f * d * (fd - 2), f2 * d * (fd - 3), 0.5 * f2 * d2 - 2 * fd + 1],
        ])


class Cosine(_Leaf):
    """sigma^2 cos(2 pi tau / scale) (reference ``quasisep.py:636-673``); J = 2."""

    def __init__(self, scale, sigma=1.0):
        self.scale, self.sigma = scale, sigma

    @property
    def _stationary(self):
        from tinygp_amd.kernels.stationary import Cosine as Cs
        return Cs

    def design_matrix(self):
        f = 2 * np.pi / self.scale
        return np.array([[0.0, -f], [f, 0.0]])

    def _ssm(self):
        return _leaf_ssm(QS_COS, [2 * np.pi / float(self.scale)], [float(self.sigma), 0.0], np.eye(2))

    def _ssm_tangents(self):
        return [_leaf_tangent([-2 * np.pi / float(self.scale) ** 2], [0.0, 0.0], np.zeros((2, 2))),
                _leaf_tangent([0.0], [1.0, 0.0], np.zeros((2, 2)))]

    def _phi(self, dt):
        a = 2 * np.pi / float(self.scale) * np.asarray(dt, dtype=np.float64)
        c, s = np.cos(a), np.sin(a)
        return _damped(np.zeros_like(a), [[c, -s], [s, c]])


class Celerite(_Leaf):
    """exp(-c tau) [a cos(d tau) + b sin(d tau)] (reference ``quasisep.py:343-401``); needs a c - b d > 0."""

    _params = ("a", "b", "c", "d")

    def __init__(self, a, b, c, d):
        self.a, self.b, self.c, self.d = a, b, c, d

    def design_matrix(self):
        return np.array([[-self.c, -self.d], [self.d, -self.c]])

    def _ssm(self):
        a, b, c, d = (float(v) for v in (self.a, self.b, self.c, self.d))
        c2, d2 = c * c, d * d
        s2 = c2 + d2
        h2_2 = d2 * (a * c - b * d) / (2 * c * s2)
        h2 = np.sqrt(h2_2)
        h1 = (c * h2 - np.sqrt(a * d2 - s2 * h2_2)) / d
        P = np.array([[1.0, -c / d], [-c / d, 1 + 2 * c2 / d2]])
        return _leaf_ssm(QS_CELERITE, [c, d], [h1, h2], P)

    def _ssm_tangents(self):
        a, b, c, d = (float(v) for v in (self.a, self.b, self.c, self.d))
        s2 = c * c + d * d
        num, den = d * d * (a * c - b * d), 2 * c * s2  # h2^2 = num / den
        H = num / den
        h2 = np.sqrt(H)
        root = np.sqrt(a * d * d - s2 * H)
        h1 = (c * h2 - root) / d
        # rows: d/da, d/db, d/dc, d/dd
        dnum = np.array([d * d * c, -d ** 3, d * d * a, 2 * a * c * d - 3 * b * d * d])
        dden = np.array([0.0, 0.0, 6 * c * c + 2 * d * d, 4 * c * d])
        dH = dnum / den - num * dden / den ** 2
        dh2 = dH / (2 * h2)
        dR = np.array([d * d, 0.0, -2 * c * H, 2 * a * d - 2 * d * H]) - s2 * dH
        dc, dd = np.array([0.0, 0.0, 1.0, 0.0]), np.array([0.0, 0.0, 0.0, 1.0])
        dh1 = (dc * h2 + c * dh2 - dR / (2 * root)) / d - h1 * dd / d
        dP = [np.zeros((2, 2)), np.zeros((2, 2)),
              np.array([[0.0, -1 / d], [-1 / d, 4 * c / d ** 2]]),
              np.array([[0.0, c / d ** 2], [c / d ** 2, -4 * c * c / d ** 3]])]
        return [_leaf_tangent([dc[i], dd[i]], [dh1[i], dh2[i]], dP[i]) for i in range(4)]

    def _phi(self, dt):
        dt = np.asarray(dt, dtype=np.float64)
        c, d = float(self.c), float(self.d)
        co, si = np.cos(d * dt), np.sin(d * dt)
        return _damped(c * dt, [[co, -si], [si, co]])


class SHO(_Leaf):
    """The damped, driven simple harmonic oscillator (reference ``quasisep.py:404-488``), J = 2, in its three
    regimes: quality > 1/2, == 1/2 (``np.allclose``, as the reference decides it) and < 1/2."""

    _params = ("omega", "quality", "sigma")

    def __init__(self, omega, quality, sigma=1.0):
        self.omega, self.quality, self.sigma = omega, quality, sigma

    def design_matrix(self):
        return np.array([[0.0, 1.0], [-self.omega ** 2, -self.omega / self.quality]])

    def _regime(self):
        q = float(self.quality)
        if np.allclose(q, 0.5):
            return QS_SHO_CRIT, 0.0
        if q > 0.5:
            return QS_SHO_UNDER, np.sqrt(max(4 * q * q - 1, 0.0))
        return QS_SHO_OVER, np.sqrt(max(1 - 4 * q * q, 0.0))

    def _ssm(self):
        kind, f = self._regime()
        w = float(self.omega)
        return _leaf_ssm(kind, [w, float(self.quality), f], [float(self.sigma), 0.0], np.diag([1.0, w * w]))

    def _ssm_tangents(self):
        """A critically damped oscillator (quality 0.5) sits on the boundary between two regimes with different
        transition formulas: it has no derivative with respect to ``quality`` there, and that entry is NaN (the
        gradient reports NaN for it); ``omega`` and ``sigma`` are exact."""
        kind, f = self._regime()
        w, q = float(self.omega), float(self.quality)
        if kind == QS_SHO_CRIT:
            dq = [np.nan, np.nan, np.nan]
        else:
            dq = [0.0, 1.0, (4 * q if kind == QS_SHO_UNDER else -4 * q) / f]
        z = np.zeros((2, 2))
        return [_leaf_tangent([1.0, 0.0, 0.0], [0.0, 0.0], np.diag([0.0, 2 * w])),
                _leaf_tangent(dq, [0.0, 0.0], z), _leaf_tangent([0.0], [1.0, 0.0], z)]

    def _phi(self, dt):
        dt = np.asarray(dt, dtype=np.float64)
        w, q = float(self.omega), float(self.quality)
        kind, f = self._regime()
        if kind == QS_SHO_CRIT:
            wd = w * dt
            return _damped(wd, [[1 + wd, dt], [-w * wd, 1 - wd]])
        arg = 0.5 * f * w * dt / q
        if kind == QS_SHO_UNDER:
            s, c, decay = np.sin(arg), np.cos(arg), 0.5 * w * dt / q
        else:
            # with a = w dt / 2q: s = e^-a sinh(arg), c = e^-a cosh(arg) from e^-(a - arg) and e^-2arg, both <= 1
            # (f < 1), never as e^-a cosh(arg) = 0 * inf beyond arg ~ 710.  a - arg = 2 w q dt / (1 + f) because
            # 1 - f^2 = 4 q^2 (no cancellation for small q); expm1 keeps s accurate for small arg.
            ep, em = np.exp(-2 * w * q * dt / (1 + f)), np.expm1(-2 * arg)
            s, c, decay = -0.5 * ep * em, 0.5 * ep * (2 + em), np.zeros_like(dt)
        return _damped(decay, [[c + s / f, 2 * q * s / (w * f)], [-2 * q * w * s / f, c - s / f]])


# -- the leaf table's transitions and their tangents on the host (twins of leaf_phi / leaf_dphi in csrc/qsep.hip) --------
def _rows(m):
    return np.moveaxis(np.asarray(m, dtype=np.float64), (0, 1), (-2, -1))


def _sho_modes(kind, p, dt):
    """S = e^-a sin(h)(arg), C = e^-a cos(h)(arg) and C - S (over-damped only), a = w dt / 2Q, arg = f a."""
    w, q, f = p[0], p[1], p[2]
    a = 0.5 * w * dt / q
    arg = f * a
    if kind == QS_SHO_UNDER:
        e = np.exp(-a)
        return a, arg, e * np.sin(arg), e * np.cos(arg), None
    ep, em = np.exp(-2 * w * q * dt / (1 + f)), np.expm1(-2 * arg)
    return a, arg, -0.5 * ep * em, 0.5 * ep * (2 + em), ep * (1 + em)


def leaf_phi(kind, p, dt):
    """A(dt) of one row ``(kind, p)`` of the leaf table: shape ``dt.shape + (j, j)``."""
    dt = np.asarray(dt, dtype=np.float64)
    kind = int(kind)
    if kind == QS_EXP:
        return np.exp(-p[0] * dt)[..., None, None]
    if kind in (QS_M32, QS_SHO_CRIT):
        f, fd = p[0], p[0] * dt
        return _damped(fd, [[1 + fd, dt], [-f * fd, 1 - fd]])
    if kind == QS_M52:
        f = p[0]
        f2, fd, d2 = f * f, f * dt, dt * dt
        return _damped(fd, [
            [0.5 * f2 * d2 + fd + 1, dt * (fd + 1), 0.5 * d2],
            [-0.5 * f * f2 * d2, -f2 * d2 + fd + 1, 0.5 * dt * (2 - fd)],
            [0.5 * f2 * f * dt * (fd - 2), f2 * dt * (fd - 3), 0.5 * f2 * d2 - 2 * fd + 1]])
    if kind in (QS_COS, QS_CELERITE):
        decay, om = (np.zeros_like(dt), p[0]) if kind == QS_COS else (p[0] * dt, p[1])
        co, si = np.cos(om * dt), np.sin(om * dt)
        return _damped(decay, [[co, -si], [si, co]])
    w, q, f = p[0], p[1], p[2]
    _, _, S, Cc, _ = _sho_modes(kind, p, dt)
    return _rows([[Cc + S / f, 2 * q * S / (w * f)], [-2 * q * w * S / f, Cc - S / f]])


def leaf_dphi(kind, p, dp, dt):
    """The derivative of :func:`leaf_phi` along the tangent ``dp`` of the row's parameters.  Every term carries a
    factor ``dt``.  Over-damped SHO: the same ``exp(-(a - b))`` / ``expm1(-2b)`` construction as the transition, the
    two nearly equal terms of d(e^-a sinh b) regrouped around e^-(a + b), so nothing overflows past b = 710."""
    dt = np.asarray(dt, dtype=np.float64)
    kind = int(kind)
    if kind == QS_EXP:
        return (-dt * np.exp(-p[0] * dt) * dp[0])[..., None, None]
    if kind in (QS_M32, QS_SHO_CRIT):
        f, fd = p[0], p[0] * dt
        return dp[0] * _damped(fd, [[-fd * dt, -dt * dt], [f * (fd - 2) * dt, (fd - 2) * dt]])
    if kind == QS_M52:
        f = p[0]
        f2, fd, d2 = f * f, f * dt, dt * dt
        v = [[0.5 * f2 * d2 + fd + 1, dt * (fd + 1), 0.5 * d2],
             [-0.5 * f * f2 * d2, -f2 * d2 + fd + 1, 0.5 * dt * (2 - fd)],
             [0.5 * f2 * f * dt * (fd - 2), f2 * dt * (fd - 3), 0.5 * f2 * d2 - 2 * fd + 1]]
        vf = [[f * d2 + dt, d2, np.zeros_like(dt)],
              [-1.5 * f2 * d2, -2 * f * d2 + dt, -0.5 * d2],
              [2 * f2 * f * d2 - 3 * f2 * dt, 3 * f2 * d2 - 6 * fd, f * d2 - 2 * dt]]
        return dp[0] * _damped(fd, [[vf[i][j] - dt * v[i][j] for j in range(3)] for i in range(3)])
    if kind in (QS_COS, QS_CELERITE):
        decay, om, dom, ddec = (np.zeros_like(dt), p[0], dp[0], 0.0) if kind == QS_COS else (p[0] * dt, p[1], dp[1],
                                                                                          dp[0])
        co, si = np.cos(om * dt), np.sin(om * dt)
        return _damped(decay, [[dt * (-dom * si - ddec * co), dt * (-dom * co + ddec * si)],
                               [dt * (dom * co - ddec * si), dt * (-dom * si - ddec * co)]])
    w, q, f = p[0], p[1], p[2]
    dw, dq, df = dp[0], dp[1], dp[2]
    a, arg, S, Cc, diff = _sho_modes(kind, p, dt)
    da = a * (dw / w - dq / q)
    darg = df * a + f * da
    if kind == QS_SHO_UNDER:
        dS, dC = -da * S + Cc * darg, -da * Cc - S * darg
    else:
        dd = da - darg
        dS, dC = -dd * S + diff * darg, -dd * Cc - diff * darg
    rel = df / f
    return _rows([[dC + (dS - S * rel) / f, 2 * q / (w * f) * (dS + S * (dq / q - dw / w - rel))],
                  [-2 * q * w / f * (dS + S * (dq / q + dw / w - rel)), dC - (dS - S * rel) / f]])


def model_dphi(ssm: SSM, dleaves, dt) -> np.ndarray:
    """The derivative of the whole model's A(dt) along ``dleaves`` (L, 4): the product rule over the leaves of the
    term that both states belong to.  Shape ``dt.shape + (J, J)``."""
    dt = np.asarray(dt, dtype=np.float64)
    J = ssm.J
    phi = [leaf_phi(row[0], row[1:], dt) for row in ssm.leaves]
    dphi = [leaf_dphi(row[0], row[1:], d, dt) if np.any(d != 0) else None for row, d in zip(ssm.leaves, dleaves)]
    out = np.zeros(dt.shape + (J, J))
    for r in range(J):
        for c in range(J):
            a, b = ssm.state_map[r], ssm.state_map[c]
            if np.any((a < 0) != (b < 0)):
                continue
            v, dv = np.ones(dt.shape), np.zeros(dt.shape)
            for l in np.nonzero(a >= 0)[0]:
                f = phi[l][..., a[l], b[l]]
                dv = dv * f + (v * dphi[l][..., a[l], b[l]] if dphi[l] is not None else 0.0)
                v = v * f
            out[..., r, c] = dv
    return out
