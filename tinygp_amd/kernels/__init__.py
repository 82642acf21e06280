"""Kernel building blocks (mirror of ``tinygp.kernels`` for the dense hot path).

Kernels are built as sums and products of the stationary leaves below and of the
dot-product kernels ``DotProduct`` / ``Polynomial``, exactly as in the reference; calling
a kernel evaluates it on the MI355X through the HIP tile evaluator.  A bare
``DotProduct`` / ``Polynomial`` called directly is one host GEMM; inside a tree, a
transform or a solver it runs on the device.  ``Custom`` is an arbitrary Python function:
its matrix is evaluated on the host and handed to the solver through the
``covariance=`` channel (the factorisation still runs on the device).  The ``quasisep``
submodule holds the state-space kernels of 1-D series (``Exp``, ``Matern32``, ``Matern52``,
``Cosine``, ``Celerite``, ``SHO`` and their sums, products and scalings) that
``solvers.QuasisepSolver`` factors in O(N J^2) on the device.
"""

__all__ = [
    "Distance", "L1Distance", "L2Distance", "Kernel", "Conditioned", "Custom", "Sum",
    "Product", "Constant", "DotProduct", "Polynomial", "Stationary", "Exp", "ExpSquared", "Matern32", "Matern52", "Cosine",
    "ExpSineSquared", "RationalQuadratic", "quasisep",
]

from tinygp_amd.kernels.base import (
    Conditioned,
    Constant,
    Custom,
    DotProduct,
    Kernel,
    Polynomial,
    Product,
    Sum,
)
from tinygp_amd.kernels.distance import Distance, L1Distance, L2Distance
from tinygp_amd.kernels.stationary import (
    Cosine,
    Exp,
    ExpSineSquared,
    ExpSquared,
    Matern32,
    Matern52,
    RationalQuadratic,
    Stationary,
)

from tinygp_amd.kernels import quasisep  # noqa: E402
