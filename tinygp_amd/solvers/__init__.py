"""Solvers (mirror of ``tinygp.solvers``): the dense :class:`DirectSolver` on MI355X, and
:class:`QuasisepSolver`, the O(N J^2) state-space recurrences of ``kernels.quasisep`` on sorted
1-D inputs, also on the device (:class:`QuasisepSeriesSet`: many such series at once).  ``KalmanSolver`` is not provided.
"""

__all__ = ["Solver", "DirectSolver", "DistributedDirectSolver", "QuasisepSolver", "QuasisepSeriesSet"]

from tinygp_amd.solvers.direct import DirectSolver
from tinygp_amd.solvers.distributed import DistributedDirectSolver
from tinygp_amd.solvers.solver import Solver
from tinygp_amd.solvers.quasisep import QuasisepSeriesSet, QuasisepSolver
