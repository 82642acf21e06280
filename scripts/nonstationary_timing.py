"""Wall-clock of one evaluation at fresh hyper-parameters (warm, N = 16 384, fp64, bench.py's inputs) for a tree with
a dot-product leaf, on the device route and on the host route it took before the DOT op existed, next to a
stationary tree of the same shape:

  1. 1.5**2 * ExpSquared(2.5) + 0.3 * DotProduct()   device program (DOT leaf): value, value-and-gradient
  2. the same kernel through the host route                host matrix through covariance=: value only
  3. 1.5**2 * ExpSquared(2.5) + 0.3 * Matern32(1.2)   device program: value, value-and-gradient

The host route is the one `Sum._host_matrix` took: the stationary operand and the constant as device matrices,
downloaded, the dot product as a host GEMM, K + noise uploaded again through `covariance=`.
"value" is DirectSolver.factor_log_probability(resid, kernel) with a new kernel object per call (assembly, Cholesky,
forward solve); "value+grad" adds log_probability_and_grad on that factor.  One line per row, then one JSON line.

  python scripts/nonstationary_timing.py [N] [reps]
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tinygp_amd import kernels, synthetic  # noqa: E402
from tinygp_amd.noise import Diagonal  # noqa: E402
from tinygp_amd.solvers import DirectSolver  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
X, y = synthetic.make_inputs(n, 1, "float64")
noise = Diagonal(diag=np.full(n, 0.01))


def dot_tree(i):
    return 1.5**2 * kernels.ExpSquared(2.5 + 1e-3 * i) + 0.3 * kernels.DotProduct()


def stationary_tree(i):
    return 1.5**2 * kernels.ExpSquared(2.5 + 1e-3 * i) + 0.3 * kernels.Matern32(1.2)


class HostRoute(kernels.Kernel):
    """`dot_tree` evaluated as before the DOT op: no device program, so the solver takes `kernel(X, X) + noise`."""

    def __init__(self, i):
        self.i = i

    def _lower(self, X):
        raise NotImplementedError("host route")

    def __call__(self, X1, X2=None):
        k1 = 1.5**2 * kernels.ExpSquared(2.5 + 1e-3 * self.i)
        A, B = np.asarray(X1), np.asarray(X2)
        dot = np.multiply.outer(A, B) if A.ndim == 1 else A @ B.T
        return k1(X1, X2) + kernels.Constant(0.3)(X1, X2) * dot


def timed(label, build, grad, count):
    s = DirectSolver(build(0), X, noise)
    r = np.ascontiguousarray(y)
    step = [0]

    def one():
        step[0] += 1
        v = s.factor_log_probability(r, build(step[0]))
        if grad:
            v, _ = s.log_probability_and_grad(r)
        return v

    for _ in range(2):
        one()
    t = []
    for _ in range(count):
        t0 = time.perf_counter()
        v = one()
        t.append(time.perf_counter() - t0)
    s.close()
    ms = 1e3 * np.median(t)
    print(f"{label:62s} {ms:10.2f} ms (median of {count}, min {1e3 * min(t):.2f})  ll {float(v):.6f}", flush=True)
    return ms


rows = {
    "dot_device_value": timed("1. ExpSquared + DotProduct, device, value", dot_tree, False, reps),
    "dot_device_value_grad": timed("1. ExpSquared + DotProduct, device, value+grad", dot_tree, True, reps),
    "dot_host_value": timed("2. ExpSquared + DotProduct, host matrix, value", HostRoute, False, max(3, reps // 3)),
    "stationary_value": timed("3. ExpSquared + Matern32, device, value", stationary_tree, False, reps),
    "stationary_value_grad": timed("3. ExpSquared + Matern32, device, value+grad", stationary_tree, True, reps),
}
# the two routes of row 1 / 2 at the same hyper-parameters
ll_dev = DirectSolver(dot_tree(0), X, noise).factor_log_probability(np.ascontiguousarray(y))
ll_host = DirectSolver(HostRoute(0), X, noise).factor_log_probability(np.ascontiguousarray(y))
print(f"log-likelihood at the first hyper-parameters: device {ll_dev:.10f}  host matrix {ll_host:.10f}  "
      f"relative difference {abs(ll_dev - ll_host) / abs(ll_host):.2e}", flush=True)
rows["ratio_value_1_over_3"] = rows["dot_device_value"] / rows["stationary_value"]
rows["ratio_value_grad_1_over_3"] = rows["dot_device_value_grad"] / rows["stationary_value_grad"]
rows["ratio_value_2_over_1"] = rows["dot_host_value"] / rows["dot_device_value"]
print(json.dumps({"n": n, **{k: round(v, 3) for k, v in rows.items()}, "ll_rel_diff_1_vs_2": abs(ll_dev - ll_host) / abs(ll_host)}))
