"""The dense gradient at every tile count, with every tile of K^-1 weighted.

``log_probability_and_grad`` forms K^-1 explicitly (spd_inverse_lower, csrc/chol.hip: L^-1 by halves over aligned
blocks of 1, 2, 4, ... tiles -- per level the full pairs in one batch, a remainder pair with a shorter second block on
its own, a mirror pass --, then K^-1 = M M^T) and contracts it with dK/dtheta tile by tile (kgrad_tile_kernel and
sum_partials_kernel, csrc/kmat.hip).  Which blocks a level pairs depends on the binary expansion of the tile count, so
the cases run through EVERY count from 1 to 17 (every (nfull, rem) pattern up to a lone 17th tile), each with an exact
last tile and one of 65 rows, and 33 tiles, where the 1 089 partials per sum take sum_partials_kernel's loop round a
second time.

The inputs are the box of tests/_dense_grad_np.py: dK/dtheta does not die away from the diagonal, and the reference
asserts that every tile of K^-1 enters every parameter's sum with at least 100 bars of weight (10 in fp32; at 33
tiles, for the programs where single far tiles weigh less, that the partials past the first 1 024 do).  A tile of K^-1
that is wrong by a sign, or missing, moves the result by that much.  The reference is exact -- LAPACK's K^-1, analytic
dK/dtheta -- and the bars are the project's (tests/test_gpu_2_grad.py): ll 1e-8, kernel parameters 2e-6 of the largest
component, noise 1e-6, mean 1e-7; fp32 2e-3 and ll 5e-4.  tests/test_dense_grad_cpu.py runs the reference's conditions
at every case without a GPU."""
import numpy as np
import pytest

import _dense_grad_np as dg
from tinygp_amd import GaussianProcess, kernels

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", dg.GPU_CASES, ids=lambda c: "-".join(map(str, c)))
def test_gradient_with_every_tile_of_the_inverse_weighted(case):
    name, n, dtype = case
    X, diag, y = dg.inputs(n, dg.PROGRAMS[name][0], dtype)
    ref = dg.reference(name, n, dtype)
    gp = GaussianProcess(dg.kernel(name, kernels), X, diag=diag)
    ll, g = gp.log_probability_and_grad(y)
    assert gp.solver.info == 0 and np.isfinite(ll)
    assert gp.solver.dtype == np.dtype(dtype)
    assert len(g["kernel"]) == dg.N_KERNEL[name] == len(gp.kernel.parameters())
    got = np.asarray(g["kernel"], dtype=np.float64)
    if name == "linear":
        got = np.concatenate([got, np.asarray(g["transform"], dtype=np.float64)])
    else:
        assert g["transform"] is None
    assert got.shape == ref.g.shape
    worst = dg.errors(ref, ll, got, g["noise_diag"], g["mean"])
    print(f"{name} N={n} ({ref.nt} tiles) {dtype}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
          + f" of the bar; lightest tile {ref.min_tile:.4g} bars")
    dg.check(ref, ll, got, g["noise_diag"], g["mean"])
