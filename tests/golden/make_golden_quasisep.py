#!/usr/bin/env python
"""Golden values of the quasiseparable kernels, recorded from the reference itself.

    python tests/golden/make_golden_quasisep.py      (needs the reference tree; writes ref_quasisep.npz)

Imports the unmodified reference through ``oracle/refshim/make_ref_golden.import_reference()``.  The shim's
``jax.lax.cond`` is replaced, in this process only, by a scalar Python if / else so that every SHO regime is
evaluated.  Per case: the kernel matrix at sorted points, its diagonal, and the LAPACK log-likelihood of the matrix
plus the noise for a fixed residual.
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(HERE.parent))

from _quasisep_cases import CASES, data  # noqa: E402


def main():
    from oracle.refshim.make_ref_golden import import_reference

    tinygp = import_reference()
    import jax

    jax.lax.cond = lambda pred, f_true, f_false, *ops: f_true(*ops) if bool(pred) else f_false(*ops)
    q = tinygp.kernels.quasisep
    t, noise, r = data()
    out = {"t": t, "noise": noise, "r": r}
    for name, build in CASES.items():
        k = build(q)
        K = np.asarray(k(t, t), dtype=np.float64)
        out[f"{name}__K"] = K
        out[f"{name}__diag"] = np.asarray(k(t), dtype=np.float64)
        Kn = K + np.diag(noise)
        L = np.linalg.cholesky(Kn)
        z = np.linalg.solve(L, r)
        out[f"{name}__logp"] = np.float64(-0.5 * z @ z - np.sum(np.log(np.diag(L))) - 0.5 * len(t) * np.log(2 * np.pi))
    np.savez_compressed(HERE / "ref_quasisep.npz", **out)
    print(f"wrote {len(CASES)} cases at N = {len(t)}")


if __name__ == "__main__":
    main()
