"""The default schedule's launch records (tgp_trace_factor) at N = 16 384, kept so that a change of the schedule's
host logic that is meant to touch non-default options only can be shown to leave the default trace alone
(tests/test_schedule.py::test_default_schedule_trace_is_unchanged):

  * chain_n16384: the persistent chain's configuration of test_schedule.py, fused (trace(16384, ..., chain_kernel=1));
  * c2_fused / c2_factor: the library's defaults (bench.py's workload, config 2), with and without the fused solve.

Ten int64 per record: kind, stream, v[0..7].

    python tests/golden/make_golden_schedule.py      (needs the built library, no GPU)
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parents[1]))

import test_schedule as ts  # noqa: E402


def traces():
    return {
        "chain_n16384": ts.trace(16384, 1024, 1, 5, 1100, 3, 0, chain_kernel=1),
        "c2_fused": ts.trace_options(16384, {}, 1),
        "c2_factor": ts.trace_options(16384, {}, 0),
    }


if __name__ == "__main__":
    out = {k: np.asarray(v, dtype=np.int64) for k, v in traces().items()}
    np.savez_compressed(HERE / "schedule_traces.npz", **out)
    print({k: v.shape for k, v in out.items()})
