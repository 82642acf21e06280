"""Schedule option sets of the Cholesky's panel chain, shared by the GPU tests that run the factorisation under each
(test_gpu_0_kernels.py::test_panel_chain_variants_agree: the factor; test_gpu_8_fused_schedules.py: the fused
log-likelihood).  Context options by name (tgp_ctx_set_option); library defaults for the others.  And the schedule's
dry run under such a set (tgp_trace_factor), which needs no GPU."""
import ctypes as C

import numpy as np

from tinygp_amd import _ffi

PANEL_CHAIN_VARIANTS = [
    dict(chain_kernel=0, fused_step=1, gate_split=0), dict(chain_kernel=0, fused_step=1, gate_split=1),
    dict(chain_kernel=0, fused_step=1, gate_split=1, lookahead=0),
    dict(chain_kernel=0, fused_step=0, chain_reserve=0), dict(chain_kernel=0, fused_step=1, chain_reserve=256),
    dict(chain_kernel=0, sub_panel=512), dict(chain_kernel=0, sub_panel=256, first_split=4),
    dict(chain_kernel=0, nb_first=256), dict(chain_kernel=0, nb_first=512, sub_panel=512, lookahead=0),
    dict(chain_kernel=0, split_tail=1), dict(chain_kernel=0, split_tail=1, sub_panel=512, nb_first=768),
    dict(chain_kernel=0),
    # the persistent chain (the default): panel by panel only, without look-ahead, two
    # chain workgroups per compute unit, narrow panels + early share, a narrow first panel
    dict(chain_full_rows=0), dict(lookahead=0), dict(lookahead=0, chain_full_rows=0),
    dict(chain_lds_pad=0), dict(nb_outer=512, first_split=3, chain_full_rows=2048),
    dict(nb_first=256, chain_full_rows=1024), dict(first_split=0, chain_reserve=0),
    # round 5: update tasks on the 4x4x4 MFMA form with LDS-direct operands (measured, not the default); the
    # followers of a chain launch behind a stream wait-value / behind the whole launch
    # (default: the wall-clock-bounded one-wave poll kernel)
    dict(chain_fast_update=1), dict(chain_polls=3), dict(chain_polls=0),
    dict(chain_fast_update=1, chain_polls=3, chain_full_rows=0),
    # round 6 (measured, not the defaults): K-batched update tasks, everywhere and in the
    # one-launch tail only; the next panel's first diagonal block beside the gate
    dict(chain_batch=4, chain_batch_minrows=0), dict(chain_batch=4, chain_full_rows=8192),
    dict(chain_batch=8, chain_batch_lag=2, chain_batch_rowlag=3, chain_batch_minrows=0),
    dict(chain_gate_split=1), dict(chain_gate_split=1, chain_full_rows=0),
    # the merged schedule's prefix poll as a kernel of its own (default: inside the panel's potf2)
    dict(chain_polls=2), dict(chain_polls=2, chain_full_rows=0),
    # the chain of a panel sub-panel by sub-panel (measured, not the default: profiles/r06_i)
    dict(chain_sub_panel=512), dict(chain_sub_panel=256, chain_sub_role=0, chain_full_rows=0),
]


def option_id(opts):
    return "-".join(f"{k}{v}" for k, v in opts.items()) or "defaults"


def trace_options(n_pad, opts, fused):
    """The records of tgp_trace_factor with exactly these context options (library defaults for the others)."""
    lib = _ffi.load_library()
    cap = 48 * (n_pad // 128) + 256
    out = np.zeros(cap * 10, dtype=np.int64)
    n = C.c_int64()
    text = ",".join(f"{k}={v}" for k, v in opts.items())
    st = lib.tgp_trace_factor(n_pad, text.encode(), fused, out.ctypes.data_as(C.POINTER(C.c_int64)), cap, C.byref(n))
    assert st == 0, lib.tgp_last_error()
    return out[: n.value * 10].reshape(-1, 10).tolist()
