"""Sets of series on coordinates of their own (``tgp_qsep_series_logprob``): the extent and split rules of
``csrc/qsep.hip`` restated on the host, and the series of the tests (test infrastructure; shared by
``test_quasisep_series_cpu.py`` and ``test_gpu_4_quasisep_series.py``).

DESIGN section 11, "Batches of series": a series' chunk length, chunk count and scan levels are functions of its own
length; a call runs as launch chains filled in the order given, a function of (N_0 .. N_{B-1}, J) alone.  If
``chunk_length``, ``series_need`` or ``series_split`` in ``csrc/qsep.hip`` change, this has to follow by hand (the
handle reports the number of chains of a call, not the rule)."""
import functools
from typing import NamedTuple

import numpy as np

MODEL_DOUBLES = 141   # sizeof(QModel) / 8
MAX_MEMBERS = 64      # BATCH_MAX_MEMBERS
MAX_LEVELS = 4        # MAXLEV: scan levels the extent table holds per series
CAP_DOUBLES = (1 << 30) // 8


class Extent(NamedTuple):
    lc: int        # steps per chunk
    nchunks: int
    levels: tuple  # the scan's own level sizes, levels[0] == nchunks


def extent(n):
    lc = 16
    while lc < 256 and lc * 4096 < n:
        lc *= 2
    nc = -(-n // lc)
    levels = [nc]
    while levels[-1] > 64:
        levels.append(-(-levels[-1] // 64))
    return Extent(lc, nc, tuple(levels))


def need(n, J):
    """Doubles of a chain's buffer that a series of n points takes: noise, residual, c, z (n each), w (n J), the scan
    work space (256 per element of MAX_LEVELS levels, 1 element beyond the series' own depth), per-chunk sums of log c
    and z^2 and bad-pivot slots (nchunks each), results (3)."""
    e = extent(n)
    work = 256 * (sum(e.levels) + MAX_LEVELS - len(e.levels))
    return n * (4 + J) + work + 3 * e.nchunks + 3


def series_split(lengths, J):
    """The members of every chain: filled in the order given, a chain ends at MAX_MEMBERS members or before the member
    whose need would take it past the cap.  ``None``: a series does not fit alone (the call is refused)."""
    budget = CAP_DOUBLES - MAX_MEMBERS * MODEL_DOUBLES
    if any(need(n, J) > budget for n in lengths):
        return None
    chains, used = [], 0
    for n in lengths:
        if not chains or chains[-1] == MAX_MEMBERS or used + need(n, J) > budget:
            chains.append(0)
            used = 0
        chains[-1] += 1
        used += need(n, J)
    return chains


@functools.lru_cache(maxsize=None)
def series(n, seed=None):
    """``(t, noise, resid)`` of the generator of ``test_gpu_4_quasisep_batch.py``, seeded by the length unless told."""
    rng = np.random.default_rng(n if seed is None else seed)
    t = np.sort(rng.uniform(0, 0.05 * n + 1, n))
    out = t, rng.uniform(0.05, 0.2, n), rng.standard_normal(n)
    for a in out:
        a.setflags(write=False)
    return out


# the sets of the GPU tests: (case names, lengths)
EDGE_LENGTHS = [1, 15, 16, 17, 1024, 1025, 4097]
EDGE_CASES = ["exp", "matern32", "m32cos_plus_sho", "celerite4"]
MIXED_LENGTHS = [65_537, 40, 262_145, 1]
DEEP_LENGTHS = [(1 << 20) + 1, 40, 65_537, 1]
MIXED_CASES = ["matern32", "celerite4"]
COMPANY_LENGTHS = [3, 64, 1025, 300]
PROBE_LENGTH, PROBE_CASE = 257, "m32cos_plus_sho"
