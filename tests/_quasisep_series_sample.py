"""Posterior draws for sets of series (``tgp_qsep_series_sample``): the need and split rule of ``csrc/qsep.hip`` restated
on the host, and the sets of the tests (test infrastructure; shared by ``test_quasisep_series_sample_cpu.py`` and
``test_gpu_4_quasisep_series_sample.py``).

DESIGN section 11, "Batches of series: posterior draws": a call runs as launch chains filled in the order given and, inside
a chain, as passes of columns, a function of (N_0 .. N_{B-1}, M_0 .. M_{B-1}, J, nrhs, test side wanted or not) alone.  If
``series_sample_fixed``, ``series_sample_cols`` or ``series_sample_split`` in ``csrc/qsep.hip`` change, this has to follow
by hand (the handle reports the chains and passes of a call, not the rule)."""
import functools
from typing import NamedTuple

import numpy as np

import _quasisep_sample_np as so
import _quasisep_series as qs
from _quasisep_series import CAP_DOUBLES, MAX_LEVELS, MAX_MEMBERS, MODEL_DOUBLES, extent

EXT_DOUBLES = 13  # sizeof(QExtent) / 8: the extent of a member's merged grid, which goes up with its chain
MAX_COLS = 64     # SAMPLE_MAX_COLS
BUDGET = CAP_DOUBLES - MAX_MEMBERS * MODEL_DOUBLES


def _levels(n):
    """The sizes of a series' MAX_LEVELS table levels summed, 1 beyond its own depth."""
    e = extent(n)
    return sum(e.levels) + MAX_LEVELS - len(e.levels)


def fixed(n, m, J):
    """Doubles of a chain's buffer that a series of n points with m test points takes whatever the columns: what the
    value takes (``_quasisep_series.need``), the extent of its merged grid (13), xt, sidx, order (m each), gt, gp
    (n + m each)."""
    return qs.need(n, J) + EXT_DOUBLES + 3 * m + 2 * (n + m)


def per_cols(n, m, J, c, want_test=True):
    """And for c columns of a pass: xi ((n + m) max(J, 2) per column; z and alpha take its place), f and eps at the data
    (n each), with the test side f at the test points (m); per group of 8 columns the scans' work space, 192 per element
    of the larger pyramid, the data's or the merged grid's."""
    return (c * ((n + m) * max(J, 2) + 2 * n + (m if want_test else 0))
            + -(-c // 8) * 192 * max(_levels(n), _levels(n + m)))


class Chain(NamedTuple):
    members: int
    cols: int    # per pass
    passes: int


def series_sample_split(lengths, counts, J, nrhs, want_test=True, budget=BUDGET):
    """The chains of a call: filled in the order given while every member fits with one column -- a chain ends at
    MAX_MEMBERS members or before the member that would take it past the cap -- then as many columns per pass as the rest
    of the cap holds: at most MAX_COLS, a multiple of 8 or below 8 by ones.  ``None``: a series does not fit alone with
    one column (the call is refused).  ``budget``: the cap less the models, for the hand-computed cases."""
    one = [fixed(n, m, J) + per_cols(n, m, J, 1, want_test) for n, m in zip(lengths, counts)]
    if any(x > budget for x in one):
        return None
    groups, used = [], 0
    for b, x in enumerate(one):
        if not groups or len(groups[-1]) == MAX_MEMBERS or used + x > budget:
            groups.append([])
            used = 0
        groups[-1].append(b)
        used += x
    chains = []
    for g in groups:
        def total(c):
            return sum(fixed(lengths[b], counts[b], J) + per_cols(lengths[b], counts[b], J, c, want_test) for b in g)
        cols = min(nrhs, MAX_COLS)
        while cols > 1 and total(cols) > budget:
            cols -= (cols % 8 or 8) if cols > 8 else 1
        chains.append(Chain(len(g), cols, -(-nrhs // cols)))
    return chains


# -- the sets of the GPU tests ---------------------------------------------------------------------------------------------------
# (n, m) per member; m None: the series' own points.  Both extents on their edges: chunks of 16 below 65 536 points, 64
# chunks end one scan level (G = 1024 | 1025; N = 1024 | 1025), last chunks of one step (17, 1025, 4097)
EDGE_SET = [(1, None), (1, 1), (15, 1), (16, 1), (17, 9), (1000, 24), (1000, 25), (1024, None), (1025, 300), (300, 0),
            (4097, 40)]
EDGE_CASES = ["matern32", "m32cos_plus_sho", "celerite4"]
EDGE_COLS = 9  # a ragged second column group
ORACLE_MEMBERS = {"matern32": 4, "m32cos_plus_sho": 5, "celerite4": 6}  # of EDGE_SET: (17, 9), (1000, 24), (1000, 25)
SMALL_SET = [(1, 1), (5, 3), (17, 9)]
DEEP_SET = [(65_537, 40), (40, 5)]


@functools.lru_cache(maxsize=None)
def problem(n, m):
    """``_quasisep_sample_np.problem`` (neighbours 0.02 apart) for a member (n, m); m None: no test points.  Read-only."""
    out = so.problem(n, 0 if m is None else m)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def normals(n, m, J, R, seed=0):
    """``(xi (n + m, J, R), eps (n, R))`` of a member, seeded by its shape.  Read-only."""
    g = n + (0 if m is None else m)
    rng = np.random.default_rng([n, g, J, R, seed])
    out = rng.standard_normal((g, J, R)), rng.standard_normal((n, R))
    for a in out:
        a.setflags(write=False)
    return out
