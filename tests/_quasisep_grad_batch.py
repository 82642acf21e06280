"""The split rule of ``tgp_qsep_grad_batch`` restated on the host (test infrastructure; shared by
``test_quasisep_grad_batch_cpu.py`` and ``test_gpu_4_quasisep_grad_batch.py``), and the members of the test batches.

DESIGN section 11, "Batches of gradients": a call runs as member chains x direction passes, a function of (N, J, P, B,
own or shared noise, own or shared residual, vectors wanted or not) alone.  If ``grad_split`` in ``csrc/qsep.hip``
changes, this has to follow by hand (the handle reports the counts of a call, not the rule)."""
from typing import NamedTuple

MODEL_DOUBLES = 141   # sizeof(QModel) / 8
DIR_DOUBLES = 104     # sizeof(QDir) / 8: 8 x 4 leaf tangents, 8 of h, 64 of P
MAX_MEMBERS = 64      # BATCH_MAX_MEMBERS
MAX_DIRS = 8          # GRAD_MAX_BATCH
CAP_DOUBLES = (1 << 30) // 8


class Split(NamedTuple):
    members: int   # per chain; 0: one member with one direction does not fit
    dirs: int      # per pass
    chains: int
    passes: int    # summed over the chains


def _chunks_and_levels(n):
    lc = 16
    while lc < 256 and lc * 4096 < n:
        lc *= 2
    nc = -(-n // lc)
    levels = [nc]
    while levels[-1] > 64:
        levels.append(-(-levels[-1] // 64))
    return nc, sum(levels)


def layout(n, J, P, own_noise, own_resid, vectors):
    """``(fixed, per member, per member and direction)`` in doubles."""
    nc, S = _chunks_and_levels(n)
    fixed = MAX_MEMBERS * (MODEL_DOUBLES + MAX_DIRS * DIR_DOUBLES) + (0 if own_noise else n) + (0 if own_resid else n)
    per_member = ((n if own_noise else 0) + (n if own_resid else 0) + n * (2 + J) + 128 * nc
                  + (384 if vectors else 256) * S + 3 * nc + 3 + 2 * P + (2 * n if vectors else 0))
    per_dir = n * (1 + J) + 192 * S + 2 * nc
    return fixed, per_member, per_dir


def grad_split(n, J, P, B, own_noise, own_resid, vectors):
    """As many members as fit with one direction each, then as many directions per pass as the rest holds."""
    fixed, per_member, per_dir = layout(n, J, P, own_noise, own_resid, vectors)
    budget = CAP_DOUBLES - fixed
    one = per_member + (per_dir if P else 0)
    if budget < one:
        return Split(0, 0, 0, 0)
    members = min(B, MAX_MEMBERS, budget // one)
    dirs = min(P, MAX_DIRS, (budget - members * per_member) // (members * per_dir)) if P else 0
    chains = -(-B // members)
    return Split(members, dirs, chains, chains * (-(-P // dirs) if P else 0))


def member(cases, q, name, b):
    """Case ``name`` with every parameter scaled by 1 + 0.04 b: member b of a batch (b = 0: the case itself)."""
    k = cases[name](q)
    for obj, attr in k.parameters():
        setattr(obj, attr, getattr(obj, attr) * (1.0 + 0.04 * b))
    return k


def member_noise(noise, b):
    return noise * (1.0 + 0.1 * b)
