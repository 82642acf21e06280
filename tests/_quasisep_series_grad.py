"""Value and gradient for sets of series (``tgp_qsep_series_grad``): the split rule of ``csrc/qsep.hip`` restated on the
host (test infrastructure; shared by ``test_quasisep_series_grad_cpu.py`` and ``test_gpu_4_quasisep_series_grad.py``).

DESIGN section 11, "Batches of series: value and gradient": a call runs as launch chains filled in the order given, each
with direction passes of its own width, a function of (N_0 .. N_{B-1}, J, P, vectors wanted or not) alone.  If
``series_grad_split`` or the ``series_grad_*`` needs in ``csrc/qsep.hip`` change, this has to follow by hand (the handle
reports the chains and passes of a call, not the rule)."""
from _quasisep_grad_batch import DIR_DOUBLES, MAX_DIRS
from _quasisep_series import CAP_DOUBLES, MAX_LEVELS, MAX_MEMBERS, MODEL_DOUBLES, extent

FIXED = MAX_MEMBERS * MODEL_DOUBLES + MAX_MEMBERS * MAX_DIRS * DIR_DOUBLES  # models + one pass's directions
BUDGET = CAP_DOUBLES - FIXED


def parts(n, J, P, vectors):
    """``(member, dir)``: the doubles of a chain's buffer that a series of n points takes whatever the pass, and per
    direction of a pass.  member: noise, residual, c, z (n each), w (n J), both primal scans' chunk prefixes (2 x 64 per
    chunk), the scan work space (256 per element of MAX_LEVELS levels, 384 with the vectors), per-chunk sums of log c
    and z^2 and bad-pivot slots, results (3 + 2 P), with the vectors alpha and the noise gradient (n each).  dir: dc, dw
    (n (1 + J)), the tangent scans' work space (192 per element), two per-chunk sums."""
    e = extent(n)
    s4 = sum(e.levels) + MAX_LEVELS - len(e.levels)
    member = (n * (4 + J) + 128 * e.nchunks + (384 if vectors else 256) * s4 + 3 * e.nchunks + 3 + 2 * P
              + (2 * n if vectors else 0))
    return member, n * (1 + J) + 192 * s4 + 2 * e.nchunks


def series_grad_split(lengths, J, P, vectors):
    """``[(members, d, passes), ...]`` per chain: filled in the order given, a chain ends at MAX_MEMBERS members or
    before the member that would take the sum of member + [P > 0] dir past the budget; then d = min(P, MAX_DIRS, (budget
    - sum member) // sum dir) directions per pass.  ``None``: a series does not fit alone (the call is refused)."""
    one = [sum(parts(n, J, P, vectors)[:2 if P else 1]) for n in lengths]
    if any(x > BUDGET for x in one):
        return None
    chains, used = [], 0
    for n, x in zip(lengths, one):
        if not chains or len(chains[-1]) == MAX_MEMBERS or used + x > BUDGET:
            chains.append([])
            used = 0
        chains[-1].append(n)
        used += x
    out = []
    for chain in chains:
        member = sum(parts(n, J, P, vectors)[0] for n in chain)
        dirs = sum(parts(n, J, P, vectors)[1] for n in chain)
        d = min(P, MAX_DIRS, (BUDGET - member) // dirs) if P else 0
        out.append((len(chain), d, -(-P // d) if P else 0))
    return out
