"""Packing the tangents of a batch of quasiseparable models for ``tgp_qsep_grad_batch`` (host only), the entry point's
ABI, and the mirror of its split into member chains and direction passes against DESIGN's worked examples."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from tinygp_amd import _ffi
from tinygp_amd.kernels import quasisep as q

from _quasisep_grad_batch import Split, grad_split, layout

ROOT = Path(__file__).resolve().parent.parent


def _m32cos_plus_sho(scale, period, omega, quality):
    return q.Matern32(scale=scale) * q.Cosine(scale=period) + q.SHO(omega=omega, quality=quality)


def test_pack_stacks_each_members_tangents():
    ks = [_m32cos_plus_sho(1.5, 3.0, 2.0, 3.0), _m32cos_plus_sho(0.7, 2.2, 1.1, 1.4),
          _m32cos_plus_sho(4.0, 9.5, 0.3, 0.2)]
    dleaves, dh, dP, undefined = q.pack_batch_tangents(ks)
    ssm = ks[0]._lower_ssm()
    J, L, P = ssm.J, len(ssm.leaves), len(ks[0].parameters())
    assert dleaves.shape == (3, P, L, 4) and dh.shape == (3, P, J) and dP.shape == (3, P, J, J)
    assert undefined.shape == (3, P) and undefined.dtype == bool and not undefined.any()
    for a in (dleaves, dh, dP):
        assert a.dtype == np.float64 and a.flags.c_contiguous
    for b, k in enumerate(ks):
        for i, t in enumerate(k._ssm_tangents()):
            assert np.array_equal(dleaves[b, i], t.dleaves), (b, i)
            assert np.array_equal(dh[b, i], t.dh), (b, i)
            assert np.array_equal(dP[b, i], t.dPinf), (b, i)
    assert not np.array_equal(dP[0], dP[1])


def test_critically_damped_member_is_flagged_and_zeroed():
    """The quality of a critically damped SHO has no derivative: that member's entry alone is flagged."""
    ks = [q.SHO(omega=1.5, quality=quality) for quality in (3.0, 0.5, 0.3)]
    names = [attr for _, attr in ks[0].parameters()]
    iq = names.index("quality")
    dleaves, dh, dP, undefined = q.pack_batch_tangents(ks)
    want = np.zeros((3, len(names)), dtype=bool)
    want[1, iq] = True
    assert np.array_equal(undefined, want)
    assert not dleaves[1, iq].any() and not dh[1, iq].any() and not dP[1, iq].any()
    assert np.all(np.isfinite(dleaves)) and np.all(np.isfinite(dh)) and np.all(np.isfinite(dP))
    for b in (0, 2):
        t = ks[b]._ssm_tangents()[iq]
        assert np.array_equal(dleaves[b, iq], t.dleaves) and np.array_equal(dP[b, iq], t.dPinf)
        assert dleaves[b, iq].any() or dP[b, iq].any()


def test_parameter_count_mismatch_names_the_member():
    # J = 2 and one leaf both, so the structure agrees; Scale adds a parameter
    with pytest.raises(ValueError, match=r"kernel 2 .*3 parameters.*2"):
        q.pack_batch_tangents([q.Matern32(1.0), q.Matern32(2.0), 2.0 * q.Matern32(1.0)])
    with pytest.raises(ValueError, match="at least one"):
        q.pack_batch_tangents([])
    with pytest.raises(TypeError, match="kernel 1"):
        q.pack_batch_tangents([q.Matern32(1.0), object()])


def test_header_and_binding_declare_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tgp_hip.h").read_text(), flags=re.S)
    m = re.search(r"int\s+tgp_qsep_grad_batch\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "include/tgp_hip.h does not declare tgp_qsep_grad_batch"
    params = [p.strip() for p in m.group(1).split(",")]
    sig = _ffi.SIGNATURES["tgp_qsep_grad_batch"]
    assert len(params) == len(sig) == 23
    scalars = {i: (C.c_int32 if p.startswith("int32_t ") else C.c_int64) for i, p in enumerate(params) if "*" not in p}
    assert sorted(scalars) == [1, 3, 5, 9, 11, 12]
    for i, ct in scalars.items():
        assert sig[i] is ct, (i, params[i])
    assert hasattr(_ffi.load_library(), "tgp_qsep_grad_batch")
    assert _ffi.ABI_VERSION == 6 and "#define TGP_ABI_VERSION 6" in (ROOT / "include" / "tgp_hip.h").read_text()


# DESIGN section 11, "Batches of gradients": (N, J, P, B, own noise, own residual, vectors) -> the split
WORKED = [
    # 64 walkers over a short series: everything in one chain and one pass
    ((1 << 14, 2, 2, 64, True, False, True), Split(64, 2, 1, 1)),
    # J = 8, P = 16: the 64 members leave room for 3 directions each, 6 passes instead of 2
    ((1 << 14, 8, 16, 64, True, False, True), Split(64, 3, 1, 6)),
    # three long series: the cap, not the limit of 8, cuts the passes
    ((1 << 20, 8, 16, 3, True, True, True), Split(3, 2, 1, 8)),
    # 64 members at N = 2^20, J = 2: 9 per chain, one direction per pass
    ((1 << 20, 2, 2, 64, True, False, True), Split(9, 1, 8, 16)),
    # the member limit: 65 members are two chains
    ((40, 2, 2, 65, True, False, True), Split(64, 2, 2, 2)),
    # the value alone: no direction pass
    ((1 << 20, 8, 0, 64, True, True, False), Split(9, 0, 8, 0)),
    # one member beyond the cap, with and without the vectors
    ((12_000_000, 8, 16, 1, False, False, True), Split(0, 0, 0, 0)),
    ((12_000_000, 8, 16, 1, False, False, False), Split(0, 0, 0, 0)),
]


@pytest.mark.parametrize("args,want", WORKED)
def test_split_rule_reproduces_the_worked_examples(args, want):
    """Pins the Python mirror to DESIGN's worked examples, not to the device: it runs no native code.  The device's
    `grad_split` is tied to the mirror by the GPU tests that compare the chains and passes a call reports."""
    assert grad_split(*args) == want


def test_layout_formula_at_the_worked_sizes():
    """The buffer formula by hand at N = 2^14, J = 2, P = 2 (1 024 chunks of 16, S = 1 024 + 16), noise per member,
    residual shared, vectors wanted.  Like the test above this checks the mirror alone, against DESIGN's formula."""
    n, nc, S = 1 << 14, 1024, 1040
    fixed, per_member, per_dir = layout(n, 2, 2, True, False, True)
    assert fixed == 64 * (141 + 8 * 104) + n
    assert per_member == n + 4 * n + 128 * nc + 384 * S + 3 * nc + 3 + 4 + 2 * n
    assert per_dir == 3 * n + 192 * S + 2 * nc
    # what a split holds stays under the cap, and one more member or direction would not
    for args, split in WORKED:
        if not split.members:
            continue
        n, J, P, B, own_noise, own_resid, vectors = args
        fixed, per_member, per_dir = layout(n, J, P, own_noise, own_resid, vectors)
        assert fixed + split.members * (per_member + split.dirs * per_dir) <= (1 << 27)
        if P and split.dirs < min(P, 8):
            assert fixed + split.members * (per_member + (split.dirs + 1) * per_dir) > (1 << 27)
        if split.members < min(B, 64):
            assert fixed + (split.members + 1) * (per_member + (per_dir if P else 0)) > (1 << 27)
