"""Packing a batch of quasiseparable models for ``tgp_qsep_logprob_batch`` (host only), and the entry point's ABI."""
import re
from pathlib import Path

import numpy as np
import pytest

from tinygp_amd import _device, _ffi
from tinygp_amd.kernels import quasisep as q

ROOT = Path(__file__).resolve().parent.parent


def _m32cos_plus_sho(scale, period, omega, quality):
    return q.Matern32(scale=scale) * q.Cosine(scale=period) + q.SHO(omega=omega, quality=quality)


def test_pack_stacks_each_members_lowering():
    ks = [_m32cos_plus_sho(1.5, 3.0, 2.0, 3.0), _m32cos_plus_sho(0.7, 2.2, 1.1, 1.4),
          _m32cos_plus_sho(4.0, 9.5, 0.3, 7.0)]
    leaves, smap, h, P = q.pack_batch(ks)
    J, L = ks[0]._lower_ssm().J, len(ks[0]._lower_ssm().leaves)
    assert leaves.shape == (3, L, 5) and smap.shape == (J, L) and h.shape == (3, J) and P.shape == (3, J, J)
    assert smap.dtype == np.int32 and leaves.dtype == h.dtype == P.dtype == np.float64
    for a in (leaves, smap, h, P):
        assert a.flags.c_contiguous
    for b, k in enumerate(ks):
        s = k._lower_ssm()
        assert np.array_equal(leaves[b], s.leaves)
        assert np.array_equal(smap, s.state_map)
        assert np.array_equal(h[b], s.h)
        assert np.array_equal(P[b], s.Pinf)
    assert not np.array_equal(leaves[0], leaves[1])


def test_damping_regimes_share_one_batch():
    ks = [q.SHO(omega=1.5, quality=quality) for quality in (3.0, 0.5, 0.3)]
    leaves, smap, h, P = q.pack_batch(ks)
    assert [int(v) for v in leaves[:, 0, 0]] == [q.QS_SHO_UNDER, q.QS_SHO_CRIT, q.QS_SHO_OVER]
    for k in ks:
        assert np.array_equal(k._lower_ssm().state_map, smap)


def test_structure_mismatch_names_the_member():
    with pytest.raises(ValueError, match=r"kernel 1 .*J = 3.*J = 2"):
        q.pack_batch([q.Matern32(1.0), q.Matern52(1.0)])
    with pytest.raises(ValueError, match=r"kernel 2 .*leaf"):  # J = 2 both, one leaf against two
        q.pack_batch([q.Matern32(1.0), q.Matern32(2.0), q.Exp(1.0) + q.Exp(2.0)])
    with pytest.raises(ValueError, match=r"kernel 1 .*state_map"):  # J = 3, two leaves, nested the other way round
        q.pack_batch([q.Exp(1.0) + q.Matern32(1.0), q.Matern32(1.0) + q.Exp(1.0)])
    with pytest.raises(ValueError, match="at least one"):
        q.pack_batch([])


def test_nine_states_exceed_the_device():
    k = q.Matern52(1.0) + q.Matern52(2.0) + q.Matern52(3.0)
    with pytest.raises(_device.DeviceLimit, match="J = 9"):
        q.pack_batch([q.Matern52(1.0) + q.Matern52(2.0) + q.Matern32(3.0), k])


def test_header_and_binding_declare_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tgp_hip.h").read_text(), flags=re.S)
    m = re.search(r"int\s+tgp_qsep_logprob_batch\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, "include/tgp_hip.h does not declare tgp_qsep_logprob_batch"
    params = [p.strip() for p in m.group(1).split(",")]
    sig = _ffi.SIGNATURES["tgp_qsep_logprob_batch"]
    assert len(params) == len(sig) == 15
    # the scalar arguments: their C types against the ctypes of the binding, by position
    import ctypes as C
    scalars = {i: (C.c_int32 if p.startswith("int32_t ") else C.c_int64)
               for i, p in enumerate(params) if "*" not in p}
    assert sorted(scalars) == [1, 3, 5, 9, 11]
    for i, ct in scalars.items():
        assert sig[i] is ct, (i, params[i])
    assert hasattr(_ffi.load_library(), "tgp_qsep_logprob_batch")
