"""CPU suite: the argument checks of ``ocn_heads_fused`` past the NULL-pointer check, and the size / count entries beside it.

tests/test_host.py::test_entries_reject_bad_arguments_before_any_launch stops at the first refusal of the entry (a NULL
pointer).  Here every pointer field holds a non-NULL host pointer, so the case under test is the one that refuses; every case
returns before the entry's first HIP call (heads.hip: ocn_heads_fused), so none needs a GPU."""
import ctypes

import pytest

from ocn_amd import _lib

E = -1                                                                # OCN_EINVAL


def _args(H=128, B=4, ldx=0, **over):
    """An OcnHeadsArgs whose every pointer field is a non-NULL host pointer (never dereferenced on these paths: scoring mode,
    so `dump` stays NULL unless a case sets it); ``over``: fields to overwrite, None = NULL."""
    one = ctypes.c_int64(0)
    p = ctypes.cast(ctypes.pointer(one), ctypes.c_void_p).value
    a = _lib.OcnHeadsArgs()
    for i in range(3):
        a.x[i] = a.p_first[i] = a.p_out[i] = p
    a.p_mid[0] = a.p_mid[1] = p
    a.vec = a.ranges = a.y_row_map = a.y = a.cpark = a.scratch = p
    a.dump = None
    a.H, a.B, a.ldx = H, B, ldx
    a.eps, a.ln, a.b_on_union = 1e-5, 1, 1
    for k, v in over.items():
        setattr(a, k, p if v == "p" else v)
    a._keep = one                                                     # the pointee lives as long as the struct
    return a


REFUSED = {
    "H=64": dict(H=64),                                               # widths the fused kernel is not built for
    "H=512": dict(H=512),
    "ldx=124<H": dict(ldx=124),
    "ldx=130 not a multiple of 4": dict(ldx=130),
    "dump with B=2": dict(B=2, dump="p", y=None),
    "neither y nor dump": dict(y=None),
    "y without cpark": dict(cpark=None),
    "B=-1": dict(B=-1),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_heads_fused_refuses(hiplib, case):
    a = _args(**REFUSED[case])
    assert hiplib.ocn_heads_fused(ctypes.byref(a), None) == E, case


def test_heads_fused_empty_batch_is_no_error(hiplib):
    """B = 0 returns 0 before any pointer is looked at and without a launch: with valid fields, and with every field NULL."""
    assert hiplib.ocn_heads_fused(ctypes.byref(_args(B=0)), None) == 0
    empty = _lib.OcnHeadsArgs()
    empty.H, empty.B = 128, 0
    assert hiplib.ocn_heads_fused(ctypes.byref(empty), None) == 0


@pytest.mark.parametrize("H", [128, 256])
def test_heads_size_and_count_entries(hiplib, H):
    assert hiplib.ocn_heads_const_bytes(H) == 2 * H * 32 * 4           # two shares of one wave's 32 rows
    assert hiplib.ocn_heads_scratch_bytes(H) >= 256 * 4 * 2 * H * 32 * 4      # 256 workgroups x 4 waves x two parked shares
    assert hiplib.ocn_heads_nvec() == 17
    assert hiplib.ocn_heads_nscal() == 16
