"""``ocn_cn_gather_pair_min_batch`` without a GPU: an addition to ABI 9, declared, bound, and a process-wide bound that a
call sets and returns the way ``ocn_cn_flags_pair_min_batch`` does."""
import os

from ocn_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pool_pair_bound_is_an_addition_to_abi_9(hiplib):
    hdr = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    assert "int64_t ocn_cn_gather_pair_min_batch(int64_t min_rows);" in hdr
    assert "ocn_cn_gather_pair_min_batch" in hdr[hdr.index("Later additions to 9"):hdr.index("#define OCN_ABI_VERSION")]
    assert "#define OCN_ABI_VERSION 9" in hdr and hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9
    assert "ocn_cn_gather_pair_min_batch" in _lib.SIGNATURES


def test_pool_pair_bound_is_set_and_returned(hiplib):
    default = hiplib.ocn_cn_gather_pair_min_batch(-1)                      # a negative argument only queries
    assert default == hiplib.ocn_cn_gather_pair_min_batch(-1) == 32768
    try:
        assert ops.gather_pair_min_batch(0) == default and ops.gather_pair_min_batch() == 0
        assert ops.gather_pair_min_batch(1 << 40) == 0 and ops.gather_pair_min_batch(-5) == 1 << 40
        assert hiplib.ocn_cn_flags_pair_min_batch(-1) == 32768              # (the intersection pass's bound is its own)
    finally:
        hiplib.ocn_cn_gather_pair_min_batch(default)
    assert hiplib.ocn_cn_gather_pair_min_batch(-1) == default
