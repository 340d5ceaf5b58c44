"""Short lists beyond 128 (``ocn_segment_keep_best``, ``ops.segment_keep_best``, ``recommend.PathSums``) without a GPU: the
mirror the GPU tests compare against is itself checked against the documented order, the entry's argument checks, the
validation of the new stage, and the limits of the existing entry points, which stay."""
import math
import struct
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from ocn_amd import _lib
from tests import keep_mirror

P = c_void_p(4096)             # a non-NULL address that is never read: every call below returns before its first HIP call
Z = c_void_p(0)


def f32(bits: int) -> float:
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def test_the_mirror_orders_as_the_contract_says():
    """Higher score first, +0.0 == -0.0, ties to the lower position, NaN after every number (-inf included) and NaNs among
    themselves by position — stated as a plain Python sort, compared with the mirror's uint64 keys."""
    nan2 = f32(0xffc00001)                                               # a negative NaN with a payload
    vals = [0.0, -0.0, 1.5, float("inf"), float("nan"), -1.5, f32(1), -f32(1), f32(0x007fffff), -f32(0x007fffff), 0.0,
            float("-inf"), 1.5, 1.5, nan2, -0.0, 3.0e38, -3.0e38, float("inf"), float("-inf"), 1.5, -1.5, float("nan"), 2.0 ** -126,
            -0.0, 0.0, 1.5, -7.25, -7.25, 1e-45, -1e-45, 1.5]
    seg = np.array(vals, dtype=np.float32)
    want = sorted(range(len(vals)), key=lambda i: (1, 0.0, i) if math.isnan(seg[i]) else (0, -float(seg[i]), i))
    assert keep_mirror.order(seg).tolist() == want
    k = keep_mirror.keys(seg)
    assert len(set(k.tolist())) == len(vals) and int(k.min()) > 0        # distinct, and none is the empty key
    img = keep_mirror.image(seg)
    assert img[0] == img[1] == 0x80000000 and img[4] == img[14] == 0 and img[11] == 0x007fffff and img[3] == 0xff800000
    for m in (1, 3, 7, len(vals), len(vals) + 5):
        ptr_m, keep, cut = keep_mirror.keep_best(seg, np.array([0, len(vals)]), m)
        assert keep.tolist() == sorted(want[:m]) and ptr_m.tolist() == [0, min(m, len(vals))]
        assert int(cut[0]) == int(k[want[min(m, len(vals)) - 1]])
    ptr_m, keep, cut = keep_mirror.keep_best(seg, np.array([0, 0, 5, 5, len(vals)]), 2)
    assert ptr_m.tolist() == [0, 0, 2, 2, 4] and cut[0] == 0 and cut[2] == 0
    assert keep.tolist() == [2, 3] + sorted(int(p) + 5 for p in keep_mirror.order(seg[5:])[:2])


def test_the_entry_is_an_addition_to_abi_9(hiplib):
    assert "ocn_segment_keep_best" in _lib.SIGNATURES and hasattr(hiplib, "ocn_segment_keep_best")
    assert len(_lib.SIGNATURES["ocn_segment_keep_best"][1]) == 8
    assert hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9


def test_the_entry_rejects_bad_arguments_before_any_hip_call(hiplib):
    def keep(**kw):
        a = dict(scores=P, ptr=P, Q=4, m=300, ptr_m=P, pos=P, cut=Z)
        a.update(kw)
        return hiplib.ocn_segment_keep_best(a["scores"], a["ptr"], a["Q"], a["m"], a["ptr_m"], a["pos"], a["cut"], Z)

    for name in ("scores", "ptr", "ptr_m", "pos"):
        assert keep(**{name: Z}) == -1, name
        assert keep(**{name: Z}, cut=P) == -1, name
    assert keep(Q=-1) == -1
    assert keep(m=0) == -1 and keep(m=-5) == -1 and keep(m=1 << 31) == -1
    assert keep(Q=0, m=0) == -1 and keep(Q=0, ptr=Z) == -1 and keep(Q=0, ptr_m=Z) == -1 and keep(Q=0, pos=Z) == -1
    assert keep(Q=0) == 0 and keep(Q=0, m=1) == 0 and keep(Q=0, m=(1 << 31) - 1, cut=P) == 0


def test_the_op_checks_m_and_refuses_cpu_tensors(hiplib):
    from ocn_amd import ops
    scores, ptr = torch.zeros(4), torch.tensor([0, 4])
    for bad in (0, -1, True, 2.0, "3", None, 1 << 31):
        with pytest.raises(ValueError, match="m must be"):
            ops.segment_keep_best(scores, ptr, bad)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.segment_keep_best(scores, ptr, 300)


def test_path_sums_is_checked_on_construction_and_against_hops(hiplib):
    from ocn_amd import recommend as R
    for kind in ("jaccard", "pa", "", None, 3):
        with pytest.raises(ValueError, match="no path sum"):
            R.PathSums(kind, 300)
    for bad in (True, False, 300.0, 0, -4, "300", None, 1 << 31):
        with pytest.raises(ValueError, match="m must be"):
            R.PathSums("ra", bad)
    for bad in (-0.5, float("nan"), float("inf"), True, "0.5"):
        with pytest.raises(ValueError, match="decay must be"):
            R.PathSums("ra", 300, bad)
    st = R.PathSums("ra", 300)
    assert (st.kind, st.m, st.decay) == ("ra", 300, None) and st == R.PathSums("ra", 300) and R.PathSums("cn", 1).m == 1
    with pytest.raises(Exception):
        st.m = 5                                                         # frozen
    assert R._check_prefilter(st, 128, 2) is st and R._prefilter_m(st) == 300
    with pytest.raises(ValueError, match="needs decay"):
        R._check_prefilter(st, 10, 3)
    st3 = R.PathSums("aa", 1000, 0.5)
    assert R._check_prefilter(st3, 10, 3) is st3
    with pytest.raises(ValueError, match="decay belongs to hops=3"):
        R._check_prefilter(st3, 10, 2)
    union = R._check_prefilter(R.ShortListUnion(st, ("cn", 16)), 300, 2)
    assert isinstance(union, R.ShortListUnion) and union.stages == (st, ("cn", 16))
    with pytest.raises(ValueError, match="fewer than k = 301"):
        R._check_prefilter(R.ShortListUnion(st, ("cn", 16)), 301, 2)
    with pytest.raises(ValueError, match="needs decay"):
        R._check_prefilter(R.ShortListUnion(st), 1, 3)


def _tiny():
    from ocn_amd.sparse import SparseTensor
    return SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(4, 4))


def test_the_existing_limits_and_refusals_stay(hiplib):
    from ocn_amd import ops, recommend as R
    from ocn_amd.model import predictor_dict
    assert ops.segment_topk_max_k() == 128 and hiplib.ocn_mips_max_m() == hiplib.ocn_segment_topk_max_k()
    adj, src = _tiny(), torch.tensor([0, 2])
    pred = predictor_dict["cn5"](8, 8, 1, 3, 0.0).eval()
    h = torch.randn(4, 8)
    with pytest.raises(ValueError, match="m must be in 1..128"):
        R.recommend_links(pred, h, adj, adj, src, 3, 64, prefilter=("ra", 129))
    with pytest.raises(ValueError, match="m must be in 1..128"):
        R.prefilter_candidates(adj, src, "ra", 129)
    with pytest.raises(ValueError, match="m must be in 1..128"):
        R.RandomWalks(129, 64, 2)
    with pytest.raises(ValueError, match="k must be in 1..128"):
        ops.segment_topk(torch.zeros(4), torch.tensor([0, 4]), 129)
    with pytest.raises(ValueError, match="k must be in 1..128"):
        R.recommend_links(pred, h, adj, adj, src, 129, 64, prefilter=R.PathSums("ra", 300))      # a ranked top-k stays <= 128


def test_k_above_m_is_refused_and_a_long_stage_reaches_the_device_layer(hiplib):
    from ocn_amd import ranking, recommend as R
    from ocn_amd.model import predictor_dict
    adj, src = _tiny(), torch.tensor([0, 2])
    pred = predictor_dict["cn5"](8, 8, 1, 3, 0.0).eval()
    h = torch.randn(4, 8)
    with pytest.raises(ValueError, match="fewer than k = 6"):
        R.recommend_links(pred, h, adj, adj, src, 6, 64, prefilter=R.PathSums("ra", 5))
    with pytest.raises(ValueError, match="stage must be a PathSums"):
        R.prefilter_candidates_long(adj, src, ("ra", 300))
    with pytest.raises(ValueError, match="needs decay"):
        R.prefilter_candidates_long(adj, src, R.PathSums("ra", 300), hops=3)
    # the argument checks accept the stage: the first thing to object is the device layer
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        R.recommend_links(pred, h, adj, adj, src, 3, 64, prefilter=R.PathSums("ra", 300))
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        R.recommend_links(pred, h, adj, adj, src, 3, 64, prefilter=R.PathSums("ra", 300, 0.5), hops=3)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        R.prefilter_candidates_long(adj, src, R.PathSums("cn", 4096))
    truth = (torch.tensor([0, 1, 2]), torch.tensor([2, 0]))
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ranking.rank_links(pred, h, adj, adj, src, truth, 64, prefilter=R.PathSums("ra", 300))
