"""Link recommendation (ocn_amd/recommend.py; ``ocn_row_diff_count`` / ``_fill``, ``ocn_segment_topk``) without a GPU: the
entries' argument checks, the limits they publish, and the refusals of the Python layers."""
from ctypes import c_void_p

import pytest
import torch

from ocn_amd import _lib

P = c_void_p(4096)             # a non-NULL address that is never read: every call below returns before its first HIP call
Z = c_void_p(0)


def test_new_entries_are_additions_to_abi_9(hiplib):
    for name in ("ocn_row_diff_stage_cols", "ocn_row_diff_count", "ocn_row_diff_fill", "ocn_segment_topk_max_k", "ocn_segment_topk"):
        assert name in _lib.SIGNATURES and hasattr(hiplib, name)
    assert hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9
    assert hiplib.ocn_segment_topk_max_k() >= 100                        # Hits@100 is the convention of half the datasets
    assert hiplib.ocn_row_diff_stage_cols() >= 64


def test_row_diff_entries_reject_bad_arguments_before_any_hip_call(hiplib):
    def count(**kw):
        a = dict(rpP=P, cP=P, rpM=P, cM=P, rows=P, Q=4, drop=1, count=P)
        a.update(kw)
        return hiplib.ocn_row_diff_count(a["rpP"], a["cP"], a["rpM"], a["cM"], a["rows"], a["Q"], a["drop"], a["count"], Z)

    def fill(**kw):
        a = dict(rpP=P, cP=P, rpM=P, cM=P, rows=P, Q=4, drop=1, off=P, edges=P)
        a.update(kw)
        return hiplib.ocn_row_diff_fill(a["rpP"], a["cP"], a["rpM"], a["cM"], a["rows"], a["Q"], a["drop"], a["off"], a["edges"], Z)

    for name in ("rpP", "cP", "rpM", "cM", "rows", "count"):
        assert count(**{name: Z}) == -1, name
    for name in ("rpP", "cP", "rpM", "cM", "rows", "off", "edges"):
        assert fill(**{name: Z}) == -1, name
    assert count(Q=-1) == -1 and fill(Q=-1) == -1
    assert count(Q=0, rows=Z) == -1 and fill(Q=0, off=Z) == -1           # (an empty call is still checked)
    assert count(Q=0) == 0 and fill(Q=0) == 0                            # ... and a valid one launches nothing


def test_segment_topk_entry_rejects_bad_arguments_before_any_hip_call(hiplib):
    kmax = hiplib.ocn_segment_topk_max_k()

    def topk(**kw):
        a = dict(scores=P, ptr=P, Q=4, k=10, val=P, pos=P)
        a.update(kw)
        return hiplib.ocn_segment_topk(a["scores"], a["ptr"], a["Q"], a["k"], a["val"], a["pos"], Z)

    for name in ("scores", "ptr", "val", "pos"):
        assert topk(**{name: Z}) == -1, name
    assert topk(Q=-1) == -1
    assert topk(k=0) == -1 and topk(k=-3) == -1 and topk(k=kmax + 1) == -1
    assert topk(Q=0, k=0) == -1 and topk(Q=0, ptr=Z) == -1
    assert topk(Q=0, k=1) == 0 and topk(Q=0, k=kmax) == 0


def _tiny():
    from ocn_amd.sparse import SparseTensor
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(4, 4))
    other = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(5, 5))
    return adj, other


def test_recommend_layer_raises_value_errors_on_misuse(hiplib):
    """``sources`` that is not 1-d int64, ``known`` / ``adj2`` of another size, ``k`` out of range: host-side errors, raised
    before anything touches a device (the adjacencies here live on the CPU)."""
    from ocn_amd import ops, recommend as R
    adj, other = _tiny()
    src = torch.tensor([0, 2])
    for bad in (src.int(), src.view(1, 2), src.view(2, 1), src.float(), [0, 2]):
        with pytest.raises(ValueError, match="sources must be a 1-d int64"):
            R.two_hop_candidates(adj, adj, bad)
        with pytest.raises(ValueError, match="sources must be a 1-d int64"):
            R.recommend_links_heuristic(adj, adj, bad, 3, 64, "cn")
    with pytest.raises(ValueError, match="known is"):
        R.two_hop_candidates(adj, adj, src, known=other)
    with pytest.raises(ValueError, match="adj2 is"):
        R.two_hop_candidates(adj, other, src)
    with pytest.raises(ValueError, match="known is"):
        R.recommend_links_heuristic(adj, adj, src, 3, 64, "cn", known=other)
    kmax = ops.segment_topk_max_k()
    assert kmax >= 100
    for k in (0, -1, kmax + 1):
        with pytest.raises(ValueError, match="k must be in 1"):
            R.segment_topk(torch.zeros(4), torch.tensor([0, 4]), k)
        with pytest.raises(ValueError, match="k must be in 1"):
            ops.segment_topk(torch.zeros(4), torch.tensor([0, 4]), k)
        with pytest.raises(ValueError, match="k must be in 1"):
            R.recommend_links_heuristic(adj, adj, src, k, 64, "cn")
    with pytest.raises(ValueError, match="unknown heuristic"):
        R.recommend_links_heuristic(adj, adj, src, 3, 64, "katz")


def test_recommend_links_guards_eval_mode_and_k(hiplib):
    from ocn_amd import recommend as R
    from ocn_amd.model import predictor_dict
    adj, _ = _tiny()
    src = torch.tensor([0, 2])
    pred = predictor_dict["cn5"](8, 8, 1, 3, 0.0)
    with pytest.raises(RuntimeError, match="eval path"):
        R.recommend_links(pred.train(), torch.randn(4, 8), adj, adj, src, 3, 64)
    with pytest.raises(ValueError, match="k must be in 1"):
        R.recommend_links(pred.eval(), torch.randn(4, 8), adj, adj, src, 0, 64)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        R.recommend_links(pred.eval(), torch.randn(4, 8), adj, adj, src, 3, 64)


def test_recommend_layer_refuses_cpu_tensors(hiplib):
    from ocn_amd import ops, recommend as R
    adj, _ = _tiny()
    src = torch.tensor([0, 2])
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        R.two_hop_candidates(adj, adj, src)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        R.recommend_links_heuristic(adj, adj, src, 3, 64, "ra")
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        R.segment_topk(torch.zeros(4), torch.tensor([0, 4]), 2)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.row_diff_count(adj._rowptr, adj._col, adj._rowptr, adj._col, src)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.row_diff_fill(adj._rowptr, adj._col, adj._rowptr, adj._col, src, torch.tensor([0, 1, 2]))


def test_op_wrappers_check_shapes_before_the_library(monkeypatch):
    """What the kernels index is bounded on the host: P and M with one row count (``rows`` is checked against it), one offset
    per query and the total."""
    from ocn_amd import ops
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    monkeypatch.setattr(ops, "validate_indices", False)
    rp3, rp2, col = torch.tensor([0, 1, 2, 2]), torch.tensor([0, 1, 2]), torch.tensor([1, 0], dtype=torch.int32)
    rows = torch.tensor([0, 1])
    with pytest.raises(ValueError, match="P has 3 rows, M 2"):
        ops.row_diff_count(rp3, col, rp2, col, rows)
    with pytest.raises(ValueError, match="P has 2 rows, M 3"):
        ops.row_diff_fill(rp2, col, rp3, col, rows, torch.tensor([0, 1, 2]))
    with pytest.raises(ValueError, match="off: one entry per query and the total"):
        ops.row_diff_fill(rp3, col, rp3, col, rows, torch.tensor([0, 1]))
    with pytest.raises(ValueError, match=r"ptr: \[Q \+ 1\] offsets"):
        ops.segment_topk(torch.zeros(4), torch.zeros(0, dtype=torch.int64), 2)
