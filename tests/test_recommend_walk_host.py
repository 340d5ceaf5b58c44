"""Link recommendation without a materialised A² (``ocn_two_hop_diff_count`` / ``_fill``, ``adj2=None`` in
ocn_amd/recommend.py) without a GPU: the entries' argument checks, the window they publish, and the refusals of the Python
layers."""
from ctypes import c_void_p

import pytest
import torch

from ocn_amd import _lib

P = c_void_p(4096)             # a non-NULL address that is never read: every call below returns before its first HIP call
Z = c_void_p(0)


def test_two_hop_entries_are_additions_to_abi_9(hiplib):
    for name in ("ocn_two_hop_window_cols", "ocn_two_hop_diff_count", "ocn_two_hop_diff_fill"):
        assert name in _lib.SIGNATURES and hasattr(hiplib, name)
    assert hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9
    window = hiplib.ocn_two_hop_window_cols()
    assert window >= 64 and window % 64 == 0


def _count(lib, **kw):
    a = dict(rpA=P, cA=P, rpM=P, cM=P, n=100, rows=P, Q=4, drop=1, window=0, count=P)
    a.update(kw)
    return lib.ocn_two_hop_diff_count(a["rpA"], a["cA"], a["rpM"], a["cM"], a["n"], a["rows"], a["Q"], a["drop"], a["window"],
                                      a["count"], Z)


def _fill(lib, **kw):
    a = dict(rpA=P, cA=P, rpM=P, cM=P, n=100, rows=P, Q=4, drop=1, window=0, off=P, edges=P)
    a.update(kw)
    return lib.ocn_two_hop_diff_fill(a["rpA"], a["cA"], a["rpM"], a["cM"], a["n"], a["rows"], a["Q"], a["drop"], a["window"],
                                     a["off"], a["edges"], Z)


def test_two_hop_entries_reject_bad_arguments_before_any_hip_call(hiplib):
    for name in ("rpA", "cA", "rpM", "cM", "rows", "count"):
        assert _count(hiplib, **{name: Z}) == -1, name
    for name in ("rpA", "cA", "rpM", "cM", "rows", "off", "edges"):
        assert _fill(hiplib, **{name: Z}) == -1, name
    window = hiplib.ocn_two_hop_window_cols()
    for call in (_count, _fill):
        assert call(hiplib, Q=-1) == -1
        for n in (0, -5, 1 << 31, 1 << 40):
            assert call(hiplib, n=n) == -1, n
        for w in (-64, -1, 1, 63, 65, 100, window - 1, window + 64, 2 * window):
            assert call(hiplib, window=w) == -1, w
        # (an empty call is still checked) ... and a valid one launches nothing
        assert call(hiplib, Q=0, rows=Z) == -1 and call(hiplib, Q=0, n=0) == -1 and call(hiplib, Q=0, window=32) == -1
        assert call(hiplib, Q=0) == 0 and call(hiplib, Q=0, n=(1 << 31) - 1) == 0
        assert call(hiplib, Q=0, window=64) == 0 and call(hiplib, Q=0, window=window) == 0
    assert _count(hiplib, Q=0, count=Z) == -1 and _fill(hiplib, Q=0, off=Z) == -1 and _fill(hiplib, Q=0, edges=Z) == -1


def _tiny():
    from ocn_amd.sparse import SparseTensor
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(4, 4))
    other = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(5, 5))
    return adj, other


def test_two_hop_kinds_keep_refusing_a_missing_adj2(hiplib):
    from ocn_amd import recommend as R
    adj, _ = _tiny()
    src = torch.tensor([0, 2])
    for kind in ("cn2", "aa2", "ra2"):
        with pytest.raises(ValueError, match="adj2, which is None"):
            R.recommend_links_heuristic(adj, None, src, 3, 64, kind)
    with pytest.raises(ValueError, match="unknown heuristic"):
        R.recommend_links_heuristic(adj, None, src, 3, 64, "katz")


def test_walk_recommendation_guards_eval_mode_k_and_operands(hiplib):
    from ocn_amd import ops, recommend as R
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import score_edges_walk
    adj, other = _tiny()
    src = torch.tensor([0, 2])
    pred = predictor_dict["cn5"](8, 8, 1, 3, 0.0)
    h = torch.randn(4, 8)
    with pytest.raises(RuntimeError, match="eval path"):
        R.recommend_links(pred.train(), h, adj, None, src, 3, 64)
    with pytest.raises(RuntimeError, match="eval path"):
        score_edges_walk(pred.train(), h, adj, torch.tensor([[0, 2]]), 64)
    with pytest.raises(ValueError, match="k must be in 1"):
        R.recommend_links(pred.eval(), h, adj, None, src, 0, 64)
    with pytest.raises(ValueError, match=r"edges must be \[n, 2\]"):
        score_edges_walk(pred.eval(), h, adj, torch.tensor([[0], [2]]), 64)
    with pytest.raises(ValueError, match="sources must be a 1-d int64"):
        R.two_hop_candidates(adj, None, src.int())
    with pytest.raises(ValueError, match="known is"):
        R.two_hop_candidates(adj, None, src, known=other)
    # no CPU path: the 1-hop heuristic and the model both get as far as the first device operand
    for call in (lambda: R.two_hop_candidates(adj, None, src),
                 lambda: R.recommend_links_heuristic(adj, None, src, 3, 64, "ra"),
                 lambda: R.recommend_links(pred.eval(), h, adj, None, src, 3, 64),
                 lambda: ops.two_hop_diff_count(adj._rowptr, adj._col, adj._rowptr, adj._col, src),
                 lambda: ops.two_hop_diff_fill(adj._rowptr, adj._col, adj._rowptr, adj._col, src, torch.tensor([0, 1, 2]))):
        with pytest.raises(_lib.OcnHipError, match="no CPU path"):
            call()


def test_two_hop_op_wrappers_check_shapes_and_the_window_before_the_library(hiplib, monkeypatch):
    from ocn_amd import ops
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    monkeypatch.setattr(ops, "validate_indices", False)
    rp3, rp2, col = torch.tensor([0, 1, 2, 2]), torch.tensor([0, 1, 2]), torch.tensor([1, 0], dtype=torch.int32)
    rows = torch.tensor([0, 1])
    with pytest.raises(ValueError, match="P has 3 rows, M 2"):
        ops.two_hop_diff_count(rp3, col, rp2, col, rows)
    with pytest.raises(ValueError, match="off: one entry per query and the total"):
        ops.two_hop_diff_fill(rp3, col, rp3, col, rows, torch.tensor([0, 1]))
    for w in (-64, 32, 100, ops.two_hop_window_cols() + 64):
        with pytest.raises(ValueError, match="window_cols must be 0 or a multiple of 64"):
            ops.two_hop_diff_count(rp3, col, rp3, col, rows, window_cols=w)
        with pytest.raises(ValueError, match="window_cols must be 0 or a multiple of 64"):
            ops.two_hop_diff_fill(rp3, col, rp3, col, rows, torch.tensor([0, 1, 2]), window_cols=w)
