"""Message saliency without a GPU: the refusals of ``explain_link_edges`` that happen before any device work,
``EdgeExplanation`` as a plain object, and the call counting of ``message_masks``."""
import io
from types import SimpleNamespace

import pytest
import torch

from ocn_amd import _lib


def tiny():
    from ocn_amd.model import GCN
    from ocn_amd.sparse import SparseTensor
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(3, 3))
    torch.manual_seed(0)
    return GCN(16, 16, 16, 2, 0.0, conv_fn="gcn").eval(), adj, torch.tensor([[0, 1], [1, 2]]), torch.randn(3, 16)


def test_explain_link_edges_refuses_before_any_device_work(hiplib, monkeypatch):
    from ocn_amd import ops
    from ocn_amd.explain import explain_link_edges
    from ocn_amd.model import GCN, predictor_dict
    model, adj, edges, x = tiny()
    cn5 = predictor_dict["cn5"](16, 16, 1, 3, 0.0).eval()
    # any device work would go through one of these
    for name in ("spmm_csr", "sddmm_csr", "deg_rsqrt", "cn_flags", "cn_gather", "segment_topk"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: pytest.fail(f"ops.{_n} was reached"))
    with pytest.raises(NotImplementedError, match="cn6"):
        explain_link_edges(model, predictor_dict["cn6"](16, 16, 1, 3, 0.0).eval(), x, adj, adj, edges, 0)
    with pytest.raises(TypeError):
        explain_link_edges(model, torch.nn.Linear(2, 2), x, adj, adj, edges, 0)
    with pytest.raises(RuntimeError, match="eval"):
        explain_link_edges(model, cn5.train(), x, adj, adj, edges, 0)
    cn5.eval()
    with pytest.raises(RuntimeError, match="model.eval"):
        explain_link_edges(model.train(), cn5, x, adj, adj, edges, 0)
    model.eval()
    cn5.set_edge_sharding(None, True)
    with pytest.raises(RuntimeError, match="sharded"):
        explain_link_edges(model, cn5, x, adj, adj, edges, 0)
    cn5.set_edge_sharding(None, False)
    for which in (-1, 2, 1.0, True, None):
        with pytest.raises(ValueError, match="which must be"):
            explain_link_edges(model, cn5, x, adj, adj, edges, which)
    limit = int(hiplib.ocn_segment_topk_max_k())
    for top in (0, -1, limit + 1, 2.0, True, None):
        with pytest.raises(ValueError, match="top must be"):
            explain_link_edges(model, cn5, x, adj, adj, edges, 0, top=top)
    for rank in ("abs", "", None, 1):
        with pytest.raises(ValueError, match="rank must be"):
            explain_link_edges(model, cn5, x, adj, adj, edges, 0, rank=rank)
    for bad in (edges[:0], edges[:, :1].contiguous(), torch.zeros(2, 3, dtype=torch.int64), edges.to(torch.int32), edges[0], [[0, 1]]):
        with pytest.raises(ValueError, match="edges"):
            explain_link_edges(model, cn5, x, adj, adj, bad, 0)
    with pytest.raises(ValueError, match="args"):
        explain_link_edges(model, predictor_dict["cn7"](16, 16, 1, 3, 0.0).eval(), x, adj, adj, edges, 0)
    with pytest.raises(ValueError, match="max aggregation"):
        explain_link_edges(GCN(16, 16, 16, 2, 0.0, conv_fn="max").eval(), cn5, x, adj, adj, edges, 0)
    with pytest.raises(ValueError, match="no message-passing layer"):
        explain_link_edges(GCN(16, 16, 16, 0, 0.0).eval(), cn5, x, adj, adj, edges, 0)
    assert not cn5.training and not model.training and cn5._frozen is None
    assert all(p.grad is None for p in list(cn5.parameters()) + list(model.parameters()))


def test_a_valid_request_on_cpu_tensors_reaches_the_device_layer(hiplib):
    from ocn_amd.explain import explain_link_edges
    from ocn_amd.model import predictor_dict
    model, adj, edges, x = tiny()
    for adj2 in (adj, None):
        with pytest.raises(_lib.OcnHipError, match="no CPU path"):
            explain_link_edges(model, predictor_dict["cn5"](16, 16, 1, 3, 0.0).eval(), x, adj, adj2, edges, 1, top=int(hiplib.ocn_segment_topk_max_k()))
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        explain_link_edges(model, predictor_dict["cn7"](16, 16, 1, 3, 0.0).eval(), x, adj, adj, edges, 0, args=SimpleNamespace(sum=1.0))


def test_edge_explanation_is_a_plain_dataclass_that_survives_torch_save():
    import dataclasses
    from ocn_amd.explain import EdgeExplanation
    top, L = 4, 2
    ex = EdgeExplanation(score=torch.tensor(0.25), entries=torch.tensor([[1, 0], [0, 1], [-1, -1], [-1, -1]]),
                         saliency=torch.tensor([0.5, -0.25, 0.0, 0.0]), per_layer=torch.randn(top, L), input_share=torch.randn(3),
                         flat=torch.randn(L, 2))
    assert dataclasses.is_dataclass(ex)
    names = [f.name for f in dataclasses.fields(ex)]
    assert names == ["score", "entries", "saliency", "per_layer", "input_share", "flat"]
    blob = io.BytesIO()
    torch.save(ex, blob)
    blob.seek(0)
    back = torch.load(blob)
    assert isinstance(back, EdgeExplanation)
    for name in names:
        assert torch.equal(getattr(back, name), getattr(ex, name)), name
    bare = EdgeExplanation(ex.score, ex.entries, ex.saliency, ex.per_layer)
    assert bare.input_share is None and bare.flat is None


def test_message_masks_counts_its_calls(monkeypatch):
    """The masks are dealt in call order to the ``_spmm`` calls on the context's adjacency — another adjacency is not counted —
    and a number of calls other than ``len(masks)`` raises on exit.  (``ops.spmm_csr`` is replaced by a dense product: this test
    is about the routing.)"""
    from ocn_amd import ops
    from ocn_amd.model import _spmm, message_masks
    from ocn_amd.sparse import SparseTensor
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(3, 3))
    other = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(3, 3))
    dense = torch.zeros(3, 3)
    dense[torch.tensor([0, 1, 1, 2]), torch.tensor([1, 0, 2, 1])] = 1.0
    seen = []
    monkeypatch.setattr(ops, "spmm_csr", lambda rowptr, col, x, **kw: (seen.append(col.numel()), dense @ x)[1])
    x = torch.randn(3, 16)
    masks = [torch.ones(4, requires_grad=True) for _ in range(2)]
    with message_masks(adj, masks) as ctx:
        y1 = _spmm(adj, x, mode="sum")
        assert not _spmm(other, x, mode="sum").requires_grad         # another adjacency: unmasked, not counted
        y2 = _spmm(adj, x, mode="sum")
        assert ctx.calls == 2
    assert y1.requires_grad and y2.requires_grad and seen == [4, 2, 4]
    assert y1.grad_fn is not y2.grad_fn
    with pytest.raises(RuntimeError, match="2 masks for 0"):
        with message_masks(adj, masks):
            pass
    with pytest.raises(RuntimeError, match="2 masks for 1"):
        with message_masks(adj, masks):
            _spmm(adj, x, mode="sum")
    with pytest.raises(RuntimeError, match="1 masks for 2"):
        with message_masks(adj, masks[:1]):
            _spmm(adj, x, mode="sum")
            assert not _spmm(adj, x, mode="sum").requires_grad       # one call too many: unmasked, reported on exit
    with pytest.raises(KeyError):                                       # an error of the body is not replaced by the count
        with message_masks(adj, masks):
            raise KeyError("body")
    assert message_masks._active is None
    with pytest.raises(RuntimeError, match="re-entrant"):
        with message_masks(adj, masks[:0]):
            with message_masks(adj, masks[:0]):
                pass
    assert message_masks._active is None
    assert not _spmm(adj, x, mode="sum").requires_grad                  # outside the context _spmm is unchanged
