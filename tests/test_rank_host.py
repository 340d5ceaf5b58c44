"""Ranking held-out links (ocn_amd/ranking.py on ``ocn_segment_rank``) without a GPU: the entry's declaration and argument
checks, the refusals of the Python layers, and ``ranking_metrics`` on hand-written results against values worked out here."""
import math
import os
import re
from ctypes import c_void_p

import pytest
import torch

from ocn_amd import _lib

P = c_void_p(4096)             # a non-NULL address that is never read: every call below returns before its first HIP call
Z = c_void_p(0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segment_rank_is_an_addition_to_abi_9(hiplib):
    assert "ocn_segment_rank" in _lib.SIGNATURES and hasattr(hiplib, "ocn_segment_rank")
    assert hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9
    with open(os.path.join(ROOT, "include", "ocn_hip.h")) as f:
        text = f.read()
    decl = re.search(r"^int ocn_segment_rank\(([^;]*)\);", text, re.M)
    assert decl, "ocn_segment_rank is not declared in include/ocn_hip.h"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert [p.rsplit(" ", 1)[-1].lstrip("*") for p in params] == ["scores", "ptr", "edges", "Q", "tptr", "tnode", "P", "rank", "pos", "stream"]
    res, args = _lib.SIGNATURES["ocn_segment_rank"]
    assert res is _lib.c_int32 and len(args) == len(params)
    for p, a in zip(params, args):                                       # pointers are pointers, sizes are int64
        assert (a is _lib.c_void_p) == ("*" in p) and (a is _lib.c_int64) == p.startswith("int64_t ")
    history = text[text.index("ABI history"):text.index("#define OCN_ABI_VERSION")]
    assert "ocn_segment_rank" in history[history.index("Later additions to 9"):]
    assert "#define OCN_ABI_VERSION 9" in text


def test_segment_rank_entry_rejects_bad_arguments_before_any_hip_call(hiplib):
    def rank(**kw):
        a = dict(scores=P, ptr=P, edges=P, Q=4, tptr=P, tnode=P, P=6, rank=P, pos=P)
        a.update(kw)
        return hiplib.ocn_segment_rank(a["scores"], a["ptr"], a["edges"], a["Q"], a["tptr"], a["tnode"], a["P"], a["rank"], a["pos"], Z)

    for name in ("scores", "ptr", "edges", "tptr", "tnode", "rank", "pos"):
        assert rank(**{name: Z}) == -1, name
        assert rank(Q=0, **{name: Z}) == -1 and rank(P=0, **{name: Z}) == -1, name     # (an empty call is still checked)
    assert rank(Q=-1) == -1 and rank(P=-1) == -1 and rank(Q=-1, P=0) == -1 and rank(Q=0, P=-1) == -1
    assert rank(Q=0) == 0 and rank(P=0) == 0 and rank(Q=0, P=0) == 0                   # ... and a valid one launches nothing


def _tiny():
    from ocn_amd.sparse import SparseTensor
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(4, 4))
    other = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(5, 5))
    return adj, other


def _public_calls(adj, src, truth, known=None):
    """The three public functions on one request, as thunks."""
    from ocn_amd import ranking as K
    from ocn_amd.model import predictor_dict
    pred = predictor_dict["cn5"](8, 8, 1, 3, 0.0).eval()
    h = torch.randn(4, 8)
    return {"rank_links": lambda: K.rank_links(pred, h, adj, adj, src, truth, 64, known=known),
            "rank_links_heuristic": lambda: K.rank_links_heuristic(adj, adj, src, truth, 64, "cn", known=known),
            "rank_path_index": lambda: K.rank_path_index(adj, src, truth, "ra", 2, known=known)}


def test_public_functions_raise_value_errors_on_misuse(hiplib):
    """Host-side errors, raised before anything touches a device (everything here lives on the CPU)."""
    from ocn_amd import ranking as K
    from ocn_amd.model import predictor_dict
    adj, other = _tiny()
    src = torch.tensor([0, 2])
    good = (torch.tensor([0, 1, 2]), torch.tensor([2, 0]))
    for bad in (src.int(), src.view(1, 2), src.float(), [0, 2]):
        for name, call in _public_calls(adj, bad, good).items():
            with pytest.raises(ValueError, match="sources must be a 1-d int64"):
                call()
    for name, call in _public_calls(adj, src, other).items():            # a truth of another size
        with pytest.raises(ValueError, match="truth is"):
            call()
    for name, call in _public_calls(adj, src, good, known=other).items():
        with pytest.raises(ValueError, match="known is"):
            call()
    for tptr in (torch.tensor([0, 2]), torch.tensor([0, 1, 2, 2])):      # a tptr of the wrong length
        for name, call in _public_calls(adj, src, (tptr, good[1])).items():
            with pytest.raises(ValueError, match="tptr has"):
                call()
    for bad in ((good[0].int(), good[1]), (good[0], good[1].int()), (good[0].view(3, 1), good[1]), (good[0], good[1].view(1, 2)),
                (good[0],), "truth", None, ([0, 1, 2], [2, 0])):
        for name, call in _public_calls(adj, src, bad).items():
            with pytest.raises(ValueError, match="truth"):
                call()
    for tptr in (torch.tensor([0, 1, 3]), torch.tensor([1, 1, 2]), torch.tensor([0, 3, 2])):   # not the offsets of tnode
        for name, call in _public_calls(adj, src, (tptr, good[1])).items():
            with pytest.raises(ValueError, match="tptr must ascend from 0"):
                call()
    pred = predictor_dict["cn5"](8, 8, 1, 3, 0.0).eval()
    h = torch.randn(4, 8)
    for pf, hops in ((("ra", 5, 0.5), 2), (("ra", 5), 3), (("pa", 5), 2), (("ra", 0), 2), ("ra", 2)):
        with pytest.raises(ValueError):
            K.rank_links(pred, h, adj, adj, src, good, 64, prefilter=pf, hops=hops)
    with pytest.raises(ValueError, match="hops must be 2 or 3"):
        K.rank_links(pred, h, adj, adj, src, good, 64, hops=4)
    with pytest.raises(ValueError, match="hops must be 2 or 3"):
        K.rank_links_heuristic(adj, adj, src, good, 64, "cn", hops=1)
    with pytest.raises(ValueError, match="unknown heuristic"):
        K.rank_links_heuristic(adj, adj, src, good, 64, "katz")
    with pytest.raises(ValueError, match="cn6 needs adj2"):
        K.rank_links(predictor_dict["cn6"](8, 8, 1, 3, 0.0).eval(), h, adj, None, src, good, 64)
    with pytest.raises(ValueError, match="is no path sum"):
        K.rank_path_index(adj, src, good, "jaccard", 2)
    with pytest.raises(ValueError, match="hops must be 2 or 3"):
        K.rank_path_index(adj, src, good, "ra", 4)
    with pytest.raises(ValueError, match="decay must be"):
        K.rank_path_index(adj, src, good, "ra", 3)                       # decay has no default
    with pytest.raises(ValueError, match="decay must be"):
        K.rank_path_index(adj, src, good, "ra", 3, decay=-1.0)
    with pytest.raises(ValueError, match="budget must be"):
        K.rank_path_index(adj, src, good, "ra", 3, decay=0.5, budget=0)
    with pytest.raises(ValueError, match="belong to hops=3"):
        K.rank_path_index(adj, src, good, "ra", 2, decay=0.5)
    with pytest.raises(ValueError, match="belong to hops=3"):
        K.rank_path_index(adj, src, good, "ra", 2, budget=100)


def test_training_mode_and_cpu_tensors_are_refused(hiplib):
    from ocn_amd import ops, ranking as K
    from ocn_amd.model import predictor_dict
    adj, _ = _tiny()
    src = torch.tensor([0, 2])
    good = (torch.tensor([0, 1, 2]), torch.tensor([2, 0]))
    pred = predictor_dict["cn5"](8, 8, 1, 3, 0.0)
    with pytest.raises(RuntimeError, match="eval path"):
        K.rank_links(pred.train(), torch.randn(4, 8), adj, adj, src, good, 64)
    with pytest.raises(RuntimeError, match="eval path"):                 # ... before anything else is looked at
        K.rank_links(pred.train(), torch.randn(4, 8), adj, adj, src.int(), None, 64)
    for truth in (good, adj):
        for name, call in _public_calls(adj, src, truth).items():
            with pytest.raises(_lib.OcnHipError, match="no CPU path"):
                call()
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        K.rank_path_index(adj, src, good, "cn", 3, decay=0.5, budget=10)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.segment_rank(torch.zeros(2), torch.tensor([0, 2]), torch.tensor([[0, 1], [0, 2]]), torch.tensor([0, 1]), torch.tensor([2]))


def test_segment_rank_wrapper_checks_shapes_before_the_library(monkeypatch):
    """What the kernel indexes is bounded on the host.  ``_req`` itself — the device, dtype, dimension and contiguity check of
    every wrapper — is replaced here by its dtype and dimension half, since the tensors live on the CPU."""
    from ocn_amd import ops

    def req(t, dtype, name, ndim=None):
        if t.dtype != dtype:
            raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
        if ndim is not None and t.dim() != ndim:
            raise ValueError(f"{name}: expected {ndim}-d, got shape {tuple(t.shape)}")
        return t
    monkeypatch.setattr(ops, "_req", req)
    sc, ptr, ed = torch.zeros(3), torch.tensor([0, 1, 3]), torch.tensor([[0, 1], [2, 0], [2, 3]])
    tptr, tnode = torch.tensor([0, 1, 2]), torch.tensor([1, 3])
    for name, args in (("scores", (sc.view(1, 3), ptr, ed, tptr, tnode)), ("ptr", (sc, ptr.view(3, 1), ed, tptr, tnode)),
                       ("edges", (sc, ptr, ed.reshape(-1), tptr, tnode)), ("tptr", (sc, ptr, ed, tptr.view(1, 3), tnode)),
                       ("tnode", (sc, ptr, ed, tptr, tnode.view(2, 1)))):
        with pytest.raises(ValueError, match=f"{name}: expected"):
            ops.segment_rank(*args)
    for name, args in (("scores", (sc.double(), ptr, ed, tptr, tnode)), ("ptr", (sc, ptr.int(), ed, tptr, tnode)),
                       ("edges", (sc, ptr, ed.int(), tptr, tnode)), ("tptr", (sc, ptr, ed, tptr.int(), tnode)),
                       ("tnode", (sc, ptr, ed, tptr, tnode.int()))):
        with pytest.raises(TypeError, match=f"{name}: expected"):        # (a dtype is a TypeError in every wrapper of ops)
            ops.segment_rank(*args)
    with pytest.raises(ValueError, match=r"edges: expected the \[T, 2\] pair layout"):
        ops.segment_rank(sc, ptr, torch.zeros(3, 3, dtype=torch.int64), tptr, tnode)
    with pytest.raises(ValueError, match="edges: one pair per score"):
        ops.segment_rank(sc, ptr, ed[:2], tptr, tnode)
    with pytest.raises(ValueError, match=r"ptr: \[Q \+ 1\] offsets"):
        ops.segment_rank(sc, ptr[:0], ed, tptr[:0], tnode)
    for bad in (tptr[:2], torch.tensor([0, 1, 2, 2])):
        with pytest.raises(ValueError, match="tptr: one target list per segment"):
            ops.segment_rank(sc, ptr, ed, bad, tnode)


# ---- ranking_metrics ----------------------------------------------------------------------------------------------------------
def _res(n_targets, rank, retrieval=None, m=None):
    from ocn_amd.ranking import RankResult
    tptr = torch.tensor([0] + n_targets).cumsum(0)
    rank = torch.tensor(rank, dtype=torch.int64)
    return RankResult(sources=torch.arange(len(n_targets)), tptr=tptr, target=torch.arange(rank.numel()), n_cand=torch.full((len(n_targets),), 9),
                      rank=rank, retrieval_rank=None if retrieval is None else torch.tensor(retrieval, dtype=torch.int64), m=m)


def d(r):
    return 1.0 / math.log2(1.0 + r)


def test_ranking_metrics_by_hand():
    """Four sources: A has the targets ranked (1, 3, 40); B has none and enters no mean; C has two targets, both unranked; D has
    one target at rank 7.  Ranks of the form 2^j - 1 have an exact gain (1, 1/2, 1/3), so the sums below are exact too."""
    from ocn_amd.ranking import ranking_metrics
    res = _res([3, 0, 2, 1], [3, 40, 1, 0, 0, 7])
    met = ranking_metrics(res, ks=(1, 3, 10, 1000))
    assert met["n_sources"] == 4 and met["n_eval"] == 3 and met["n_pairs"] == 6
    ideal3 = d(1) + d(2) + d(3)
    want = {
        "recall@1": (1 / 3 + 0 + 0) / 3, "hit_rate@1": 1 / 3, "pair_hits@1": 1 / 6, "ndcg@1": (1.0 / 1.0 + 0 + 0) / 3,
        "recall@3": (2 / 3 + 0 + 0) / 3, "hit_rate@3": 1 / 3, "pair_hits@3": 2 / 6, "ndcg@3": ((1.0 + 0.5) / ideal3 + 0 + 0) / 3,
        "recall@10": (2 / 3 + 0 + 1) / 3, "hit_rate@10": 2 / 3, "pair_hits@10": 3 / 6,
        "ndcg@10": ((1.0 + 0.5) / ideal3 + 0 + (1 / 3) / 1.0) / 3,
        "recall@1000": (1 + 0 + 1) / 3, "hit_rate@1000": 2 / 3, "pair_hits@1000": 4 / 6,        # k above every segment and every list
        "ndcg@1000": ((1.0 + 0.5 + d(40)) / ideal3 + 0 + (1 / 3) / 1.0) / 3,
        "mrr": (1.0 + 0.0 + 1 / 7) / 3, "coverage": 4 / 6,
    }
    assert set(met) == set(want) | {"n_sources", "n_eval", "n_pairs"}
    for key, v in want.items():
        assert met[key] == pytest.approx(v, rel=1e-14, abs=0), key
    assert met["recall@1000"] == 2 / 3 and met["hit_rate@10"] == 2 / 3 and met["pair_hits@3"] == 2 / 6 and met["coverage"] == 4 / 6
    assert ranking_metrics(res, ks=[3]) == {k: v for k, v in met.items() if "@" not in k or k.endswith("@3")}
    assert ranking_metrics(res, ks=(1, 3, 10, 1000)) == met              # fixed order: the same bits again
    with pytest.raises(ValueError, match="ks must be"):
        ranking_metrics(res, ks=())
    for bad in ((0,), (10, -1), (10.0,), (True,), 10, "10", None):
        with pytest.raises(ValueError, match="ks must be"):
            ranking_metrics(res, ks=bad)
    with pytest.raises(ValueError, match="tptr must ascend"):
        ranking_metrics(_res([3, 0, 2, 1], [1, 2]))


def test_ranking_metrics_separate_the_three_failures():
    """A short list of m = 4.  Of eight pairs: two are no candidates (retrieval rank 0), two were dropped by the short list
    (retrieval rank 5 and 90 > m), four were ranked by the model.  coverage = 6 / 8, retention = 4 / 6."""
    from ocn_amd.ranking import ranking_metrics
    res = _res([4, 3, 0, 1], rank=[2, 0, 0, 1, 0, 3, 4, 0], retrieval=[4, 5, 0, 1, 90, 2, 3, 0], m=4)
    assert torch.equal(res.rank > 0, (res.retrieval_rank >= 1) & (res.retrieval_rank <= 4))      # the invariant of a RankResult
    met = ranking_metrics(res, ks=(2,))
    assert met["m"] == 4 and met["coverage"] == 6 / 8 and met["retention"] == 4 / 6 and met["n_eval"] == 3
    assert met["pair_hits@2"] == 2 / 8 and met["hit_rate@2"] == 1 / 3
    assert met["recall@2"] == pytest.approx((2 / 4 + 0 / 3 + 0 / 1) / 3, rel=1e-14)
    assert met["mrr"] == pytest.approx((1.0 + 1 / 3 + 0.0) / 3, rel=1e-14)
    none = ranking_metrics(_res([2, 1], rank=[0, 0, 0], retrieval=[0, 0, 0], m=4), ks=(5,))       # a share of nothing is 0.0
    assert none["coverage"] == 0.0 and none["retention"] == 0.0 and none["mrr"] == 0.0 and none["ndcg@5"] == 0.0
    empty = ranking_metrics(_res([0, 0], rank=[]), ks=(5,))
    assert empty["n_eval"] == 0 and empty["n_pairs"] == 0 and empty["recall@5"] == 0.0 and empty["coverage"] == 0.0
    moved = res.to("cpu")
    assert torch.equal(moved.rank, res.rank) and moved.m == 4 and torch.equal(moved.retrieval_rank, res.retrieval_rank)
