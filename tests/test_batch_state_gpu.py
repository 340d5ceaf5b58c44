"""The declared batch state and the one layered head evaluation on the GPU, on a graph as small as it can be while its bit
rows still cross one 64-lane word: 70 nodes, the last one isolated and used as a source."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.helpers import product_adj2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N, H_STATE, H_HEADS = 70, 16, 64
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "heads_layered_h64.npy")
BATCHES = (5, 70)                                                # one partial row tile; more than the 64 rows of one
CASES = [(name, B) for name in ("cn5", "cn7") for B in BATCHES]       # the rows of GOLDEN, in this order

LOOP_FIELDS = {"cls", "_cls_decided", "pooled", "cnt1", "cnt2", "order", "walk", "B", "N", "ws"}
STATE_FIELDS = LOOP_FIELDS | {"adj", "t2", "src", "dst", "off", "flags", "wc", "hist", "status", "scal", "rec", "sched",
                              "_sched_ready", "sharded", "shard_group", "_hist_live"}


def small_graph():
    """Symmetric, 69 connected-ish nodes and the isolated node 69."""
    from ocn_amd.sparse import SparseTensor
    a = np.random.default_rng(5).random((N, N)) < 0.12
    a = np.triu(a, 1)
    a[:, N - 1] = False
    a = a | a.T
    assert a[N - 1].sum() == 0 and a[:, 64:N - 1].any()
    r, c = np.nonzero(a)
    adj = SparseTensor.from_edge_index(torch.from_numpy(np.stack([r, c]).astype(np.int64)).to(DEV), sparse_sizes=(N, N))
    return adj, product_adj2(adj)


def candidates(B):
    """[2, B]: seeded pairs; the isolated node is the source of candidate 1 and the target of candidate 3."""
    e = torch.randint(0, N - 1, (2, B), generator=torch.Generator().manual_seed(100 + B))
    e[0, 1], e[1, 3] = N - 1, N - 1
    return e.to(DEV)


def declared(klass):
    """The data attributes a class and its bases declare in their class blocks."""
    return {k for c in klass.__mro__[:-1] for k, v in vars(c).items()
            if not k.startswith("__") and not callable(v) and not isinstance(v, (classmethod, staticmethod, property))}


def test_every_route_builds_a_state_with_the_declared_fields(hiplib):
    from ocn_amd import ops
    from ocn_amd.utils import CN8State, CNState
    adj, adj2 = small_graph()
    e = candidates(5)
    x = torch.randn(N, H_STATE, generator=torch.Generator().manual_seed(1)).to(DEV)
    pattern = CNState(adj, adj, adj2, e)
    states = dict(pattern=pattern, walk=CNState(adj, None, None, e, walk=True),
                  materialized=CNState.from_materialized(adj, pattern.materialize(1), pattern.materialize(2), e),
                  hop3=CNState.hop3(adj, adj2, e))
    assert declared(CNState) == STATE_FIELDS
    for route, st in states.items():
        assert set(vars(st)) <= STATE_FIELDS, route                    # nothing is bolted on beside the declaration
        got = {f: getattr(st, f) for f in sorted(STATE_FIELDS)}         # (no default: a missing field raises here)
        assert (got["cls"], got["_cls_decided"], got["pooled"], got["_sched_ready"], got["sharded"], got["shard_group"],
                got["_hist_live"]) == (None, False, None, False, False, None, True), route
        assert (got["B"], got["N"], got["walk"]) == (5, N, route == "walk") and got["adj"] is adj
        for f in ("src", "dst", "off", "flags", "hist", "cnt1", "status", "scal"):
            assert got[f] is not None, (route, f)
        absent = dict(pattern=("wc", "ws"), walk=("t2", "rec", "sched", "ws"), materialized=("t2", "order", "wc", "rec", "sched", "ws"),
                      hop3=("t2", "wc", "cnt2", "rec", "sched", "ws"))[route]
        assert all(got[f] is None for f in absent), (route, [f for f in absent if got[f] is not None])
    assert pattern.t2 is adj2 and pattern.rec is not None and states["walk"].wc is not None
    assert torch.equal(states["materialized"].cnt1, pattern.cnt1) and torch.equal(states["materialized"].cnt2, pattern.cnt2)
    assert pattern.cnt1[1].item() == 0 and states["hop3"].cnt1[1].item() == 0          # the isolated source

    st8 = CN8State(adj, adj, adj2, e)
    assert LOOP_FIELDS <= declared(CN8State) and set(vars(st8)) <= declared(CN8State)
    got = {f: getattr(st8, f) for f in sorted(LOOP_FIELDS)}
    assert (got["cls"], got["_cls_decided"], got["pooled"], got["cnt1"], got["cnt2"], got["order"], got["walk"], got["B"], got["N"],
            got["ws"]) == (None, True, None, None, None, None, False, 5, N, None)
    x1, _, xij = st8.pool(x)
    assert torch.equal(st8.cnt1, pattern.cnt1) and torch.equal(st8.cnt2, pattern.cnt2)

    # the pooling takes the states whose constructors leave no records and no schedule
    w = ops.unit_weights(N, DEV)
    want_ij = x[e[0]] * x[e[1]]
    for route in ("materialized", "hop3"):
        g1, g2, gij = states[route].gather(w, x)
        assert g1.shape == g2.shape == gij.shape == (5, H_STATE) and torch.equal(gij, want_ij), route
    assert x1.shape == (5, H_STATE) and torch.equal(xij, want_ij)
    torch.cuda.synchronize()
    for st in states.values():
        st.check_status()


def heads_case(name, B):
    """A seeded predictor at H = 64 (below the fused kernel's widths) and one pooled batch of the small graph: in batch order
    (the three pools back to back, as the pooling leaves them) and in class-major rows with their class order."""
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    from ocn_amd.utils import adjoverlap, fuse
    adj, adj2 = small_graph()
    e = candidates(B)
    torch.manual_seed(7)
    pred = predictor_dict[name](H_HEADS, H_HEADS, 1, 3, 0.0, 0.0, True)
    with torch.no_grad():
        pred.alpha.copy_(torch.tensor([0.3, -0.2, 0.1]))
        pred.beta.fill_(0.7)
    pred = pred.to(DEV).eval()
    x = torch.randn(N, H_HEADS, generator=torch.Generator().manual_seed(2)).to(DEV)
    st = fuse(adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e), e, None, adj=adj)
    w = pred._weights(st, SimpleNamespace(sum=2.74))
    cls = ops.class_order(st.cnt1, st.cnt2, st.order, None)
    return pred, x, st.gather(w, x), st.gather(w, x, out_row=cls[1]), cls


def per_branch(pred, xcn1, xcn2, xij):
    from ocn_amd import ops
    from ocn_amd.model import _seq_eval
    xij, xcn1, xcn2 = _seq_eval(pred.xijlin, xij), _seq_eval(pred.xcn1lin, xcn1), _seq_eval(pred.xcn2lin, xcn2)
    return _seq_eval(pred.lin, ops.combine3(pred._mix_coef(), xcn1, xcn2, xij))


@pytest.mark.parametrize("name,B", CASES)
def test_layered_heads_without_and_with_a_class_order(hiplib, name, B):
    """Without a class order H = 64 takes the layered form: the scores are those the commit before the two layered functions
    were merged gave for the same seeds (GOLDEN: its grouped form folds the branch mix into the third layers' weights and so
    differs from the per-branch walk in the last bits, there as here).  With the batch's class order, on class-major rows,
    the same function returns the same bits in batch order."""
    with torch.no_grad():
        pred, x, pooled, pooled_cm, cls = heads_case(name, B)
        assert pred._layout(H_HEADS).layered and not pred._layout(H_HEADS).fused
        plain = pred._heads(x, *pooled, None)
        assert torch.equal(plain, pred._heads_layered(*pooled, None))
        row = CASES.index((name, B))
        want = torch.from_numpy(np.load(GOLDEN)[row, :B]).to(DEV).reshape(B, 1)
        walk = per_branch(pred, *pooled)
        assert torch.equal(plain, want)
        assert torch.equal(pred._heads(x, *pooled_cm, cls), plain)
        # no back-to-back inputs: the per-branch walk runs instead
        apart = [torch.empty(B + 1, H_HEADS, device=DEV)[:B].copy_(t) for t in pooled]
        assert pred._heads_layered(*apart, None) is None and torch.equal(pred._heads(x, *apart, None), walk)
