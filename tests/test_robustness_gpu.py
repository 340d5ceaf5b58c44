"""GPU tests of the host-side hazards the round-3 review found: lazy adjacency caches under
several streams, the cn7 row-sum cache across re-allocated embeddings, a scan on a workspace that is not zero, and the
sticky status words a scoring loop reads once per split."""
from types import SimpleNamespace

import pytest
import torch

from oracle import ocn_oracle as O
from tests.helpers import batch, make_graph, product_adj2, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("route", ["pattern", "walk"])
def test_scoring_loops_on_a_cold_adjacency_equal_forward(hiplib, monkeypatch, route):
    """score_edges / score_mrr_split on a FRESH SparseTensor (no bit rows, no degree sums, no longest row cached) with three
    batches in flight: phase A of batches 0 and 1 runs on two side streams that are ordered against the caller's stream only,
    so whoever builds a lazy cache must publish it to the other.  Scores equal forward() batch by batch."""
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import score_edges, score_mrr_split
    from ocn_amd.utils import adjoverlap, get_cn1_cn2
    n, H, bs = 3000, 64, 512
    oadj = make_graph(n, 14, 300, seed=21)
    monkeypatch.setattr(ops, "overlap_min_batch", 0)
    monkeypatch.setattr(ops, "overlap_depth", 3)
    torch.manual_seed(3)
    x = torch.randn(n, H, device=DEV)
    name = "cn5" if route == "pattern" else "cn7"
    pred = predictor_dict[name](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    args = SimpleNamespace(sum=0.5)
    e = batch(oadj, 6 * bs + 37, 5).to(DEV)

    def fresh():
        adj = to_product(oadj, DEV)
        assert adj._bitmap is None and adj._nds is None and adj._maxdeg is None
        return adj

    with torch.no_grad():
        if route == "pattern":
            adj = fresh()
            adj2 = product_adj2(adj)
            got = score_edges(pred, x, adj, adj2, e.t().contiguous(), bs, args)
            ref_adj = fresh()
            ref = torch.cat([pred(x, ref_adj, adjoverlap(ref_adj, ref_adj, b), adjoverlap(ref_adj, adj2, b), b, args).reshape(-1)
                             for b in e.split(bs, dim=1)])
        else:
            adj = fresh()
            src, dst = e[0, :2 * bs + 11].contiguous(), e[1, :2 * bs + 11].contiguous()
            neg = torch.randint(0, n, (src.numel(), 3), device=DEV)
            pos, negp = score_mrr_split(pred, x, adj, src, dst, neg, bs, args)
            got = torch.cat([pos, negp.reshape(-1)])
            ref_adj = fresh()
            allsrc = torch.cat([src, src.view(-1, 1).repeat(1, 3).view(-1)])
            alldst = torch.cat([dst, neg.reshape(-1)])
            outs = []
            for s, d in ((src, dst), (allsrc[src.numel():], alldst[src.numel():])):
                for q in range(0, s.numel(), bs):
                    b = torch.stack((s[q:q + bs], d[q:q + bs]))
                    outs.append(pred(x, ref_adj, *get_cn1_cn2(ref_adj, b), b, args).reshape(-1))
            ref = torch.cat(outs)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)


def test_lazy_caches_publish_an_event_for_other_streams(hiplib):
    """The cache builder records an event; a reader on another stream waits for it; once complete it is dropped."""
    oadj = make_graph(800, 10, 100, seed=4)
    adj = to_product(oadj, DEV)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        bm = adj.bit_rows()
        nds = adj.neighbor_degree_sum()
    assert "bitmap" in adj._ready and "nds" in adj._ready
    bm2, nds2 = adj.bit_rows(), adj.neighbor_degree_sum()         # the default stream: waits for (or finds complete) the events
    assert bm2 is bm and nds2 is nds
    deg = adj._rowptr[1:] - adj._rowptr[:-1]
    want = torch.zeros(800, dtype=torch.int64, device=DEV).index_add_(0, adj._row64(), deg[adj._col.long()])
    assert torch.equal(nds2, want)
    torch.cuda.synchronize()
    adj.bit_rows(), adj.neighbor_degree_sum()
    assert not adj._ready


def test_cn7_row_sum_cache_follows_the_embeddings_not_their_address(hiplib, monkeypatch):
    """the drivers' test() computes a fresh h per evaluation; the allocator hands it the freed h's
    address, version 0, same shape.  The shortcut's cache must not hit on that: scores equal share_full_rows=False."""
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    from ocn_amd.utils import adjoverlap
    n, H, B = 1200, 64, 4096
    oadj = make_graph(n, 400, 1100, seed=13, clique_frac=0.2)
    adj = to_product(oadj, DEV)
    adj2 = product_adj2(adj)
    assert adj2.nnz() * 2 > n * n
    e = batch(oadj, B, 2).to(DEV)
    pred = predictor_dict["cn7"](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    args = SimpleNamespace(sum=2.74)

    def score(x):
        with torch.no_grad():
            return pred(x, adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e), e, args).clone()

    torch.manual_seed(0)
    x = torch.randn(n, H, device=DEV)
    first = score(x)
    addr = x.data_ptr()
    del x
    x = torch.randn(n, H, device=DEV) * 3.0                        # a different tensor; the caching allocator reuses the block
    same_address = x.data_ptr() == addr
    got = score(x)
    monkeypatch.setattr(ops, "share_full_rows", False)
    ref = score(x)
    assert torch.equal(got, ref) and not torch.equal(got, first)
    assert same_address or True                                    # (the address usually repeats; the test holds either way)
    # an in-place update of the SAME tensor is seen through its version counter
    monkeypatch.setattr(ops, "share_full_rows", True)
    x.mul_(0.5)
    got2 = score(x)
    monkeypatch.setattr(ops, "share_full_rows", False)
    assert torch.equal(got2, score(x))


def test_scan_on_a_dirty_workspace_poisons_the_total_instead_of_trapping(hiplib):
    """VERDICT r3 #13 / ADVICE r3: a chained scan whose workspace is not zero used to end in __builtin_trap() (the process
    aborts).  Now: bounded wait, zero offsets for the tiles that cannot chain, total = OCN_SCAN_POISON, no abort — and the
    host wrapper that reads a total raises a Python error."""
    from ocn_amd import _lib, ops
    n = 100003
    cnt = torch.randint(0, 1000, (n,), dtype=torch.int32, device=DEV)
    out = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    words = int(hiplib.ocn_scan_workspace_bytes(n)) // 8 + 1
    want = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(cnt.long(), 0)])
    for ticket in (5, 1 << 40):                                    # tiles 0 .. 4 never drawn (later tiles wait for them in vain) / no ticket inside the launch
        ws = torch.zeros(words, dtype=torch.int64, device=DEV)
        ws[0] = ticket
        ops.check(hiplib.ocn_scan_i32(ops.ptr(cnt), n, ops.ptr(out), ops.ptr(ws), ops.stream_ptr()), "scan")
        torch.cuda.synchronize()                                   # (returns: no trap, no hang)
        assert int(out[n]) == -1
    with pytest.raises(_lib.OcnHipError):
        ops._total(out[n])
    ws = torch.zeros(words, dtype=torch.int64, device=DEV)           # a clean workspace scans correctly afterwards
    ops.check(hiplib.ocn_scan_i32(ops.ptr(cnt), n, ops.ptr(out), ops.ptr(ws), ops.stream_ptr()), "scan")
    assert torch.equal(out, want) and not bool(ws.any())


def test_poisoned_offsets_raise_the_sticky_status_and_orders_fall_back(hiplib):
    """The consumers of a poisoned scan: the intersection pass raises OCN_ST_SCAN in status[0] and the sticky status[3]
    (predictor.check_errors reads the latter once per split), the processing / class orders fall back to batch order."""
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    from ocn_amd.utils import CNState, adjoverlap
    n, B, H = 20000, 40000, 64
    oadj = make_graph(n, 10, 300, seed=8)
    adj = to_product(oadj, DEV)
    adj2 = product_adj2(adj)
    e = batch(oadj, B, 1).to(DEV)
    # (1) order_by_node with a dirty scan state: batch order, counters left zero
    nn, Bo = 100000, 50000
    src = torch.randint(0, nn, (Bo,), device=DEV)
    order = torch.empty(Bo, dtype=torch.int64, device=DEV)
    ws = torch.zeros(int(hiplib.ocn_order_workspace_bytes(nn)) // 8 + 1, dtype=torch.int64, device=DEV)
    ws[(((nn * 4 + 15) // 16) * 16 + (nn + 1) * 8) // 8] = 7      # the ticket word of the scan state behind the counters and the node offsets
    ops.check(hiplib.ocn_order_by_node(ops.ptr(src), Bo, nn, ops.ptr(order), ops.ptr(ws), ops.stream_ptr()), "order")
    assert torch.equal(order, torch.arange(Bo, device=DEV))
    # (2) a predictor whose scratch set holds a dirty scan workspace: scores are void, check_errors says so
    pred = predictor_dict["cn5"](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    torch.manual_seed(1)
    x = torch.randn(n, H, device=DEV)
    with torch.no_grad():
        good = pred(x, adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e), e, None).clone()
        pred.check_errors()                                        # nothing raised so far
        key = next(k for k in pred._ws if k[0] == "scan_ws")
        pred._ws[key][0] = 3                                       # ticket word of the batch's offset scan
        pred(x, adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e), e, None)
        with pytest.raises(RuntimeError, match="scan workspace"):
            pred.check_errors()
        pred.check_errors()                                        # cleared by the read
        pred._ws[key].zero_()
        again = pred(x, adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e), e, None)
        pred.check_errors()
    assert torch.equal(again, good)
    # (3) CNState.check_status names the bit
    st = CNState(adj, adj, adj2, e)
    st.check_status()


@pytest.mark.parametrize("route", ["pattern", "walk"])
def test_graph_replayed_scoring_loop_equals_the_eager_loop(hiplib, monkeypatch, route):
    """pipeline.GraphedPhases: after two eager uses of a scratch set, phase A (prep .. pooling) and phase B (heads) of its
    batches are captured HIP graphs replayed with a fresh copy of the candidate ids.  Scores of a split of 70 batches (ragged
    tail included) equal the launch-by-launch loop bit for bit, on both CN routes; graphs were actually captured."""
    from ocn_amd import ops, pipeline
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import score_edges, score_mrr_split
    n, H, bs = 3000, 64, 256
    oadj = make_graph(n, 14, 300, seed=21)
    adj = to_product(oadj, DEV)
    adj2 = product_adj2(adj)
    monkeypatch.setattr(ops, "overlap_min_batch", 0)
    torch.manual_seed(3)
    x = torch.randn(n, H, device=DEV)
    name = "cn5" if route == "pattern" else "cn7"
    pred = predictor_dict[name](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    args = SimpleNamespace(sum=0.5)
    e = batch(oadj, 70 * bs - 19, 5).to(DEV)
    made = []
    orig = pipeline.GraphedPhases.finish

    def spy(self, token):
        made.append(token[0])
        return orig(self, token)
    monkeypatch.setattr(pipeline.GraphedPhases, "finish", spy)

    def run():
        with torch.no_grad():
            if route == "pattern":
                return score_edges(pred, x, adj, adj2, e.t().contiguous(), bs, args)
            neg = torch.randint(0, n, (e.shape[1], 1), generator=torch.Generator().manual_seed(1)).to(DEV)
            pos, negp = score_mrr_split(pred, x, adj, e[0].contiguous(), e[1].contiguous(), neg, bs, args)
            return torch.cat([pos, negp.reshape(-1)])
    monkeypatch.setattr(ops, "graph_loops", True)
    got = run()
    assert made.count("graph") > 20 and "eager" in made
    monkeypatch.setattr(ops, "graph_loops", False)
    ref = run()
    torch.cuda.synchronize()
    assert torch.equal(got, ref)


def test_two_stream_loop_under_stress_at_every_pooling_width(hiplib):
    """Round 4 found the H = 64 wave pooling kernel returning 64 wrong bytes of one xcn1 row about once in a hundred batches — only
    while another stream's heads ran beside it, so no single-stream test saw it (packed f32 multiply-add with an undefined high source
    register in chain_rows; now two scalar chains: cn_pool.hip).  Thirty repetitions of the depth-2 loop per
    width, every batch against the one-stream loop: a fault at that rate fails this test nine times in ten."""
    from types import SimpleNamespace
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import overlapped_steps
    from ocn_amd.utils import adjoverlap
    from tests.helpers import batch, make_graph, product_adj2, to_product
    n, B = 20000, 8192
    oadj = make_graph(n, 10, 600, 3, isolated=100)
    adj = to_product(oadj, DEV)
    with torch.no_grad():
        adj2 = product_adj2(adj)
    e0 = batch(oadj, B, 53).to(DEV)
    g = torch.Generator().manual_seed(9)
    batches = [e0[:, torch.randperm(B, generator=g).to(DEV)][:, : B - 5 * q].contiguous() for q in range(12)]
    args = SimpleNamespace(sum=0.7)
    for H in (64, 32, 128):
        torch.manual_seed(8 + H)
        x = torch.randn(n, H, device=DEV)
        pred = predictor_dict["cn5"](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
        pred.innerprod.fill_(0.37)

        def begin(it):
            e = batches[it]
            return pred.begin(x, adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e), e, slot=it, args=args)

        def run(overlap):
            return [o.clone() for o in overlapped_steps(begin, lambda tok: pred.finish(x, tok, args), len(batches), overlap=overlap)]
        with torch.no_grad():
            base = run(False)
            for rep in range(30 if H == 64 else 8):
                outs = run(True)
                torch.cuda.synchronize()
                bad = [(i, int((a != b).sum())) for i, (a, b) in enumerate(zip(outs, base)) if not torch.equal(a, b)]
                assert not bad, (H, rep, bad)
