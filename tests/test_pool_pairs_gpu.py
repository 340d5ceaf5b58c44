"""The pair form of the H = 256 pooling (cn_pool.hip, cn_gather_pair_kernel: a wave owns two neighbouring slots of one
schedule group; ``ocn_cn_gather_pair_min_batch``) against the one-slot form on the same inputs.  The form is forced with a
bound of 0 and switched off with one of 2^40; every comparison is of the bits of (xcn1, xcn2, x_i * x_j) — ``torch.equal``
on their int32 view, so that the NaN the buffers are pre-filled with (rows the heads never read stay unwritten under
class-major output rows, as in tests/test_heads_gpu.py) compare equal and -0 differs from +0.

Two kinds of batches: hand-built slot records over a hand-built graph, where each pair's contents are written down, and
the real intersection pass on a 3 000-node graph with three hubs (two of them longer than a pooling row may be) at the
batch sizes where the launch takes another path."""
from types import SimpleNamespace

import pytest
import torch

from oracle import ocn_oracle as O
from tests.helpers import batch, product_adj2, slot_record, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H = 256
NAN = float("nan")


def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _pooled_both(B, call):
    """call(ws) -> (xcn1, xcn2, xij) pooled into ws's NaN-filled buffer: with the pair form forced, then with it off."""
    from ocn_amd import ops
    outs = []
    prev = ops.gather_pair_min_batch()
    try:
        for bound in (0, 1 << 40):
            ops.gather_pair_min_batch(bound)
            ws = {}
            ops.buf(ws, "pooled", (3, B, H), torch.float32, DEV).fill_(NAN)
            outs.append([o.clone() for o in call(ws)])
        torch.cuda.synchronize()
    finally:
        ops.gather_pair_min_batch(prev)
    return outs


# ---- hand-built records ----------------------------------------------------------------------------------------------------------
N_HAND = 3000
ROW_LEN = {0: 0, 1: 5, 2: 70, 3: 1100, 4: 40, 5: 64, 6: 130}          # source node -> row length (3: cn_gather_long_kernel's)
# (source, flag pattern) per slot; slots 2g and 2g + 1 are one wave's pair
SLOTS = [
    (2, "rand"), (2, "rand"),            # same source, both with entries (two rounds of 64 positions)
    (4, "rand"), (4, "none"),            # same source, one without entries
    (6, "cn1@p"), (6, "cn2@p"),          # same source, cn1-only and cn2-only entries at the same positions
    (1, "rand"), (5, "dense"),           # different sources: five positions beside 64 live ones
    (0, "none"), (4, "rand"),            # a source with no neighbours
    (3, "rand"), (5, "rand"),            # a row longer than 1 024 beside an ordinary one
    (5, "rand"), (5, "rand"),
    (5, "rand"), (6, "rand"),            # the pair straddles the end of source 5's run
]


def _hand_built(copies, seed):
    """`copies` times the sixteen slots (flags drawn anew per copy), as the arrays ocn_cn_gather reads."""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.sort(torch.randperm(N_HAND, generator=g)[:ROW_LEN.get(r, 0)])[0].to(torch.int32) for r in range(8)]
    rowptr = torch.zeros(N_HAND + 1, dtype=torch.int64)
    rowptr[1:9] = torch.cumsum(torch.tensor([r.numel() for r in rows]), 0)
    rowptr[9:] = rowptr[8]
    col = torch.cat(rows)
    src, dst, off, flags, rec, cost = [], [], [0], [], [], []
    for c in range(copies):
        for s, (i, kind) in enumerate(SLOTS):
            d = ROW_LEN[i]
            if kind == "none":
                f = torch.zeros(d, dtype=torch.uint8)
            elif kind == "dense":
                f = torch.randint(1, 4, (d,), generator=g).to(torch.uint8)
            elif kind in ("cn1@p", "cn2@p"):
                f = torch.zeros(d, dtype=torch.uint8)
                f[torch.tensor([0, 3, 63, 64, 65, 100, d - 1])] = 1 if kind == "cn1@p" else 2
            else:
                f = (torch.randint(0, 4, (d,), generator=g) * (torch.rand(d, generator=g) < 0.3)).to(torch.uint8)
                f[int(torch.randint(0, d, (1,), generator=g))] |= 1
            e = len(src)
            j = 10 + e
            has1, has2 = int((f & 1).any()), int((f & 2).any())
            rec.append(slot_record(e, i, j, int(rowptr[i]), d, off[-1], has1, has2, False))
            src.append(i); dst.append(j); flags.append(f); off.append(off[-1] + d)
            cost.append(int((f & 1).sum() + ((f >> 1) & 1).sum()))
    B = len(src)
    rec = torch.tensor(rec, dtype=torch.int64)
    gcost = torch.tensor(cost + [0] * (-B % 4)).view(-1, 4).max(1)[0].to(torch.int32)
    w = torch.rand(N_HAND, 4, generator=g)
    w[:, 1] *= (torch.rand(N_HAND, generator=g) < 0.5)                 # t: zero for half the columns
    w[:, 3] = 0
    h = torch.randn(N_HAND, H, generator=g)
    d = lambda t: t.to(DEV)
    return SimpleNamespace(B=B, rowptr=d(rowptr), col=d(col), src=d(torch.tensor(src)), dst=d(torch.tensor(dst)),
                           off=d(torch.tensor(off)), flags=d(torch.cat(flags)), rec=d(rec), gcost=gcost, w=d(w), h=d(h))


@pytest.mark.parametrize("class_major", [False, True])
@pytest.mark.parametrize("copies", [1, 4], ids=["B16_no_schedule", "B64_scheduled"])
def test_hand_built_pairs(hiplib, copies, class_major):
    """Every pair content of SLOTS: 16 slots in source order without a schedule (four groups), and four copies with one
    (16 groups, two per eighth: workgroup b pools groups perm[2b] and perm[2b + 1])."""
    from ocn_amd import ops
    c = _hand_built(copies, 3 + copies)
    out_row = torch.randperm(c.B, generator=torch.Generator().manual_seed(1)).to(DEV) if class_major else None

    def call(ws):
        sched = None
        if copies > 1:                                 # the costs the intersection pass would have left, and room for the order
            sched = torch.zeros(2 * (c.B // 4), dtype=torch.int32, device=DEV)
            sched[: c.B // 4] = c.gcost.to(DEV)
        return ops.cn_gather(c.rowptr, c.col, c.src, c.dst, c.off, c.flags, None, c.w, c.h, order=None,
                             max_row_len=max(ROW_LEN.values()), wsd=ws, out_row=out_row, rec=c.rec, sched=sched)

    two, one = _pooled_both(c.B, call)
    assert _bits_equal(two, one)
    # (the one-slot form is the reference; a few rows against the definition, so that "equal" is not "equally empty")
    x1, x2, xij = (t.cpu() for t in two)
    rowptr, col, flags, w, h = c.rowptr.cpu(), c.col.cpu().long(), c.flags.cpu(), c.w.cpu(), c.h.cpu()
    for e in (0, 3, 4, 5, 7, 8, 10, 15):
        i, j, o = int(c.src[e]), int(c.dst[e]), int(out_row[e]) if class_major else e
        assert torch.equal(xij[o], h[i] * h[j])
        ks = col[rowptr[i]: rowptr[i + 1]]
        f = flags[int(c.off[e]): int(c.off[e + 1])]
        a1, a2 = torch.zeros(H), torch.zeros(H)
        for k, fk in zip(ks.tolist(), f.tolist()):
            if fk:
                wa = w[k, 0] if fk & 1 else torch.tensor(0.0)
                wb = ((1.0 if fk & 2 else 0.0) - (w[k, 1] if fk & 1 else torch.tensor(0.0))) * w[k, 2]
                if float(wa) != 0.0 or float(wb) != 0.0:
                    a1, a2 = a1 + wa * h[k], a2 + wb * h[k]
        has1, has2 = bool((f & 1).any()), bool((f & 2).any())
        if not class_major or has1:
            assert torch.equal(x1[o], a1), e
        else:
            assert bool(torch.isnan(x1[o]).all()), e                       # never read by the heads: left alone
        if not class_major or has1 or has2:
            assert torch.equal(x2[o], a2), e
        else:
            assert bool(torch.isnan(x2[o]).all()), e


# ---- the real intersection pass ------------------------------------------------------------------------------------------------------
_G = {}
N_REAL = 3000
HUBS = {0: 1100, 1: 1030, 2: 700}                   # two rows longer than LONG_ROW (1 024), one long ordinary row


def _graph():
    if not _G:
        from ocn_amd.synth import chung_lu_graph
        n = N_REAL
        ei = chung_lu_graph(n - 4, avg_deg=10, max_deg=300, seed=5, clique_frac=0.5)       # the last four nodes: no neighbours
        g = torch.Generator().manual_seed(6)
        extra = [torch.stack([torch.full((d,), hub), 3 + torch.randperm(n - 7, generator=g)[:d]]) for hub, d in HUBS.items()]
        oadj = O.to_symmetric(O.from_edge_index(torch.cat([ei] + extra, 1), n))
        adj = to_product(oadj, DEV)
        _G.update(oadj=oadj, adj=adj, adj2=product_adj2(adj), x=torch.randn(n, H, generator=g))
        assert int(oadj.rowcount()[0]) > 1024 and int(oadj.rowcount()[n - 1]) == 0
    return SimpleNamespace(**_G)


def _edges(gr, B, seed):
    """B candidates: the sampler's, with hub sources, a source without neighbours and runs of one source planted."""
    e = batch(gr.oadj, B, seed).clone()
    plant = [0, 0, 1, 2, 2, 2, N_REAL - 1, 7, 7, 7, 7, 7]
    k = min(B, len(plant))
    e[0, :k] = torch.tensor(plant[:k])
    return e


def _state(gr, e, monkeypatch, sort):
    from ocn_amd import ops
    from ocn_amd.utils import CNState
    # sort: the batch is processed in source order and the intersection pass leaves the group costs for the schedule, as for
    # a batch of a scoring loop; else in batch order, no schedule
    monkeypatch.setattr(ops, "sort_edges_min_batch", 0 if sort else 1 << 40)
    return CNState(gr.adj, gr.adj, gr.adj2, e.to(DEV))


WEIGHTS = {"cn5_fresh": lambda st: st.weights_cn5(torch.zeros(1, device=DEV)),
           "cn5_trained": lambda st: st.weights_cn5(torch.tensor([0.37], device=DEV)),
           "cn7": lambda st: st.weights_cn7(0.7)}


# 1, 2, 7: tails; 61: an odd tail, 16 groups but no schedule (not a multiple of 32); 64: 16 groups, two per eighth — the
# smallest batch with the schedule on; 72: 18 groups, no multiple of eight; 96: a schedule with three groups per eighth,
# which keeps the one-slot form; 128: four per eighth
@pytest.mark.parametrize("B", [1, 2, 7, 61, 64, 72, 96, 128])
def test_pairs_pool_what_single_slots_pool(hiplib, monkeypatch, B):
    from ocn_amd import ops
    gr = _graph()
    e = _edges(gr, B, 100 + B)
    x = gr.x.to(DEV)
    for sort in (True, False):
        for kind, weights in WEIGHTS.items():
            for class_major in (False, True):
                st = _state(gr, e, monkeypatch, sort)
                assert st.rec is not None and (st.sched is not None) == sort
                w = weights(st)
                out_row = ops.class_order(st.cnt1, st.cnt2, st.order)[1] if class_major else None
                two, one = _pooled_both(B, lambda ws: (setattr(st, "ws", ws), st.gather(w, x, out_row=out_row))[1])
                assert _bits_equal(two, one), (sort, kind, class_major)
                if class_major and B >= 61:            # (something was left alone, and something was not)
                    nan_rows = torch.isnan(two[0]).all(1)
                    assert bool(nan_rows.any()) and not bool(nan_rows.all())


def test_pairs_against_the_oracle(hiplib, monkeypatch):
    """xcn1 of the forced pair form, scheduled, is the oracle's bit for bit (and xcn2, innerprod = 0)."""
    from ocn_amd import ops
    gr = _graph()
    B = 128
    e = _edges(gr, B, 77)
    ref1, ref2, _ = O.cn5_pool(gr.x, O.adjoverlap(gr.oadj, gr.oadj, e), O.adjoverlap(gr.oadj, O.adj2_sparse(gr.oadj), e),
                               torch.tensor([0.0]))
    st = _state(gr, e, monkeypatch, True)
    w = st.weights_cn5(torch.zeros(1, device=DEV))
    prev = ops.gather_pair_min_batch(0)
    try:
        x1, x2, xij = st.gather(w, gr.x.to(DEV))
        torch.cuda.synchronize()
    finally:
        ops.gather_pair_min_batch(prev)
    assert torch.equal(x1.cpu(), ref1) and torch.equal(x2.cpu(), ref2)
    assert torch.equal(xij.cpu(), gr.x[e[0]] * gr.x[e[1]])


def test_pair_form_beside_the_heads(hiplib):
    """Twelve 4 096-candidate batches through pipeline.overlapped_steps with the pair form forced: the pooling runs in
    phase A on the side streams, beside the fused heads of earlier batches — the scores of the one-stream loop, and of
    the one-slot form, bit for bit."""
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import overlapped_steps
    from ocn_amd.utils import adjoverlap
    gr = _graph()
    B = 4096
    x = gr.x.to(DEV)
    torch.manual_seed(4)
    pred = predictor_dict["cn5"](H, H, 1, 3, 0.0, 0.0, True).to(DEV).eval()
    batches = [_edges(gr, B, 300 + q).to(DEV) for q in range(12)]

    def begin(it):
        e = batches[it]
        return pred.begin(x, gr.adj, adjoverlap(gr.adj, gr.adj, e), adjoverlap(gr.adj, gr.adj2, e), e, slot=it)

    def loop(overlap):
        outs = [o.clone() for o in overlapped_steps(begin, lambda tok: pred.finish(x, tok), len(batches), overlap=overlap, batch=B)]
        torch.cuda.synchronize()
        return outs

    prev = ops.gather_pair_min_batch(0)
    try:
        with torch.no_grad():
            two_streams, one_stream = loop(True), loop(False)
            ops.gather_pair_min_batch(1 << 40)
            one_slot = loop(False)
    finally:
        ops.gather_pair_min_batch(prev)
    for a, b, c in zip(two_streams, one_stream, one_slot):
        assert torch.equal(a, b) and torch.equal(a, c)
