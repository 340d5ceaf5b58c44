"""The intersection pass (`ocn_cn_flags`, `ocn_cn_flags_rec` behind `ocn_order_by_node_finish_rec`) against a torch
restatement: every output is an integer, so every comparison is `torch.equal`.  The graphs are built by hand so that each
branch of the kernel is taken: empty source row; source rows of 1, 63, 64, 65 and 200 entries (one trip, the trip boundary,
several trips); target rows of 0, 64 (registers), 65 (LDS copy) and 1500 > T1_CAP entries (search in memory); a full T2 row;
T2 absent, as a CSR (short rows and sampled long rows) and as bit rows; T1 as bit rows; the LDS histogram of a small graph;
batches of 3 and of 1003 candidates (not multiples of four) with duplicates and runs of one source; a poisoned offset scan;
with and without processing order, records and group costs."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import slot_record

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HF = 21
SRC_LEN = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 200}
T1_LEN = {0: 0, 1: 64, 2: 65, 3: 1500, 4: 1}
FULL_ROW = 6                                   # row of T2 that holds every column


def _csr(n, n_cols, lens, seed, mean):
    """Sorted CSR pattern with the given row lengths for the special rows, random short rows elsewhere."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for r in range(n):
        d = lens.get(r, int(torch.randint(0, 2 * mean, (1,), generator=g)))
        d = min(d, n_cols)
        rows.append(torch.sort(torch.randperm(n_cols, generator=g)[:d])[0].to(torch.int32))
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([r.numel() for r in rows]), 0)
    return rowptr, torch.cat(rows), rows


def _bit_rows(rows, n_cols):
    """int32 [n_rows][ceil(n_cols / 32)]: bit k of row r = column k is in row r."""
    words = (n_cols + 31) // 32
    bits = np.zeros((len(rows), words * 32), dtype=np.uint8)
    for r, cols in enumerate(rows):
        bits[r, cols.numpy()] = 1
    return torch.from_numpy(np.packbits(bits, axis=1, bitorder="little").view("<i4").copy())


def _candidates(n, B, seed):
    g = torch.Generator().manual_seed(seed)
    special = [(s, d) for s in SRC_LEN for d in list(T1_LEN) + [FULL_ROW]]
    src = torch.randint(0, n, (B,), generator=g)
    dst = torch.randint(0, n, (B,), generator=g)
    for q, (s, d) in enumerate(special[:max(B - 2, 0)]):
        src[q], dst[q] = s, d
    if B >= 64:
        src[40:52] = 5                                              # one hub source on consecutive slots
        src[52], dst[52] = src[53], dst[53] = 4, 3                  # duplicate candidates
        src[B - 1], dst[B - 1] = 5, 3
    return src, dst


def _expect(A, T1, T2, src, dst, off, order, n_cols, void):
    B = src.numel()
    flags = torch.zeros(int(off[B]) if not void else 0, dtype=torch.uint8)
    hist = torch.zeros(n_cols, dtype=torch.int64)
    cnt1 = torch.zeros(B, dtype=torch.int32)
    cnt2 = torch.zeros(B, dtype=torch.int32)
    rec = torch.zeros(B, 4, dtype=torch.int64)
    cost = torch.zeros(4 * ((B + 3) // 4), dtype=torch.int32)
    for slot in range(B):
        e = int(order[slot])
        i, j = int(src[e]), int(dst[e])
        row = A[2][i] if not void else A[2][i][:0]
        f1 = torch.isin(row, T1[2][j])
        f2 = torch.isin(row, T2[2][j]) if T2 is not None else torch.zeros_like(f1)
        base = int(off[e]) if not void else 0
        flags[base:base + row.numel()] = (f1.to(torch.uint8) | (f2.to(torch.uint8) << 1))
        hist.index_add_(0, row.long(), f1.long() | (f2.long() << HF) | ((f1 | f2).long() << (2 * HF)))
        c1, c2 = int(f1.sum()), int(f2.sum())
        cnt1[e], cnt2[e] = c1, c2
        rec[slot] = torch.tensor(slot_record(e, i, j, int(A[0][i]), row.numel(), base, c1 > 0, c2 > 0,
                                             row.numel() > 0 and c2 == row.numel()))
        cost[slot] = c1 + c2
    return flags, hist, cnt1, cnt2, rec, cost.view(-1, 4).max(1)[0]


def _run(lib, A, T1, T2, src, dst, n_cols, mode, t1_bits, t2_bits, want_rec, poison):
    from ocn_amd import ops
    P, S = ops.ptr, ops.stream_ptr
    B, n = src.numel(), A[0].numel() - 1
    d = lambda t: None if t is None else t.to(DEV)
    rowptrA, colA, rp1, c1, src_d, dst_d = d(A[0]), d(A[1]), d(T1[0]), d(T1[1]), d(src), d(dst)
    rp2, c2 = (d(T2[0]), d(T2[1])) if T2 is not None else (None, None)
    bm1 = d(_bit_rows(T1[2], n_cols)) if t1_bits else None
    bm2 = d(_bit_rows(T2[2], n_cols)) if (t2_bits and T2 is not None) else None
    off = torch.empty(B + 1, dtype=torch.int64, device=DEV)
    sws = torch.zeros(int(lib.ocn_scan_workspace_bytes(B)) // 8 + 1, dtype=torch.int64, device=DEV)
    ows = torch.zeros(int(lib.ocn_order_workspace_bytes(n)) // 8 + 1, dtype=torch.int64, device=DEV)
    order = torch.empty(B, dtype=torch.int64, device=DEV) if mode != "none" else None
    rec = torch.full((B, 4), -7, dtype=torch.int64, device=DEV) if (want_rec or mode == "rec") else None
    gcost = torch.full(((B + 3) // 4,), -7, dtype=torch.int32, device=DEV) if rec is not None else None
    if mode == "rec":
        ops.check(lib.ocn_batch_prep(P(rowptrA), P(src_d), B, P(off), P(sws), n, P(ows), None, None, 0, S()), "prep")
    else:
        ops.check(lib.ocn_edge_offsets(P(rowptrA), P(src_d), B, P(off), P(sws), S()), "offsets")
    true_off = off.cpu()
    if poison:
        off[B] = -1
    if mode == "rec":
        ops.check(lib.ocn_order_by_node_finish_rec(P(src_d), P(dst_d), P(rowptrA), P(off), B, n, P(order), P(rec), P(ows), S()), "finish_rec")
    elif mode == "plain":
        ops.check(lib.ocn_order_by_node(P(src_d), B, n, P(order), P(ows), S()), "order")
    cap = int(true_off[B])
    flags = torch.zeros(max(cap, 1), dtype=torch.uint8, device=DEV)
    hist = torch.zeros(n_cols, 2, dtype=torch.int64, device=DEV)
    cnt1 = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    cnt2 = torch.full((B,), -7, dtype=torch.int32, device=DEV) if T2 is not None else None
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    fn = lib.ocn_cn_flags_rec if mode == "rec" else lib.ocn_cn_flags
    ops.check(fn(P(rowptrA), P(colA), P(rp1), P(c1), P(rp2), P(c2), P(bm1), bm1.shape[1] if bm1 is not None else 0,
                 P(bm2), bm2.shape[1] if bm2 is not None else 0, P(src_d), P(dst_d), P(order), B, n_cols, P(off), P(flags), cap,
                 P(hist), P(cnt1), P(cnt2), P(status), P(rec), P(gcost), S()), "flags")
    torch.cuda.synchronize()
    cw = ((n * 4 + 15) // 16) * 16 // 8       # order workspace: per-node counters | n + 1 node offsets (scratch) | scan state
    assert int(ows[:cw].abs().sum()) == 0 and int(ows[cw + n + 1:].abs().sum()) == 0 and int(sws.abs().sum()) == 0      # left zero
    c = lambda t: None if t is None else t.cpu()
    return dict(off=true_off, order=c(order) if order is not None else torch.arange(B), flags=c(flags)[:cap], hist=c(hist),
                cnt1=c(cnt1), cnt2=c(cnt2), rec=c(rec), gcost=c(gcost), status=c(status))


def _check(out, A, T1, T2, src, dst, n_cols, poison):
    B = src.numel()
    assert torch.equal(torch.sort(out["order"])[0], torch.arange(B))
    assert bool((src[out["order"]][1:] >= src[out["order"]][:-1]).all()) or torch.equal(out["order"], torch.arange(B))
    flags, hist, cnt1, cnt2, rec, gcost = _expect(A, T1, T2, src, dst, out["off"], out["order"], n_cols, poison)
    if not poison:
        assert torch.equal(out["flags"], flags)
    assert torch.equal(out["hist"][:, 0], hist) and int(out["hist"][:, 1].abs().sum()) == 0
    assert torch.equal(out["cnt1"], cnt1)
    if out["cnt2"] is not None:
        assert torch.equal(out["cnt2"], cnt2)
    if out["rec"] is not None:
        assert torch.equal(out["rec"], rec)
        assert torch.equal(out["gcost"], gcost)
    assert int(out["status"][0]) == (2 if poison else 0) and int(out["status"][3]) == (2 if poison else 0)


def _graph(n):
    A = _csr(n, n, SRC_LEN, seed=1, mean=20)
    # (targets share columns with the sources' rows often enough: rows are dense draws from few columns when n is small)
    T1 = _csr(n, n, {k: min(v, n) for k, v in T1_LEN.items()}, seed=2, mean=40)
    t2_len = {0: 0, 1: 64, 2: 65, 3: min(3000, n - 1), 4: 500, FULL_ROW: n}
    T2 = _csr(n, n, t2_len, seed=3, mean=150)
    return A, T1, T2


GRAPHS = {}


def graph(n):
    if n not in GRAPHS:
        GRAPHS[n] = _graph(n)
    return GRAPHS[n]


# n = 9000 columns: the histogram goes to memory; n = 1600: the workgroup's LDS histogram (ocn_cn_flags_small_graph_cols)
@pytest.mark.parametrize("n", [9000, 1600])
@pytest.mark.parametrize("t2", ["none", "csr", "bits"])
@pytest.mark.parametrize("mode", ["rec", "plain", "none"])
def test_flags_match_the_torch_restatement(hiplib, n, t2, mode):
    assert (n <= hiplib.ocn_cn_flags_small_graph_cols()) == (n == 1600)
    A, T1, T2 = graph(n)
    T2u = None if t2 == "none" else T2
    for B in (1003, 3):
        src, dst = _candidates(n, B, seed=B)
        out = _run(hiplib, A, T1, T2u, src, dst, n, mode, False, t2 == "bits", want_rec=(mode != "none" or B == 3), poison=False)
        _check(out, A, T1, T2u, src, dst, n, False)
        again = _run(hiplib, A, T1, T2u, src, dst, n, mode, False, t2 == "bits", want_rec=(mode != "none" or B == 3), poison=False)
        for k in ("flags", "hist", "cnt1", "cnt2"):
            assert (out[k] is None and again[k] is None) or torch.equal(out[k], again[k]), k
        if out["rec"] is not None:                                   # slots of one source may swap between runs: compare by batch row
            by_row = lambda r: r[torch.argsort(r[:, 0])][:, [0, 1, 2, 3]]
            assert torch.equal(by_row(out["rec"]), by_row(again["rec"]))


@pytest.mark.parametrize("n", [9000, 1600])
@pytest.mark.parametrize("mode", ["rec", "plain"])
def test_bit_rows_of_t1(hiplib, n, mode):
    A, T1, T2 = graph(n)
    src, dst = _candidates(n, 1003, seed=5)
    out = _run(hiplib, A, T1, T2, src, dst, n, mode, True, True, want_rec=True, poison=False)
    _check(out, A, T1, T2, src, dst, n, False)


@pytest.mark.parametrize("mode", ["rec", "plain", "none"])
def test_poisoned_offsets_give_a_void_batch(hiplib, mode):
    A, T1, T2 = graph(9000)
    src, dst = _candidates(9000, 1003, seed=6)
    out = _run(hiplib, A, T1, T2, src, dst, 9000, mode, False, True, want_rec=True, poison=True)
    _check(out, A, T1, T2, src, dst, 9000, True)


def test_records_absent_and_argument_errors(hiplib):
    from ocn_amd import ops
    A, T1, T2 = graph(9000)
    src, dst = _candidates(9000, 1003, seed=7)
    out = _run(hiplib, A, T1, T2, src, dst, 9000, "plain", False, True, want_rec=False, poison=False)
    assert out["rec"] is None
    _check(out, A, T1, T2, src, dst, 9000, False)
    p = ctypes.c_void_p(16)
    N = ctypes.c_void_p(0)
    # the record-fed form needs both the order and the records
    assert hiplib.ocn_cn_flags_rec(p, p, p, p, N, N, N, 0, N, 0, p, p, N, 4, 10, p, p, 0, p, p, N, p, p, N, N) == -1
    assert hiplib.ocn_cn_flags_rec(p, p, p, p, N, N, N, 0, N, 0, p, p, p, 4, 10, p, p, 0, p, p, N, p, N, N, N) == -1
    assert hiplib.ocn_order_by_node_finish_rec(p, p, p, p, 4, 10, p, N, p, N) == -1
    assert hiplib.ocn_order_by_node_finish_rec(p, p, p, p, 0, 10, p, p, p, N) == 0


def test_the_product_path_feeds_the_records_from_the_prep_pass(hiplib):
    """CNState at a batch large enough for a processing order: the records come from ocn_order_by_node_finish_rec and equal
    what the batch-order call (no order: records written by the intersection pass itself) gives for the same rows."""
    from ocn_amd import ops
    from ocn_amd.utils import CNState
    from tests.helpers import batch, make_graph, product_adj2, to_product
    oadj = make_graph(20000, 10, 300, seed=8)
    adj = to_product(oadj, DEV)
    adj2 = product_adj2(adj)
    e = batch(oadj, max(ops.sort_edges_min_batch, 4096) + 1, 1).to(DEV)
    st = CNState(adj, adj, adj2, e)
    assert st.order is not None
    rec = st.rec.clone().cpu()
    cnt1, cnt2, hist = st.cnt1.clone(), st.cnt2.clone(), st.hist.clone()
    keep = ops.sort_edges_min_batch
    ops.sort_edges_min_batch = 1 << 40
    try:
        st0 = CNState(adj, adj, adj2, e)
    finally:
        ops.sort_edges_min_batch = keep
    assert st0.order is None
    rec0 = st0.rec.clone().cpu()
    assert torch.equal(cnt1, st0.cnt1) and torch.equal(cnt2, st0.cnt2) and torch.equal(hist, st0.hist)
    assert torch.equal(rec[torch.argsort(rec[:, 0])], rec0)
