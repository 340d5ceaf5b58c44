"""GPU tests of the training-side kernels (NeighborOverlap_large.py:56-63, 76-90): the per-batch
COO -> CSR build, the weight gradient and the deterministic pooling backward, through the C ABI."""
import pytest
import torch

from ocn_amd import ops
from ocn_amd.sparse import SparseTensor
from tests.graph_build_mirror import csr_of_coo

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# torch restatement on the CPU: sort by (row, col), optionally with the transposed entries and without duplicates
_ref_csr = csr_of_coo


def _coo_case(name):
    g = torch.Generator().manual_seed(7)
    if name == "small":                      # rows of every short length, duplicates, empty rows
        n = 300
        row = torch.randint(0, n - 20, (4000,), generator=g)
        col = torch.randint(0, n, (4000,), generator=g)
    elif name == "hubs":                     # rows longer than a wave, longer than the LDS sort (12 288), one of 40 000
        n = 60000
        parts_r = [torch.randint(0, n, (200000,), generator=g), torch.full((40000,), 5), torch.full((9000,), 77),
                   torch.full((300,), 11)]
        parts_c = [torch.randint(0, n, (200000,), generator=g), torch.randint(0, n, (40000,), generator=g),
                   torch.randint(0, 3000, (9000,), generator=g), torch.randint(0, 200, (300,), generator=g)]
        row, col = torch.cat(parts_r), torch.cat(parts_c)
    elif name == "collab":                   # the size the training loop builds per batch
        n = 235868
        row = torch.randint(0, n, (1_100_000,), generator=g)
        col = torch.randint(0, n, (1_100_000,), generator=g)
    else:
        raise KeyError(name)
    return n, row, col


@pytest.mark.parametrize("name", ["small", "hubs", "collab"])
@pytest.mark.parametrize("symmetrize,dedupe", [(False, False), (True, True), (False, True)])
def test_coo_to_csr_equals_sort_and_unique(hiplib, name, symmetrize, dedupe):
    n, row, col = _coo_case(name)
    rowptr, out = ops.coo_to_csr(row.to(DEV), col.to(DEV), n, n, symmetrize=symmetrize, dedupe=dedupe)
    rp, c = _ref_csr(row, col, n, n, symmetrize, dedupe)
    assert torch.equal(rowptr.cpu(), rp)
    assert out.dtype == torch.int32 and torch.equal(out.cpu(), c)


def test_coo_to_csr_edge_cases(hiplib):
    e = torch.empty(0, dtype=torch.int64, device=DEV)
    rowptr, out = ops.coo_to_csr(e, e, 5, 5, symmetrize=True, dedupe=True)
    assert rowptr.tolist() == [0] * 6 and out.numel() == 0
    rowptr, out = ops.coo_to_csr(e, e, 0, 0)
    assert rowptr.tolist() == [0] and out.numel() == 0
    # rectangular, no symmetrisation; a self loop is its own transpose
    r = torch.tensor([2, 0, 2, 2], device=DEV)
    c = torch.tensor([6, 1, 0, 6], device=DEV)
    rowptr, out = ops.coo_to_csr(r, c, 3, 7, dedupe=True)
    assert rowptr.tolist() == [0, 1, 1, 3] and out.tolist() == [1, 0, 6]
    rowptr, out = ops.coo_to_csr(torch.tensor([1, 1], device=DEV), torch.tensor([1, 0], device=DEV), 2, 2, symmetrize=True, dedupe=True)
    assert rowptr.tolist() == [0, 1, 3] and out.tolist() == [1, 0, 1]
    with pytest.raises(IndexError):
        ops.coo_to_csr(torch.tensor([0, 3], device=DEV), torch.tensor([1, 1], device=DEV), 3, 3)
    with pytest.raises(IndexError):
        ops.coo_to_csr(torch.tensor([0, 1], device=DEV), torch.tensor([1, -1], device=DEV), 3, 3)


def test_sparse_tensor_builds_the_masked_adjacency_on_the_library(hiplib, monkeypatch):
    """The drivers' per-batch build (NeighborOverlap_large.py:56-63) through the product's SparseTensor: the same CSR as
    the torch restatement, built by ocn_coo_to_csr (twice: from_edge_index, to_symmetric) with torch's sort / unique never
    called.  (The kernel list of a training step is profiles/r03_train_step_kernel_stats.csv.)"""
    n, row, col = _coo_case("collab")
    tei = torch.stack([row, col]).to(DEV)
    calls = []
    real = ops.coo_to_csr
    monkeypatch.setattr(ops, "coo_to_csr", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    for name in ("sort", "argsort", "unique", "unique_consecutive"):
        monkeypatch.setattr(torch, name, lambda *a, _n=name, **k: (_ for _ in ()).throw(AssertionError(f"torch.{_n} called")))
    adj = SparseTensor.from_edge_index(tei, sparse_sizes=(n, n)).to_device(DEV, non_blocking=True)
    adj = adj.to_symmetric()
    monkeypatch.undo()
    assert len(calls) == 2 and calls[1].get("symmetrize") and calls[1].get("dedupe")
    rp, c = _ref_csr(row, col, n, n, True, True)
    rowptr, colx, _ = adj.csr()
    assert torch.equal(rowptr.cpu(), rp) and torch.equal(colx.cpu().to(torch.int32), c)


WGRAD_SHAPES = [(65536, 256, 256), (1000, 256, 256), (4096, 64, 64), (2048, 32, 32), (77, 1, 33), (1152, 256, 1433),
                (5000, 200, 58), (16, 128, 128), (3, 5, 7)]


@pytest.mark.parametrize("B,N,K", WGRAD_SHAPES, ids=lambda v: str(v))
def test_wgrad_is_as_accurate_as_an_fp32_gemm_and_deterministic(hiplib, B, N, K):
    """dW = dY^T X and db = column sums against an fp64 evaluation: error no worse than twice torch's own fp32 GEMM (floor
    1e-6 of the largest entry); two runs give the same bits (partial sums are added in a fixed order)."""
    g = torch.Generator().manual_seed(B + N + K)
    gy = (torch.randn(B, N, generator=g) * torch.logspace(-3, 2, N)).to(DEV)        # columns of mixed magnitude
    x = (torch.randn(B, K, generator=g) * (1.0 + 5.0 * torch.rand(B, 1, generator=g))).to(DEV)
    gw, gb = ops.wgrad(gy, x)
    gw2, gb2 = ops.wgrad(gy, x)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
    ref = gy.double().t() @ x.double()
    ref_b = gy.double().sum(0)
    err = (gw.double() - ref).abs().max().item()
    err_t = ((gy.t() @ x).double() - ref).abs().max().item()
    assert err <= 2 * err_t + 1e-6 * ref.abs().max().item(), (err, err_t)
    err_b = (gb.double() - ref_b).abs().max().item()
    assert err_b <= 2 * (gy.sum(0).double() - ref_b).abs().max().item() + 1e-6 * ref_b.abs().max().item()
    gw3, none = ops.wgrad(gy, x, with_bias=False)
    assert none is None and torch.equal(gw3, gw)


def test_wgrad_reads_strided_rows(hiplib):
    """A layer's input / upstream gradient may be one half of a wider buffer (row stride > width)."""
    g = torch.Generator().manual_seed(3)
    wide_y = torch.randn(3000, 96, generator=g).to(DEV)
    wide_x = torch.randn(3000, 200, generator=g).to(DEV)
    gy, x = wide_y[:, 32:96], wide_x[:, :128]
    gw, gb = ops.wgrad(gy, x)
    gwc, gbc = ops.wgrad(gy.contiguous(), x.contiguous())
    assert torch.equal(gw, gwc) and torch.equal(gb, gbc)
    gw0, gb0 = ops.wgrad(torch.empty(0, 8, device=DEV), torch.empty(0, 4, device=DEV))
    assert gw0.shape == (8, 4) and not gw0.any() and not gb0.any()


def _pool_case(n, avg, mx, B, H, seed):
    from oracle import ocn_oracle as O   # graph generator helpers only
    from tests.helpers import batch, make_graph, product_adj2, to_product
    from ocn_amd.utils import adjoverlap
    oadj = make_graph(n, avg, mx, seed)
    e = batch(oadj, B, seed + 5).to(DEV)
    adj = to_product(oadj, DEV)
    return adj, product_adj2(adj), e


def _assert_backward_key_lists(adj, adj2, e):
    """Host-side reference of the per-node key lists the deterministic pooling backward accumulates from, checked BEFORE the
    accumulate pass runs (round 3 chased a GPU memory fault in that pass by re-running it; the lists were
    verified by hand then — this is that check, kept).  Also every index the accumulate will form from a key is in range."""
    from ocn_amd.utils import CNState
    st = CNState(adj, adj, adj2, e)
    N, B, cap = adj.size(0), st.B, st.flags.numel()
    col_off, keys = ops.cn_gather_backward_lists(adj._rowptr, adj._col, st.src, st.dst, st.off, st.flags, N)
    rows = adj[st.src]                                            # row e = N(src[e]), columns ascending
    r, c, _ = rows.coo()
    pos = torch.arange(r.numel(), device=DEV) - rows._rowptr[:-1][r] + st.off[:-1][r]
    live = st.flags[pos] != 0
    eb = torch.arange(B, device=DEV)
    node = torch.cat([c[live], st.src, st.dst])
    key = torch.cat([pos[live], cap + 2 * eb, cap + 2 * eb + 1])
    want_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(torch.bincount(node, minlength=N), 0)])
    assert torch.equal(col_off, want_off)
    assert torch.equal(keys.long(), key[torch.argsort(node * (1 << 32) + key)])
    k = keys.long()
    pooled = k < cap
    row = torch.searchsorted(st.off, k[pooled], right=True) - 1     # the batch row pb_accumulate's binary search finds
    assert bool((row >= 0).all()) and bool((row < B).all()) and bool((st.flags[k[pooled]] != 0).all())
    assert bool((k[pooled] < st.off[B]).all())
    t = k[~pooled] - cap
    assert bool((t >= 0).all()) and bool(((t >> 1) < B).all())
    other = torch.where((t & 1) == 1, st.src[t >> 1], st.dst[t >> 1])
    assert bool((other >= 0).all()) and bool((other < N).all())
    # the lists are rebuilt identically by a second call on recycled memory (the fault showed on the SECOND call only)
    col_off2, keys2 = ops.cn_gather_backward_lists(adj._rowptr, adj._col, st.src, st.dst, st.off, st.flags, N)
    assert torch.equal(col_off2, col_off) and torch.equal(keys2, keys)


@pytest.mark.parametrize("n,avg,mx,B,H", [(500, 8, 100, 300, 32), (3000, 12, 400, 2048, 64), (20000, 10, 600, 8192, 256),
                                          (2000, 30, 1500, 4096, 128)], ids=lambda v: str(v))
@pytest.mark.parametrize("name", ["cn5", "cn7"])
def test_pooling_backward_is_deterministic_and_equals_the_atomic_form(hiplib, monkeypatch, name, n, avg, mx, B, H):
    """The node-by-node pooling backward (ocn_cn_gather_backward_det): the same bits on every run, and the atomic kernel's
    result to rounding (fp32 sums in another order)."""
    from ocn_amd.model import predictor_dict
    from ocn_amd.utils import adjoverlap
    from types import SimpleNamespace
    adj, adj2, e = _pool_case(n, avg, mx, B, H, seed=n + B)
    _assert_backward_key_lists(adj, adj2, e)
    torch.manual_seed(1)
    pred = predictor_dict[name](H, H, 1, 3, 0.0, 0.0, True).eval().to(DEV)
    x = torch.randn(n, H, device=DEV)
    wgt = torch.randn(B, 1, device=DEV)

    def grad():
        xd = x.clone().requires_grad_(True)
        out = pred(xd, adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e), e, SimpleNamespace(sum=1.0))
        (out * wgt).sum().backward()
        return xd.grad

    monkeypatch.setattr(ops, "deterministic_backward", True)
    a, b = grad(), grad()
    assert torch.equal(a, b)
    monkeypatch.setattr(ops, "deterministic_backward", False)
    c = grad()
    assert (a - c).abs().max().item() <= 2e-5 * max(1.0, c.abs().max().item())


def test_product_column_ids_are_deferred_until_read(hiplib):
    """A @ A on a graph whose product comes with dense bit rows: the counting pass, the scan of the row lengths and the bit rows
    are done at once, the FILL pass (and its host sync for the output size) only when the column ids are read — the
    intersection pass probes the bit rows and never reads them, so a training step that rebuilds A² per batch
    (NeighborOverlap_large.py:68-74) skips it.  Same flags, counts and histograms as with the ids present; the ids, once
    read, are the eager product's."""
    from oracle import ocn_oracle as O
    from ocn_amd.utils import CNState
    from tests.helpers import batch, make_graph, to_product
    oadj = make_graph(3000, 12, 400, seed=2)
    adj = to_product(oadj, DEV)
    sp = adj.to_torch_sparse_coo_tensor()
    lazy = SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False)
    assert lazy._bitmap is not None and not lazy.col_materialized()
    e = batch(oadj, 2048, 7).to(DEV)
    st = CNState(adj, adj, lazy, e)
    assert not lazy.col_materialized()                          # the intersection pass did not need them
    rowptr, col, _ = ops.spgemm_pattern(adj._rowptr, adj._col, adj._rowptr, adj._col, adj.size(1))      # the eager form
    eager = SparseTensor(rowptr=rowptr, col=col, sparse_sizes=adj.sparse_sizes())
    eager._bitmap = None                                        # ... searched as a CSR row, not probed
    ref = CNState(adj, adj, eager, e)
    assert torch.equal(st.flags[: int(st.off[-1])], ref.flags[: int(ref.off[-1])])
    assert torch.equal(st.cnt1, ref.cnt1) and torch.equal(st.cnt2, ref.cnt2) and torch.equal(st.hist, ref.hist)
    assert torch.equal(lazy._rowptr, rowptr)
    assert lazy.nnz() == col.numel() and lazy.col_materialized() and torch.equal(lazy._col, col)
    oadj2 = O.adj2_sparse(oadj)
    r, c, _ = lazy.coo()
    assert r.cpu().tolist() == oadj2.row.tolist() and c.cpu().tolist() == oadj2.col.tolist()


def test_product_rows_are_built_on_demand_under_autograd(hiplib, monkeypatch):
    """A @ A formed while autograd records, on a graph past the small-graph histogram (N > 8192): nothing is computed until
    somebody needs it.  The intersection pass asks for the bit rows of its candidates' TARGET rows (ocn_spgemm_bit_rows: each
    row built once, duplicates and later batches skip it) and gets the same flags, counts and histograms as from the whole
    product; anything that treats the product as a matrix completes it — the eager product's row pointers, ids and bit rows."""
    from ocn_amd.utils import CNState
    from tests.helpers import batch, make_graph, to_product
    n = 12000
    oadj = make_graph(n, 10, 300, seed=5, isolated=40)
    adj = to_product(oadj, DEV)
    sp = adj.to_torch_sparse_coo_tensor()
    assert torch.is_grad_enabled()
    lazy = SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False)
    assert lazy.rows_on_demand() and lazy.sizes() == [n, n] and lazy.device() == adj.device()
    with torch.no_grad():
        full = SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False)
    assert not full.rows_on_demand() and full._bitmap is not None
    e1, e2 = batch(oadj, 4096, 7).to(DEV), batch(oadj, 3000, 8).to(DEV)
    e2[1, :100] = e1[1, :100]                                   # rows of the first batch again
    e2[1, 100:200] = e2[1, 100]                                 # duplicates inside a batch
    seen = torch.zeros(n, dtype=torch.bool, device=DEV)
    for e in (e1, e2):
        st, ref = CNState(adj, adj, lazy, e), CNState(adj, adj, full, e)
        assert lazy.rows_on_demand()                            # the intersection pass did not complete it
        assert torch.equal(st.off, ref.off) and torch.equal(st.flags[: int(st.off[-1])], ref.flags[: int(ref.off[-1])])
        assert torch.equal(st.cnt1, ref.cnt1) and torch.equal(st.cnt2, ref.cnt2) and torch.equal(st.hist, ref.hist)
        seen[e[1]] = True
        assert torch.equal(lazy._done.bool(), seen)             # exactly the requested rows exist ...
        assert torch.equal(lazy._bitmap[seen], full._bitmap[seen])      # ... and they are the product's
    assert int(seen.sum()) < n // 2
    monkeypatch.setattr(ops, "_overlap_active", True)           # a loop with several phase-A streams: the whole product, once
    st = CNState(adj, adj, lazy, e1)
    monkeypatch.setattr(ops, "_overlap_active", False)
    assert not lazy.rows_on_demand() and torch.equal(st.hist, CNState(adj, adj, full, e1).hist)
    assert torch.equal(lazy._rowptr, full._rowptr) and torch.equal(lazy._bitmap, full._bitmap)
    assert lazy.nnz() == full.nnz() and torch.equal(lazy._col, full._col)
    lazy2 = SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False)                # completed by a matrix-level read
    assert lazy2.rows_on_demand() and lazy2.nnz() == full.nnz() and not lazy2.rows_on_demand()
    monkeypatch.setattr(ops, "lazy_product_rows", False)
    assert not SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False).rows_on_demand()


def test_every_consumer_of_a_product_holds_the_one_stream_rule(hiplib, monkeypatch):
    """Rows on demand are built on one stream only (``SparseTensor.probed_bit_rows``), for all four consumers of a product's
    bit rows: the flag pass, the A³-free cn3 pass, cn8's one-pass pooling and the 2-hop link heuristics.  On a graph just past
    the small-graph histogram, 96 candidates with repeated targets: outside a loop with phase-A side streams the product
    stays one, exactly the batch's target rows exist, and every output is bit-equal to the eager product's; inside such a
    loop (``ops._overlap_active``) the product is completed, once, with the same outputs."""
    from ocn_amd.heuristics import link_heuristics
    from ocn_amd.utils import CN8State, CNState, adjoverlap_3hop
    from tests.helpers import batch, make_graph, same_product, to_product
    n = ops.small_graph_cols() + 8
    oadj = make_graph(n, 6, 60, seed=11, isolated=40)
    adj = to_product(oadj, DEV)
    sp = adj.to_torch_sparse_coo_tensor()
    with torch.no_grad():
        full = SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False)
    assert torch.is_grad_enabled() and not full.rows_on_demand()
    e = batch(oadj, 96, 3).to(DEV)
    e[1, 32:64] = e[1, :32]                                     # targets of other candidates again ...
    e[1, 64:80] = e[1, 0]                                       # ... one target many times ...
    e[1, 95] = n - 1                                            # ... and an isolated one (an empty row of A²)
    seen = torch.zeros(n, dtype=torch.bool, device=DEV)
    seen[e[1]] = True
    x = torch.randn(n, 16, generator=torch.Generator().manual_seed(4)).to(DEV)

    def flag_pass(a2):
        st = CNState(adj, adj, a2, e)
        return st.off, st.flags[: int(st.off[-1])], st.cnt1, st.cnt2, st.hist

    def cn3_pass(a2):
        cn3 = adjoverlap_3hop(adj, a2, e)
        cnt, st = cn3.counts(), cn3._state
        return cnt, st.flags[: int(st.off[-1])], st.hist

    def cn8_pool(a2):
        st = CN8State(adj, adj, a2, e)
        return (*st.pool(x), st.cnt1, st.cnt2)

    def heuristics(a2):
        return (link_heuristics(adj, a2, e, kinds=("cn2", "aa2", "ra2")),)

    completed, complete = [], SparseTensor._complete
    monkeypatch.setattr(SparseTensor, "_complete", lambda self: (completed.append(self), complete(self))[1])
    for run in (flag_pass, cn3_pass, cn8_pool, heuristics):
        want = [t.clone() for t in run(full)]
        assert any(int(t.ne(0).sum()) for t in want), run.__name__
        for active in (False, True):
            lazy = SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False)
            assert lazy.rows_on_demand()
            monkeypatch.setattr(ops, "_overlap_active", active)
            got = run(lazy)
            monkeypatch.setattr(ops, "_overlap_active", False)
            assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), (run.__name__, active)
            if active:
                assert not lazy.rows_on_demand() and len(completed) == 1 and completed[0] is lazy, run.__name__
                same_product(lazy, full)
                completed.clear()
            else:
                assert lazy.rows_on_demand() and not completed, run.__name__
                assert torch.equal(lazy._done.bool(), seen), run.__name__       # exactly the batch's target rows exist ...
                assert torch.equal(lazy._bitmap[seen], full._bitmap[seen])      # ... and they are the product's
    # up to small_graph_cols() columns the flag pass reads T2's row lengths, so there (row_lengths=True) the cn3 pass completes too
    from ocn_amd.utils import _a2_bit_rows
    small = to_product(make_graph(300, 6, 40, seed=12), DEV)
    lazy = SparseTensor._lazy_product(small, small)
    bits = _a2_bit_rows(lazy, torch.arange(10, device=DEV))
    assert not lazy.rows_on_demand() and len(completed) == 1
    sp = small.to_torch_sparse_coo_tensor()
    assert torch.equal(bits, SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False).product_bit_rows())


@pytest.mark.parametrize("H,rows", [(32, 1000), (64, 4097), (256, 20000), (512, 333), (16, 70000)])
@pytest.mark.parametrize("ln,relu,p", [(True, True, 0.0), (True, True, 0.3), (False, True, 0.05), (True, False, 0.0), (False, False, 0.5)])
def test_ln_dropout_relu_tail_matches_torch_autograd(hiplib, H, rows, ln, relu, p):
    """ocn_ln_drop_relu_forward / _backward (the heads' tails under autograd): values and all three gradients against torch
    autograd of relu(LN(x) * keep / (1 - p)) with the SAME keep decisions (ocn_dropout_keep_mask), two runs bit-equal, and the
    keep rate is p's."""
    torch.manual_seed(H + rows)
    x = torch.randn(rows, H, device=DEV) * 2.0 + 0.3
    gamma = (torch.rand(H, device=DEV) + 0.5) if ln else None
    beta = torch.randn(H, device=DEV) if ln else None
    seed = 123456789 + H
    y, stats = ops.ln_drop_relu_forward(x, gamma, beta, 1e-5, p, seed, relu)
    keep = ops.dropout_keep_mask(seed, p, rows * H, DEV).view(rows, H).float() if p > 0 else torch.ones_like(x)
    if p > 0:
        assert abs(keep.mean().item() - (1 - p)) < 0.01
    xr = x.clone().requires_grad_(True)
    gr = gamma.clone().requires_grad_(True) if ln else None
    br = beta.clone().requires_grad_(True) if ln else None
    u = torch.nn.functional.layer_norm(xr, (H,), gr, br, 1e-5) if ln else xr
    d = u * keep / (1 - p)
    ref = torch.relu(d) if relu else d
    assert (y - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())
    g = torch.randn(rows, H, device=DEV)
    ref.backward(g)
    dx, dg, db = ops.ln_drop_relu_backward(g, x, y, stats, gamma, p, seed, relu)
    assert (dx - xr.grad).abs().max().item() <= 2e-5 * max(1.0, xr.grad.abs().max().item())
    if ln:
        assert (dg - gr.grad).abs().max().item() <= 2e-5 * max(1.0, gr.grad.abs().max().item()) * (rows ** 0.5)
        assert (db - br.grad).abs().max().item() <= 2e-5 * max(1.0, br.grad.abs().max().item()) * (rows ** 0.5)
    dx2, dg2, db2 = ops.ln_drop_relu_backward(g, x, y, stats, gamma, p, seed, relu)
    assert torch.equal(dx, dx2) and (not ln or (torch.equal(dg, dg2) and torch.equal(db, db2)))


def test_heads_tails_run_fused_under_autograd(hiplib, monkeypatch):
    """`_seq_train` routes the [LayerNorm] [Dropout] [ReLU] runs of the heads through the fused tail: with p = 0 the training-
    mode scores and every gradient equal the torch-module walk to rounding; with the drivers' dropout the step runs, is
    repeatable under torch.manual_seed, and the number of torch LayerNorm calls is zero."""
    from types import SimpleNamespace
    import torch.nn as nn
    from ocn_amd.model import predictor_dict
    from ocn_amd.utils import adjoverlap
    from tests.helpers import batch, make_graph, product_adj2, to_product
    n, H, B = 3000, 64, 2048
    oadj = make_graph(n, 12, 400, seed=2)
    adj = to_product(oadj, DEV)
    adj2 = product_adj2(adj)
    e = batch(oadj, B, 4).to(DEV)
    torch.manual_seed(5)
    x = torch.randn(n, H, device=DEV)

    def run(pred, fused, seed=0):
        monkeypatch.setattr(ops, "train_tails", fused)
        torch.manual_seed(seed)
        pred.zero_grad()
        xd = x.clone().requires_grad_(True)
        out = pred(xd, adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e), e, SimpleNamespace(sum=1.0))
        out.sum().backward()
        return out.detach().clone(), xd.grad.clone(), {k: p.grad.clone() for k, p in pred.named_parameters() if p.grad is not None}

    pred0 = predictor_dict["cn5"](H, H, 1, 3, 0.0, 0.0, True).to(DEV).train()        # dropout p = 0: both walks are deterministic
    a, b = run(pred0, True), run(pred0, False)
    assert (a[0] - b[0]).abs().max().item() <= 1e-5 and (a[1] - b[1]).abs().max().item() <= 2e-5 * max(1.0, b[1].abs().max().item())
    for k in b[2]:
        assert (a[2][k] - b[2][k]).abs().max().item() <= 2e-5 * max(1.0, b[2][k].abs().max().item()) * 8, k
    pred = predictor_dict["cn5"](H, H, 1, 3, 0.3, 0.0, True).to(DEV).train()
    calls = []
    hook = nn.LayerNorm.forward
    monkeypatch.setattr(nn.LayerNorm, "forward", lambda self, t: (calls.append(1), hook(self, t))[1])
    c, d = run(pred, True, seed=11), run(pred, True, seed=11)
    assert not calls and torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])
    assert not torch.equal(c[0], run(pred, True, seed=12)[0])                          # another seed, another mask


@pytest.mark.parametrize("shape", [(4, 4), (1000, 64), (65536, 256), (333, 32)])
def test_branch_mix_backward_matches_torch_autograd(hiplib, shape):
    """ocn_mix3_backward (model._MixFn: the branch mix alpha0 a + alpha1 b + beta c under autograd): the three input gradients
    and the three coefficient gradients against torch autograd, two runs bit-equal."""
    from ocn_amd.model import _MixFn
    torch.manual_seed(sum(shape))
    xs = [torch.randn(*shape, device=DEV) for _ in range(3)]
    coef = torch.tensor([0.7, -0.3, 1.1], device=DEV)
    g = torch.randn(*shape, device=DEV)
    refs = [t.clone().requires_grad_(True) for t in xs]
    cr = coef.clone().requires_grad_(True)
    (cr[0] * refs[0] + cr[1] * refs[1] + cr[2] * refs[2]).backward(g)
    ins = [t.clone().requires_grad_(True) for t in xs]
    cd = coef.clone().requires_grad_(True)
    z = _MixFn.apply(cd, *ins)
    assert torch.equal(z, (coef[0] * xs[0] + coef[1] * xs[1]) + coef[2] * xs[2])
    z.backward(g)
    for a, b in zip(ins, refs):
        assert torch.equal(a.grad, b.grad)
    n = g.numel()
    assert (cd.grad - cr.grad).abs().max().item() <= 1e-5 * max(1.0, cr.grad.abs().max().item()) * (n ** 0.5) / 10
    d = ops.mix3_backward(coef, g, *xs)
    d2 = ops.mix3_backward(coef, g, *xs)
    assert all(torch.equal(p, q) for p, q in zip(d, d2))
