"""GPU: the transposed pooling (pool_bwd.hip, cn_scatter.hip) against references that share none of its code.

Kernel level, on synthetic flags / walk counts / column weights (no intersection pass involved).  Every live entry
(e, k, key = off[e] + p) and the two endpoint terms of every candidate are listed in COO form on the CPU, then

(a) summed in fp64 with ``index_add_`` (``dh_ref``), next to the sum A of the absolute values of every product and the
    list length L of every node;
(b) summed in fp32 in the order the header of pool_bwd.hip states: per node in ascending key order, every product and
    every sum rounded separately, endpoint terms (keys >= cap) after all flag positions.

The deterministic kernel must equal (b) bit for bit.  Every form must be within gamma(L + 2) * A of (a), with
gamma(n) = n u / (1 - n u), u = 2^-24: a term costs at most two roundings before it is added (its products, their sum — a
fused multiply-add costs fewer), and a node's L terms are joined by at most L additions, in whatever order; the cn6
backward has one product and one sum more per term, hence L + 3.  No figure in this file was read off the kernels.

Model level: gradients through ``get_cn1_cn2`` (walk counts as cn2 values) and the micro-batch protocol of the ppa
driver against torch autograd through the oracle.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

from oracle import ocn_oracle as O
from ocn_amd import _lib, ops
from tests.helpers import batch, close, make_graph, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
WIDTHS = [16, 32, 64, 128, 256, 512]


# ---- inputs --------------------------------------------------------------------------------------------------------
def _csr(n, row, col):
    """Symmetric CSR of the undirected edges (row, col): int64 rowptr, int32 columns ascending, no duplicates."""
    key = torch.unique(torch.cat([row * n + col, col * n + row]))
    r, c = torch.div(key, n, rounding_mode="floor"), key % n
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
    return rowptr, c.to(torch.int32)


def _nonzero_randn(shape, g):
    w = torch.randn(*shape, generator=g)
    return torch.where(w >= 0, w + 0.25, w - 0.25)


def _case(rowptr, col, src, dst, H, walk, seed, all_flags=False):
    """CPU tensors of one call, and ``d``: the same on the device."""
    g = torch.Generator().manual_seed(seed)
    N, B = rowptr.numel() - 1, src.numel()
    deg = rowptr[src + 1] - rowptr[src]
    off = torch.zeros(B + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(deg, 0)
    cap = int(off[B])
    assert cap > 0
    if all_flags:
        flags = torch.randint(1, 4, (cap,), generator=g)
    else:                                                       # {0, 1, 2, 3}, about half zero
        flags = torch.randint(0, 4, (cap,), generator=g) * (torch.rand(cap, generator=g) < 2.0 / 3.0)
    flags = flags.to(torch.uint8)
    wc = None
    if walk:
        wc = torch.where((flags & 2) != 0, torch.randint(1, 1001, (cap,), generator=g), torch.zeros((), dtype=torch.int64))
        wc = wc.to(torch.int32)
    weights = torch.randn(N, 4, generator=g)
    weights[:, 1:3] = _nonzero_randn((N, 2), g)                 # the trained-innerprod shape: cn1-only entries carry a wb
    c = SimpleNamespace(N=N, B=B, H=H, cap=cap, walk=walk, rowptr=rowptr, col=col, src=src, dst=dst, off=off, flags=flags,
                        wc=wc, weights=weights, h=torch.randn(N, H, generator=g), g1=torch.randn(B, H, generator=g),
                        g2=torch.randn(B, H, generator=g), g3=torch.randn(B, H, generator=g),
                        order=torch.randperm(B, generator=g))
    names = ("rowptr", "col", "src", "dst", "off", "flags", "wc", "weights", "h", "g1", "g2", "g3", "order")
    c.d = SimpleNamespace(**{k: (None if getattr(c, k) is None else getattr(c, k).to(DEV)) for k in names})
    return c


def _entries(c, flags):
    """Every position of the flag array as (candidate e, column k, key), and which of them are live."""
    deg = c.off[1:] - c.off[:-1]
    e = torch.repeat_interleave(torch.arange(c.B), deg)
    key = torch.arange(c.cap)
    k = c.col[c.rowptr[c.src[e]] + key - c.off[e]].long()
    return e, k, key, flags != 0


def _reference(c, dh0=None):
    """(a) and (b) of the module docstring for ops.cn_gather_backward, started from ``dh0`` (zeros by default)."""
    e, k, key, live = _entries(c, c.flags)
    e, k, key, f = e[live], k[live], key[live], c.flags[live].int()
    w = c.weights[k]
    zero = torch.zeros(())
    cn1, cn2 = (f & 1) != 0, (f & 2) != 0
    cval = c.wc[live].float() if c.walk else torch.ones(e.numel())
    wa = torch.where(cn1, w[:, 0], zero)                        # entry_weights (common.h): subtract, then multiply
    wb = (torch.where(cn2, cval, zero) - torch.where(cn1, w[:, 1], zero)) * w[:, 2]
    assert wa.dtype == torch.float32 and wb.dtype == torch.float32
    eb = torch.arange(c.B)
    node = torch.cat([k, c.src, c.dst])
    keys = torch.cat([key, c.cap + 2 * eb, c.cap + 2 * eb + 1])
    L = torch.bincount(node, minlength=c.N)
    # (a) fp64
    dh0 = torch.zeros(c.N, c.H) if dh0 is None else dh0
    ref, A = dh0.double().clone(), dh0.double().abs()
    pa, pb = wa.double()[:, None] * c.g1[e].double(), wb.double()[:, None] * c.g2[e].double()
    ps, pd = c.g3.double() * c.h[c.dst].double(), c.g3.double() * c.h[c.src].double()
    ref.index_add_(0, node, torch.cat([pa + pb, ps, pd]))
    A.index_add_(0, node, torch.cat([pa.abs() + pb.abs(), ps.abs(), pd.abs()]))
    # (b) fp32, one rounding per operation (torch's elementwise ops do not fuse), rank by rank over the sorted lists
    terms = torch.cat([(wa[:, None] * c.g1[e]) + (wb[:, None] * c.g2[e]), c.g3 * c.h[c.dst], c.g3 * c.h[c.src]])
    perm = torch.argsort(node * (1 << 32) + keys)
    terms, keys = terms[perm], keys[perm]
    col_off = torch.zeros(c.N + 1, dtype=torch.int64)
    col_off[1:] = torch.cumsum(L, 0)
    by_len = torch.argsort(L, descending=True)
    longer = c.N - torch.searchsorted(torch.sort(L).values, torch.arange(int(L.max())), right=True)   # nodes with L > r
    emu = dh0.clone()
    for r, m in enumerate(longer.tolist()):
        nodes = by_len[:m]
        emu[nodes] = emu[nodes] + terms[col_off[nodes] + r]
    assert emu.dtype == torch.float32
    return SimpleNamespace(ref=ref, A=A, L=L, emu=emu, col_off=col_off, keys=keys.to(torch.int32))


def _gamma(n):
    n = n.double()
    return n * U / (1.0 - n * U)


def _assert_within_bound(dh, r, extra, what):
    err = (dh.double() - r.ref).abs()
    bound = _gamma(r.L + extra)[:, None] * r.A
    worst = (err / bound.clamp(min=1e-300)).max().item()
    print(f"{what}: max |dh - ref| = {err.max().item():.3e}, largest share of the bound used = {worst:.3f}")
    assert bool((err <= bound).all()), what


def _backward(c, monkeypatch, det, order=None):
    monkeypatch.setattr(ops, "deterministic_backward", det)
    d = c.d
    return ops.cn_gather_backward(d.rowptr, d.col, d.src, d.dst, d.off, d.flags, d.wc, d.weights, d.h, d.g1, d.g2, d.g3,
                                  order=order).cpu()


def _check(c, monkeypatch, list_len=None):
    """All assertions of one case; ``list_len`` = (node, expected number of keys)."""
    r = _reference(c)
    d = c.d
    col_off, keys = ops.cn_gather_backward_lists(d.rowptr, d.col, d.src, d.dst, d.off, d.flags, c.N)
    col_off, keys = col_off.cpu(), keys.cpu()
    if list_len is not None:
        node, want = list_len
        assert int(r.L[node]) == want and int(col_off[node + 1] - col_off[node]) == want
    assert torch.equal(col_off, r.col_off) and torch.equal(keys, r.keys)
    a, b = _backward(c, monkeypatch, True), _backward(c, monkeypatch, True)
    diff = a != r.emu
    print(f"deterministic vs ordered emulation: {int(diff.sum())} of {diff.numel()} elements differ, "
          f"max |diff| = {(a - r.emu).abs().max().item():.3e}, longest list {int(r.L.max())}")
    assert torch.equal(a, b), "two runs of the deterministic form"
    assert torch.equal(a, r.emu), "the summation order of pool_bwd.hip"
    _assert_within_bound(a, r, 2, "deterministic")
    _assert_within_bound(r.emu, r, 2, "emulation")
    _assert_within_bound(_backward(c, monkeypatch, False), r, 2, "atomic, batch order")
    _assert_within_bound(_backward(c, monkeypatch, False, order=d.order), r, 2, "atomic, permuted")
    return r


# ---- graphs and batches --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chung_lu(n, avg, mx, seed, isolated):
    oadj = make_graph(n, avg, mx, seed, isolated=isolated)
    return oadj, _csr(n, oadj.row, oadj.col)


def _widths_batch():
    """n = 500, B = 300: 5 self pairs, 5 duplicated candidates, 5 candidates with an isolated source; the first and the last
    candidate have non-empty rows."""
    n, B = 500, 300
    oadj, (rowptr, col) = _chung_lu(n, 8, 100, 21, 10)
    deg = rowptr[1:] - rowptr[:-1]
    assert int(deg[n - 10:].sum()) == 0
    busy = torch.nonzero(deg > 0).flatten()
    e = batch(oadj, B, 26).clone()
    e[:, 10:15] = busy[7:12]                                    # (i, i)
    e[:, 20:25] = e[:, 30:35]                                   # duplicates
    e[0, 40:45] = torch.arange(n - 5, n)                        # da = 0 rows
    e[0, 0], e[0, B - 1] = busy[0], busy[-1]
    assert int(deg[e[0, 0]]) > 0 and int(deg[e[0, B - 1]]) > 0 and int((deg[e[0]] == 0).sum()) >= 5
    return rowptr, col, e[0].contiguous(), e[1].contiguous()


def _star(leaves, extra_nodes=0):
    """Node 0 adjacent to nodes 1 .. leaves; ``extra_nodes`` further ids without edges."""
    lv = torch.arange(1, leaves + 1)
    return _csr(leaves + 1 + extra_nodes, torch.zeros(leaves, dtype=torch.int64), lv)


def _leaf_pairs(leaves, B, g, base=0):
    """B candidates (leaf, other leaf) of the star whose hub is ``base``."""
    a = torch.randint(0, leaves, (B,), generator=g)
    b = (a + torch.randint(1, leaves, (B,), generator=g)) % leaves
    return base + 1 + a, base + 1 + b


# ---- ops.cn_gather_backward ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", [False, True], ids=["pattern", "walk"])
@pytest.mark.parametrize("H", WIDTHS)
def test_widths(hiplib, monkeypatch, H, walk):
    """Every LPE / NV instance of both kernels (H = 512: pb_accumulate_kernel<2>, cn_scatter_kernel<64, 2>), lanes >= H / 4
    idle, empty rows inside the binary search over ``off``; pattern route and walk route (wc != NULL)."""
    rowptr, col, src, dst = _widths_batch()
    _check(_case(rowptr, col, src, dst, H, walk, seed=100 + H), monkeypatch)


@pytest.mark.parametrize("walk", [False, True], ids=["pattern", "walk"])
@pytest.mark.parametrize("n", [64, 63])
@pytest.mark.parametrize("B", [1, 37])
def test_tiny(hiplib, monkeypatch, B, n, walk):
    """A partial last wave / lane group of the atomic kernel and a partial last workgroup of the node-by-node kernel
    (n = 63: N no multiple of 4)."""
    oadj, (rowptr, col) = _chung_lu(n, 5, 20, 3, 3)
    e = batch(oadj, B, 9).clone()
    e[0, 0] = torch.argmax(rowptr[1:] - rowptr[:-1])             # at least one non-empty row
    _check(_case(rowptr, col, e[0].contiguous(), e[1].contiguous(), 64, walk, seed=B + n), monkeypatch)


@pytest.mark.parametrize("walk", [False, True], ids=["pattern", "walk"])
@pytest.mark.parametrize("H", [32, 512])
@pytest.mark.parametrize("keys", [1, 3, 63, 64, 65, 66, 127, 129])
def test_list_lengths(hiplib, monkeypatch, keys, H, walk):
    """A hub whose list has exactly ``keys`` entries (one per candidate: leaf pairs, every flag set): the wave sort / long sort
    boundary at 64 | 65, a second round of 1, 2, 63 keys, round tails with m % 4 in {1, 2, 3}."""
    rowptr, col = _star(140)
    src, dst = _leaf_pairs(140, keys, torch.Generator().manual_seed(keys))
    _check(_case(rowptr, col, src, dst, H, walk, seed=keys + H, all_flags=True), monkeypatch, list_len=(0, keys))


def test_endpoint_only_node(hiplib, monkeypatch):
    """A node that is an endpoint of 70 candidates and nobody's common neighbour: a (long) list of keys all >= cap."""
    leaves = 100
    x, y, n = leaves + 1, leaves + 2, leaves + 3
    lv = torch.arange(1, leaves + 1)
    rowptr, col = _csr(n, torch.cat([torch.zeros(leaves, dtype=torch.int64), torch.tensor([x])]), torch.cat([lv, torch.tensor([y])]))
    g = torch.Generator().manual_seed(70)
    other = 1 + torch.randint(0, leaves, (70,), generator=g)
    swap = torch.arange(70) % 2 == 0
    xs = torch.full((70,), x)
    src, dst = torch.where(swap, xs, other), torch.where(swap, other, xs)          # y is never a source: x is never a column
    more = _leaf_pairs(leaves, 30, g)
    c = _case(rowptr, col, torch.cat([src, more[0]]), torch.cat([dst, more[1]]), 64, True, seed=71, all_flags=True)
    r = _check(c, monkeypatch, list_len=(x, 70))
    assert bool((r.keys[r.col_off[x]: r.col_off[x + 1]] >= c.cap).all())


def test_in_memory_sort(hiplib, monkeypatch):
    """A hub list longer than the 12 288 keys cc_sort_long_kernel sorts in LDS: 13 000 leaf pairs of a 200-leaf star, and the
    hub's own endpoint terms from four candidates it is an end of."""
    rowptr, col = _star(200)
    g = torch.Generator().manual_seed(13)
    src, dst = _leaf_pairs(200, 13000, g)
    hub, lf = torch.zeros(2, dtype=torch.int64), torch.tensor([5, 77])
    c = _case(rowptr, col, torch.cat([src, hub, lf]), torch.cat([dst, lf, hub]), 16, True, seed=14, all_flags=True)
    _check(c, monkeypatch, list_len=(0, 13006))                 # 13 002 sources adjacent to the hub + its 4 endpoint terms


def test_many_long_lists(hiplib, monkeypatch):
    """300 disjoint stars of 70 leaves with 70 candidates each: 300 lists of 70 keys, more than the 256 workgroups of the
    long-list launch (its ticket loop)."""
    stars, leaves = 300, 70
    hubs = torch.arange(stars) * (leaves + 1)
    row = hubs.repeat_interleave(leaves)
    colx = row + 1 + torch.arange(leaves).repeat(stars)
    rowptr, col = _csr(stars * (leaves + 1), row, colx)
    g = torch.Generator().manual_seed(300)
    a, b = _leaf_pairs(leaves, stars * leaves, g)
    base = hubs.repeat_interleave(leaves)
    c = _case(rowptr, col, base + a, base + b, 16, False, seed=301, all_flags=True)
    r = _check(c, monkeypatch, list_len=(int(hubs[-1]), leaves))
    assert int((r.L > 64).sum()) >= stars


def test_stride_loops(hiplib, monkeypatch):
    """N = 530 000 (> 131 072: the capped grids of pb_accumulate_kernel and cc_sort_short_kernel; > 524 288: pb_zero_kernel),
    B = 270 000 (> 262 144: pb_entries_kernel).  Average degree 2, so the lists and the emulation loop are short."""
    n, B = 530000, 270000
    g = torch.Generator().manual_seed(53)
    rowptr, col = _csr(n, torch.randint(0, n, (n,), generator=g), torch.randint(0, n, (n,), generator=g))
    src, dst = torch.randint(0, n, (B,), generator=g), torch.randint(0, n, (B,), generator=g)
    _check(_case(rowptr, col, src, dst, 16, True, seed=54), monkeypatch)


@pytest.mark.parametrize("walk", [False, True], ids=["pattern", "walk"])
def test_both_entries_add_into_dh(hiplib, walk):
    """ocn_cn_gather_backward_det and ocn_cn_gather_backward add into ``dh``: called as ops.cn_gather_backward calls them, on a
    preloaded dh.  The ordered sum starts from dh's value; |dh0| joins A (it is one more summand of the node's sum)."""
    rowptr, col, src, dst = _widths_batch()
    c = _case(rowptr, col, src, dst, 64, walk, seed=640)
    dh0 = torch.randn(c.N, c.H, generator=torch.Generator().manual_seed(641))
    r = _reference(c, dh0)
    d, l = c.d, _lib.lib()
    p, sp = _lib.ptr, _lib.stream_ptr
    dh = dh0.to(DEV)
    ws = torch.empty(int(l.ocn_cn_gather_backward_det_workspace_bytes(c.N, c.B, c.cap)), dtype=torch.uint8, device=DEV)
    _lib.check(l.ocn_cn_gather_backward_det(p(d.rowptr), p(d.col), p(d.src), p(d.dst), c.B, p(d.off), p(d.flags), p(d.wc), c.cap,
                                            p(d.weights), p(d.h), c.N, c.H, p(d.g1), p(d.g2), p(d.g3), p(dh), p(ws), sp()),
               "ocn_cn_gather_backward_det")
    got = dh.cpu()
    print(f"{int((got != r.emu).sum())} elements differ from the emulation")
    assert torch.equal(got, r.emu)
    _assert_within_bound(got, r, 2, "deterministic, preloaded")
    for order in (None, d.order):
        dh = dh0.to(DEV)
        _lib.check(l.ocn_cn_gather_backward(p(d.rowptr), p(d.col), p(d.src), p(d.dst), p(order), c.B, p(d.off), p(d.flags), p(d.wc),
                                            p(d.weights), p(d.h), c.H, p(d.g1), p(d.g2), p(d.g3), p(dh), sp()),
                   "ocn_cn_gather_backward")
        _assert_within_bound(dh.cpu(), r, 2, "atomic, preloaded")


# ---- ops.cn_gather3_backward (cn6) -----------------------------------------------------------------------------------
def _check3(c, seed):
    """cn_scatter3_kernel against the fp64 COO sum of w1 g1 + w2 g2 + w3 g3 and the endpoint terms of g4; w2 and w3 formed in
    fp32 in the kernel's order, then cast."""
    g = torch.Generator().manual_seed(seed)
    flagsB = torch.randint(0, 4, (c.cap,), generator=g).to(torch.uint8)     # only bit 1 of the second array is read
    wA, wB = c.weights, _nonzero_randn((c.N, 4), g)
    nip = torch.tensor([0.37]) * (1.0 + torch.rand(1, generator=g))
    g4 = torch.randn(c.B, c.H, generator=g)
    fb_all = flagsB & 1
    e, k, _, live = _entries(c, c.flags | fb_all)
    e, k, fa, fb = e[live], k[live], c.flags[live].int(), fb_all[live] != 0
    a, inv3 = wA[k], wB[k][:, 0]
    zero, one = torch.zeros(()), torch.ones(())
    cn1, cn2 = (fa & 1) != 0, (fa & 2) != 0
    tt = torch.where(cn1, a[:, 1], zero)
    w1 = torch.where(cn1, a[:, 0], zero)
    w2 = (torch.where(cn2, one, zero) - tt) * a[:, 2]
    w3 = ((torch.where(fb, one, zero) - tt) - nip * w2) * inv3
    assert w2.dtype == torch.float32 and w3.dtype == torch.float32
    node = torch.cat([k, c.src, c.dst])
    L = torch.bincount(node, minlength=c.N)
    p1, p2, p3 = (w.double()[:, None] * t[e].double() for w, t in ((w1, c.g1), (w2, c.g2), (w3, c.g3)))
    ps, pd = g4.double() * c.h[c.dst].double(), g4.double() * c.h[c.src].double()
    ref = torch.zeros(c.N, c.H, dtype=torch.float64).index_add_(0, node, torch.cat([p1 + p2 + p3, ps, pd]))
    A = torch.zeros(c.N, c.H, dtype=torch.float64).index_add_(0, node, torch.cat([p1.abs() + p2.abs() + p3.abs(), ps.abs(), pd.abs()]))
    r = SimpleNamespace(ref=ref, A=A, L=L)
    d = c.d
    dev = [t.to(DEV) for t in (flagsB, wA, wB, nip, g4)]
    for order in (None, d.order):
        dh = ops.cn_gather3_backward(d.rowptr, d.col, d.src, d.dst, d.off, d.flags, dev[0], dev[1], dev[2], dev[3], d.h,
                                     d.g1, d.g2, d.g3, dev[4], order=order)
        _assert_within_bound(dh.cpu(), r, 3, "cn6, atomic")


@pytest.mark.parametrize("H", WIDTHS)
def test_cn6_backward_widths(hiplib, H):
    rowptr, col, src, dst = _widths_batch()
    _check3(_case(rowptr, col, src, dst, H, False, seed=600 + H), seed=H)


@pytest.mark.parametrize("B", [1, 37])
def test_cn6_backward_tiny(hiplib, B):
    oadj, (rowptr, col) = _chung_lu(63, 5, 20, 3, 3)
    e = batch(oadj, B, 9).clone()
    e[0, 0] = torch.argmax(rowptr[1:] - rowptr[:-1])
    _check3(_case(rowptr, col, e[0].contiguous(), e[1].contiguous(), 64, False, seed=B), seed=B)


# ---- training through the walk route ---------------------------------------------------------------------------------
PARITY = [(64, 5, 20, 37, 0, 3), (500, 8, 100, 300, 1, 10)]     # the two smallest CASES of tests/test_parity_gpu.py


@functools.lru_cache(maxsize=None)
def _walk_case(i):
    n, avg, mx, B, seed, iso = PARITY[i]
    oadj = make_graph(n, avg, mx, seed, isolated=iso)
    e = batch(oadj, B, seed + 50)
    return SimpleNamespace(n=n, B=B, seed=seed, oadj=oadj, e=e, adj=to_product(oadj, DEV))


def _predictor(name, H, ip):
    from ocn_amd.model import predictor_dict
    pred = predictor_dict[name](H, H, 1, 3, 0.0, 0.0, True).eval()       # eval + enable_grad: no dropout noise
    with torch.no_grad():
        pred.innerprod.fill_(ip)
    return pred


def _leaves(module):
    return {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in module.state_dict().items()}


def _oracle_scores(name, sd, x, cn1, cn2, e):
    return O.cn5_forward(sd, x, cn1, cn2, e, True) if name == "cn5" else O.cn7_forward(sd, x, cn1, cn2, e, 1.0, True)


def _assert_grads(module, sd, got_x, ref_x, what):
    """The bar of test_backward_matches_oracle_autograd: <= 2e-5 * max(1, |g|max), for x and every used parameter."""
    err, scale = (got_x.cpu() - ref_x).abs().max().item(), ref_x.abs().max().item()
    print(f"{what}: x: |diff| = {err:.3e}, |g|max = {scale:.3e}")
    assert err <= 2e-5 * max(1.0, scale), what
    for k, p in module.named_parameters():
        g = sd[k].grad
        if g is None:
            assert p.grad is None or p.grad.abs().max().item() == 0.0, k      # xcnlin / xcn4lin are never used
            continue
        err, scale = (p.grad.cpu() - g).abs().max().item(), g.abs().max().item()
        print(f"{what}: {k}: |diff| = {err:.3e}, |g|max = {scale:.3e}")
        assert err <= 2e-5 * max(1.0, scale), (what, k)


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "atomic"])
@pytest.mark.parametrize("ip", [0.0, 0.37])
@pytest.mark.parametrize("name", ["cn5", "cn7"])
@pytest.mark.parametrize("i", [0, 1], ids=["n64_B37", "n500_B300"])
def test_walk_route_gradients_match_oracle_autograd(hiplib, monkeypatch, i, name, ip, det):
    """Gradients w.r.t. the embeddings and every used parameter through ``get_cn1_cn2`` (cn2 valued with walk counts),
    against torch autograd through the oracle on ``O.get_cn1_cn2``."""
    from ocn_amd.utils import get_cn1_cn2
    case, H = _walk_case(i), 32
    torch.manual_seed(case.seed + 17)
    x = torch.randn(case.n, H)
    pred = _predictor(name, H, ip)
    sd = _leaves(pred)
    xr = x.clone().requires_grad_(True)
    ref = _oracle_scores(name, sd, xr, *O.get_cn1_cn2(case.oadj, case.e), case.e)
    wgt = torch.randn(case.B, 1, generator=torch.Generator().manual_seed(1))
    (ref * wgt).sum().backward()
    monkeypatch.setattr(ops, "deterministic_backward", det)
    pred = pred.to(DEV)
    e = case.e.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    out = pred(xd, case.adj, *get_cn1_cn2(case.adj, e), e, SimpleNamespace(sum=1.0))
    assert out.requires_grad and close(out, ref), (out.detach().cpu() - ref).abs().max()
    (out * wgt.to(DEV)).sum().backward()
    _assert_grads(pred, sd, xd.grad, xr.grad, f"{name} ip={ip}")


@pytest.mark.parametrize("name", ["cn5", "cn7"])
def test_ppa_micro_batch_protocol(hiplib, monkeypatch, name):
    """h = h0.detach().requires_grad_(); slices of 128 candidates out of 300, each with its own get_cn1_cn2, predictor call and
    backward(), the gradients accumulating in h.grad and in the parameters; then h0.backward(h.grad) through a one-layer GCN.
    The same loop on the oracle, the same bar; two runs of the deterministic backward give the same bits."""
    import ocn_amd.model as M
    from ocn_amd.utils import get_cn1_cn2
    case, H, step = _walk_case(1), 32, 128
    torch.manual_seed(case.seed + 23)
    x = torch.randn(case.n, H)
    enc = M.GCN(H, H, H, 1, 0.0, True, False, -1, "puregcn", True).eval()
    pred = _predictor(name, H, 0.37)
    wgt = torch.randn(case.B, 1, generator=torch.Generator().manual_seed(2))
    slices = [slice(s, min(s + step, case.B)) for s in range(0, case.B, step)]
    assert len(slices) == 3

    sde, sdp = _leaves(enc), _leaves(pred)
    xr = x.clone().requires_grad_(True)
    h0 = O.gcn_forward(sde, xr, case.oadj, num_layers=1, conv_fn="puregcn", ln=True, res=False, jk=True, max_x=-1, variant=1)
    h = h0.detach().requires_grad_()
    for s in slices:
        e = case.e[:, s].contiguous()
        (_oracle_scores(name, sdp, h, *O.get_cn1_cn2(case.oadj, e), e) * wgt[s]).sum().backward()
    h0.backward(h.grad)

    enc, pred = enc.to(DEV), pred.to(DEV)

    def run():
        enc.zero_grad(set_to_none=True)
        pred.zero_grad(set_to_none=True)
        xd = x.to(DEV).requires_grad_(True)
        d0 = enc(xd, case.adj)
        dh = d0.detach().requires_grad_()
        for s in slices:
            e = case.e[:, s].contiguous().to(DEV)
            out = pred(dh, case.adj, *get_cn1_cn2(case.adj, e), e, SimpleNamespace(sum=1.0))
            (out * wgt[s].to(DEV)).sum().backward()
        d0.backward(dh.grad)
        grads = {k: p.grad.clone() for m in (enc, pred) for k, p in m.named_parameters() if p.grad is not None}
        return d0.detach(), dh.grad.clone(), xd.grad.clone(), grads

    monkeypatch.setattr(ops, "deterministic_backward", True)
    a, b = run(), run()
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert a[3].keys() == b[3].keys() and all(torch.equal(a[3][k], b[3][k]) for k in a[3])
    for det in (True, False):
        monkeypatch.setattr(ops, "deterministic_backward", det)
        d0, gh, gx, _ = run()
        assert close(d0, h0, atol=2e-5, rtol=2e-5)
        err, scale = (gh.cpu() - h.grad).abs().max().item(), h.grad.abs().max().item()
        print(f"h.grad: |diff| = {err:.3e}, |g|max = {scale:.3e}")
        assert err <= 2e-5 * max(1.0, scale)
        _assert_grads(pred, sdp, gx, xr.grad, f"{name} det={det} predictor")
        _assert_grads(enc, sde, gx, xr.grad, f"{name} det={det} encoder")
