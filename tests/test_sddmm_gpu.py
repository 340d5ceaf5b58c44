"""GPU: ``ocn_sddmm_csr`` — the sampled dense-dense product on the pattern of an encoder operator — against fp64 at every width
and in every form the encoders use, against a known answer that needs no reference, its bits fixed by its input (two runs; the
rows of a sub-matrix), its row sums against the forward ``ocn_spmm_csr``, and under autograd as ``_MaskedSpmmFn``.

The coefficient c of an entry is restated on the host in fp32, each product rounded separately, exactly as the contract in
include/ocn_hip.h words it: no extra ulp is granted for it.  The dot product is a chain of at most F / LPE <= 8 fused
multiply-adds per lane and log2(LPE) <= 6 butterfly additions, and fl(c * d) rounds once more: at most F + 2 roundings for every
F >= 16, which is the bound (F + 2) u |c| sum|g x| of ``check_against_fp64`` in tests/test_explain_gpu.py."""
from types import SimpleNamespace

import pytest
import torch

from tests.helpers import csr_of_rows, make_graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WIDTHS = (16, 32, 64, 128, 256, 512)
U = 2.0 ** -24
SENTINEL = 12345.0
N, HUB, LOOP = 1301, 1300, 7                                             # rows 1298 and 1299 are isolated


def bits(t):
    """int32 view of an fp32 tensor on the host: compared this way the signs of zeros count."""
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def graph(hiplib):
    """A symmetric Chung-Lu graph on 1 298 nodes, two isolated rows, a hub joined to 1 100 others (its row is longer than 1 024
    and than any run of entries a work item takes) and one explicit self loop (LOOP, LOOP)."""
    o = make_graph(1300, 8, 100, 23, isolated=2)
    gen = torch.Generator().manual_seed(5)
    spokes = torch.randperm(1298, generator=gen)[:1100]
    hub = torch.full_like(spokes, HUB)
    r = torch.cat([o.row, hub, spokes, torch.tensor([LOOP])])
    c = torch.cat([o.col, spokes, hub, torch.tensor([LOOP])])
    key = torch.unique(r * N + c)                                        # sorted: rows ascending, columns ascending within a row
    row, col = key // N, key % N
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=N), 0)
    lens = rowptr[1:] - rowptr[:-1]
    assert int(lens[HUB]) == 1100 > 1024 and int(lens[1298]) == 0 and int(lens[1299]) == 0
    loop_pos = int(torch.nonzero((row == LOOP) & (col == LOOP)))
    assert int(((row == col).sum())) == 1
    nnz = int(col.numel())
    pre = torch.rand(N, generator=gen) + 0.1
    post = torch.rand(N, generator=gen) + 0.1
    val = torch.rand(nnz, generator=gen) + 0.5
    d = SimpleNamespace(rowptr=rowptr.to(DEV), col=col.to(torch.int32).to(DEV), pre=pre.to(DEV), post=post.to(DEV), val=val.to(DEV))
    return SimpleNamespace(n=N, nnz=nnz, rowptr=rowptr, row=row, col=col, lens=lens, loop_pos=loop_pos, pre=pre, post=post, val=val, d=d)


# the forms of the encoders (model.py): name -> which operands, and the keywords
FORMS = {
    "plain":     ((), dict()),
    "puregcn":   (("pre", "post"), dict(edge_scale=False, self_mode=1)),
    "gcn":       (("pre",), dict(edge_scale=True, self_mode=2)),
    "pureconv2": (("pre",), dict(edge_scale=True)),
    "mean":      ((), dict(mode="mean")),
    "valued":    (("pre", "post", "val"), dict(edge_scale=True)),
    "valued_mean": (("val",), dict(mode="mean")),
}


def coefficient(c, form):
    """c of every entry in fp32 on the host, each product rounded separately, in the contract's order."""
    names, kw = FORMS[form]
    w = torch.ones(c.nnz)
    if "pre" in names:
        w = c.pre[c.row] * c.pre[c.col] if kw.get("edge_scale") else c.pre[c.col].clone()
    if "val" in names:
        w = c.val * w
    if "post" in names:
        w = c.post[c.row] * w
    if kw.get("mode") == "mean":
        w = w / c.lens[c.row].to(torch.float32)
    assert w.dtype == torch.float32
    return w


def operands(F, seed, n=N):
    """Random g and x; g scaled by 1e-3, 1 and 30 across three thirds of the rows."""
    gen = torch.Generator().manual_seed(seed)
    scale = torch.tensor([1e-3, 1.0, 30.0]).repeat_interleave((n + 2) // 3)[:n, None]
    return torch.randn(n, F, generator=gen) * scale, torch.randn(n, F, generator=gen)


def run(c, form, g, x, out=None):
    from ocn_amd import ops
    names, kw = FORMS[form]
    return ops.sddmm_csr(c.d.rowptr, c.d.col, g, x, out=out, **{k: getattr(c.d, k) for k in names}, **kw)


@pytest.mark.parametrize("F", WIDTHS)
def test_sddmm_against_fp64_every_width(graph, F):
    c = graph
    g, x = operands(F, 10 + F)
    gd, xd = g.to(DEV), x.to(DEV)
    prod = g.double()[c.row] * x.double()[c.col]
    d64, mass = prod.sum(1), prod.abs().sum(1)
    for form in FORMS:
        buf = torch.full((c.nnz + 64,), SENTINEL, device=DEV)
        out = run(c, form, gd, xd, out=buf)
        assert out.shape == (c.nnz,) and out.data_ptr() == buf.data_ptr()
        got = buf.cpu()
        assert bool((got[c.nnz:] == SENTINEL).all())                    # nothing beyond nnz is written
        coef = coefficient(c, form).double()
        live = coef != 0
        if FORMS[form][1].get("self_mode") == 2:
            live[c.loop_pos] = False
            assert int(bits(got[c.loop_pos])) == 0                      # +0: the forward replaces the entry by the self term
        err = (got[:c.nnz].double() - coef * d64).abs()
        bound = (F + 2) * U * coef.abs() * mass + 1e-37
        worst = (err[live] / bound[live]).max().item()
        print(f"sddmm F={F} {form}: {int(live.sum())} live entries, worst error / bound = {worst:.3f}")
        assert int(live.sum()) >= 2000 and bool((err[live] <= bound[live]).all()), (form, worst)
        assert bool(torch.isfinite(got[:c.nnz]).all())
    assert torch.equal(gd.cpu(), g) and torch.equal(xd.cpu(), x)


@pytest.mark.parametrize("F", WIDTHS)
def test_sddmm_known_answer_identity_x(hiplib, F):
    """N = F nodes with x = I: <g[r], x[k]> = g[r][k] exactly, every other product is an exact zero.  A star (node 0 joined to
    nodes 1 .. N/2 - 1), the path 1 - 2 - .. - N-1 and a self loop at node 3, power-of-two coefficients: out[p] is bit for bit
    c g[r][k], and +0 at the self loop under self_mode 2."""
    from ocn_amd import ops
    n = F
    rows = [set() for _ in range(n)]
    for k in range(1, n // 2):
        rows[0].add(k); rows[k].add(0)
    for k in range(1, n - 1):
        rows[k].add(k + 1); rows[k + 1].add(k)
    rows[3].add(3)
    rows = [sorted(r) for r in rows]
    rowptr, col = csr_of_rows(rows, DEV)
    row = torch.repeat_interleave(torch.arange(n), torch.tensor([len(r) for r in rows]))
    colc = col.cpu().long()
    gen = torch.Generator().manual_seed(F)
    pw = lambda m: torch.pow(2.0, torch.randint(-2, 3, (m,), generator=gen).float())
    pre, post, val = pw(n), pw(n), pw(colc.numel())
    g = torch.randn(n, F, generator=gen)
    gd, eye = g.to(DEV), torch.eye(F, device=DEV)
    gk = g[row, colc]
    loop = int(torch.nonzero((row == 3) & (colc == 3)))
    cases = [(dict(), torch.ones_like(gk)),
             (dict(pre=pre, post=post, edge_scale=False, self_mode=1), post[row] * pre[colc]),
             (dict(pre=pre, edge_scale=True, self_mode=2), pre[row] * pre[colc]),
             (dict(pre=pre, post=post, val=val, edge_scale=True), post[row] * (val * (pre[row] * pre[colc])))]
    for kw, coef in cases:
        dkw = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}
        out = ops.sddmm_csr(rowptr, col, gd, eye, **dkw)
        want = coef * gk
        if kw.get("self_mode") == 2:
            want[loop] = 0.0
        assert torch.equal(bits(out), bits(want)), (F, sorted(kw))


def test_sddmm_is_fixed_by_its_input(graph):
    """Two runs give the same bits, and the rows of a sub-matrix — the hub row among them, which falls on other run boundaries
    there — get the bits they have in the full matrix."""
    from ocn_amd import ops
    c, F = graph, 128
    g, x = operands(F, 77)
    gd, xd = g.to(DEV), x.to(DEV)
    pick = torch.randperm(N, generator=torch.Generator().manual_seed(9))[:300].tolist()
    pick = [r for r in pick if r not in (HUB, LOOP, 1298)]
    pick = pick[:100] + [HUB] + pick[100:200] + [1298, LOOP] + pick[200:]
    sub_rows = [c.col[int(c.rowptr[r]):int(c.rowptr[r + 1])].tolist() for r in pick]
    rp_s, col_s = csr_of_rows(sub_rows, DEV)
    idx = torch.tensor(pick)
    pos = torch.cat([torch.arange(int(c.rowptr[r]), int(c.rowptr[r + 1])) for r in pick])
    for names, kw in (((), dict()), (("pre", "post", "val"), dict(edge_scale=False)), (("val",), dict(mode="mean"))):
        full = {k: getattr(c.d, k) for k in names}
        first = ops.sddmm_csr(c.d.rowptr, c.d.col, gd, xd, **full, **kw)
        again = ops.sddmm_csr(c.d.rowptr, c.d.col, gd, xd, **full, **kw)
        assert torch.equal(bits(first), bits(again))
        sub = dict(full)
        if "post" in sub:
            sub["post"] = c.post[idx].to(DEV)                             # post is indexed by the operator's own row id
        if "val" in sub:
            sub["val"] = c.val[pos].to(DEV)
        part = ops.sddmm_csr(rp_s, col_s, gd[idx.to(DEV)].contiguous(), xd, **sub, **kw)
        assert part.numel() == pos.numel() > 1100
        assert torch.equal(bits(part), bits(first)[pos]), (names, kw)


@pytest.mark.parametrize("F", [16, 256])
def test_sddmm_row_sums_equal_the_forward(graph, F):
    """sum_p out[p] = <g[r], y[r]> with y the forward ``ops.spmm_csr`` of the same form (self_mode 0), within the rounding of
    both sides: (len_r + 1) roundings per feature of y, F + 2 per entry of out (module docstring): (len_r + F + 3) u mass."""
    from ocn_amd import ops
    c = graph
    g, x = operands(F, 30 + F)
    gd, xd = g.to(DEV), x.to(DEV)
    prod = (g.double()[c.row] * x.double()[c.col]).abs().sum(1)
    for form in ("plain", "pureconv2", "mean", "valued", "valued_mean"):
        names, kw = FORMS[form]
        ops_kw = {k: getattr(c.d, k) for k in names}
        y = ops.spmm_csr(c.d.rowptr, c.d.col, xd, **ops_kw, **kw)
        out = run(c, form, gd, xd)
        got = torch.zeros(N, dtype=torch.double).index_add_(0, c.row, out.cpu().double())
        want = (g.double() * y.cpu().double()).sum(1)
        mass = torch.zeros(N, dtype=torch.double).index_add_(0, c.row, coefficient(c, form).double().abs() * prod)
        bound = (c.lens.double() + F + 3) * U * mass
        err = (got - want).abs()
        busy = bound > 0
        print(f"row sums F={F} {form}: worst error / bound = {(err[busy] / bound[busy]).max().item():.3f}")
        assert bool((err <= bound).all()) and int(busy.sum()) > 1000 and bool(busy[HUB])
        assert float(got[1298]) == 0.0 and float(want[1298]) == 0.0


def test_masked_spmm_under_autograd(graph):
    """``_MaskedSpmmFn``: forward and x gradient bit-equal to ``_SpmmFn``, the mask gradient bit-equal to ``ops.sddmm_csr``; the
    mask is not read; ``max`` raises; ``message_masks`` routes ``_spmm`` and counts its calls."""
    from ocn_amd import ops
    from ocn_amd.model import _MaskedSpmmFn, _SpmmFn, _spmm, message_masks
    from ocn_amd.sparse import SparseTensor
    c, F = graph, 64
    adj = SparseTensor(rowptr=c.d.rowptr, col=c.d.col, value=None, sparse_sizes=(N, N))      # symmetric: its own transpose
    norm = ops.deg_rsqrt(adj._rowptr, 1.0)
    g, x = operands(F, 55)
    gd, xd = g.to(DEV), x.to(DEV)
    calls = [dict(pre=norm, post=norm, mode="sum", edge_scale=False, self_mode=1), dict(pre=norm, mode="sum", edge_scale=True, self_mode=2),
             dict(pre=norm, mode="sum", edge_scale=True), dict(mode="sum"), dict(mode="mean")]
    for kw in calls:
        xa = xd.clone().requires_grad_(True)
        ya = _SpmmFn.apply(xa, adj, kw)
        (gxa,) = torch.autograd.grad(ya, xa, gd)
        xb = xd.clone().requires_grad_(True)
        mask = torch.full((c.nnz,), float("nan"), device=DEV).requires_grad_(True)      # by contract ones; never read
        yb = _MaskedSpmmFn.apply(xb, mask, adj, kw)
        gxb, gm = torch.autograd.grad(yb, (xb, mask), gd)
        assert torch.equal(bits(ya), bits(yb)) and torch.equal(bits(gxa), bits(gxb)), kw
        assert torch.equal(bits(gm), bits(ops.sddmm_csr(adj._rowptr, adj._col, gd, xd, **kw))), kw
        # through the context manager, with an x that requires no grad
        m2 = torch.ones(c.nnz, device=DEV, requires_grad=True)
        with torch.enable_grad(), message_masks(adj, [m2]):
            yc = _spmm(adj, xd, **kw)
        assert yc.requires_grad and torch.equal(bits(yc), bits(ya))
        (gm2,) = torch.autograd.grad(yc, m2, gd)
        assert torch.equal(bits(gm2), bits(gm))
    with pytest.raises(ValueError, match="max"):
        _MaskedSpmmFn.apply(xd, torch.ones(c.nnz, device=DEV, requires_grad=True), adj, dict(mode="max"))
    with pytest.raises(ValueError, match="one entry per stored entry"):
        _MaskedSpmmFn.apply(xd, torch.ones(c.nnz - 1, device=DEV, requires_grad=True), adj, dict(mode="sum"))
    with pytest.raises(RuntimeError, match="2 masks for 1"):
        with message_masks(adj, [m2, m2]):
            _spmm(adj, xd, mode="sum")
    assert message_masks._active is None and not _spmm(adj, xd, mode="sum").requires_grad        # outside: unchanged
