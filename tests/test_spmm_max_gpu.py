"""GPU: max aggregation under autograd (ocn_spmm_csr_max_arg / ocn_spmm_max_backward), the valued max forward of
ocn_spmm_csr and the valued-mean backward — hand-derived answers and CPU restatements."""
import pytest
import torch

from tests.helpers import make_graph, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WIDTHS = [16, 32, 64, 128, 256, 512]
NEG_INF = float("-inf")


def _st(r, c, v, n):
    from ocn_amd.sparse import SparseTensor
    return SparseTensor(row=torch.as_tensor(r).to(DEV), col=torch.as_tensor(c).to(DEV),
                        value=None if v is None else torch.as_tensor(v, dtype=torch.float32).to(DEV), sparse_sizes=(n, n))


# ---- hand-derived known answers ----------------------------------------------------------------
# row 0: columns 1, 2, 3, all x = 5            -> a three-way tie: column 1 (the first in row order)
# row 1: columns 0 (value 2), 2 (value 1)       -> 2 * 3 = 6 beats 1 * 5: column 0 (unvalued: 5 at column 2)
# row 2: empty (node 2 is a column elsewhere)   -> y = 0, arg = -1
# row 4: an isolated node                       -> y = 0, arg = -1, no gradient
# row 5: columns 10 .. 79 (70 > 64 entries)     -> 10 at columns 75 and 78: column 75, in the second chunk
# row 6: columns 10 .. 5009 (a hub row)         -> 20 at columns 4000 and 4500: column 4000
N_HAND = 5010


def _hand_graph(valued):
    rows = {0: [(1, 1.0), (2, 1.0), (3, 1.0)], 1: [(0, 2.0), (2, 1.0)], 5: [(k, 1.0) for k in range(10, 80)],
            6: [(k, 1.0) for k in range(10, 5010)]}
    r = [i for i in sorted(rows) for _ in rows[i]]
    c = [k for i in sorted(rows) for k, _ in rows[i]]
    v = [w for i in sorted(rows) for _, w in rows[i]]
    return _st(r, c, v if valued else None, N_HAND)


def _hand_x(F):
    base = torch.zeros(N_HAND)
    base[1:4] = 5.0
    base[0] = 3.0
    k = torch.arange(10, N_HAND)
    base[10:] = -1.0 - (k % 7).float()
    base[75] = base[78] = 10.0
    base[4000] = base[4500] = 20.0
    return base[:, None].repeat(1, F).contiguous()


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("valued", [True, False], ids=["valued", "unvalued"])
def test_max_known_answers(hiplib, F, valued):
    from ocn_amd import ops
    from ocn_amd.model import _spmm
    adj = _hand_graph(valued)
    x = _hand_x(F)
    y, arg = ops.spmm_max_arg(adj._rowptr, adj._col, x.to(DEV), val=adj._value)
    want_arg = torch.full((N_HAND,), -1, dtype=torch.int32)
    want_arg[0], want_arg[1], want_arg[5], want_arg[6] = 1, 0 if valued else 2, 75, 4000
    want_y = torch.zeros(N_HAND)
    want_y[0], want_y[1], want_y[5], want_y[6] = 5.0, 6.0 if valued else 5.0, 10.0, 20.0
    assert torch.equal(arg.cpu(), want_arg[:, None].expand(N_HAND, F))
    assert torch.equal(y.cpu(), want_y[:, None].expand(N_HAND, F))
    assert torch.equal(ops.spmm_csr(adj._rowptr, adj._col, x.to(DEV), mode="max", val=adj._value).cpu(), y.cpu())

    g = torch.randint(-4, 5, (N_HAND, F), generator=torch.Generator().manual_seed(F)).float()
    want_gx = torch.zeros(N_HAND, F)
    want_gx[1] = g[0]
    want_gx[0 if valued else 2] = (2.0 if valued else 1.0) * g[1]
    want_gx[75] = g[5]
    want_gx[4000] = g[6]
    at = adj.t()
    gx = ops.spmm_max_backward(at._rowptr, at._col, arg, g.to(DEV), val=at._value)
    assert torch.equal(gx.cpu(), want_gx)
    if valued:                                            # the same through autograd (a valued adjacency walks adj.t())
        xd = x.to(DEV).requires_grad_(True)
        out = _spmm(adj, xd, mode="max")
        (out * g.to(DEV)).sum().backward()
        assert torch.equal(out.detach().cpu(), y.cpu()) and torch.equal(xd.grad.cpu(), want_gx)


# ---- random inputs against CPU restatements ----------------------------------------------------
def _valued_graph(n=300, seed=4):
    torch.manual_seed(seed)
    dense = (torch.rand(n, n) < 0.04).float() * (1.0 + torch.rand(n, n))      # valued, not symmetric
    dense.fill_diagonal_(0)
    dense[7] = 0                                                              # an empty row
    r, c = dense.nonzero(as_tuple=True)
    return dense, dense != 0, _st(r, c, dense[r, c], n)


def _symmetric_graph(n=400):
    oadj = make_graph(n, 8, 60, 33, isolated=4)
    adj = to_product(oadj, DEV)
    mask = torch.zeros(n, n, dtype=torch.bool)
    mask[oadj.row, oadj.col] = True
    return mask.float(), mask, adj


def _cpu_max(dense, mask, x):
    c = torch.where(mask[:, :, None], dense[:, :, None] * x[None], torch.full((), NEG_INF))
    return torch.where(mask.any(1)[:, None], c.amax(1), torch.zeros(())), c


def _cpu_arg(mask, c):
    return torch.where(mask.any(1)[:, None], c.argmax(1), torch.full((), -1)).to(torch.int32)


@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("kind", ["valued", "symmetric"])
def test_max_arg_forward_matches_plain_max_and_cpu(hiplib, F, kind):
    from ocn_amd import ops
    dense, mask, adj = _valued_graph() if kind == "valued" else _symmetric_graph()
    x = torch.randn(dense.shape[0], F, generator=torch.Generator().manual_seed(F))
    y, arg = ops.spmm_max_arg(adj._rowptr, adj._col, x.to(DEV), val=adj._value)
    plain = ops.spmm_csr(adj._rowptr, adj._col, x.to(DEV), mode="max", val=adj._value)
    assert torch.equal(y, plain)
    ref, c = _cpu_max(dense, mask, x)
    assert torch.equal(y.cpu(), ref)
    assert torch.equal(arg.cpu(), _cpu_arg(mask, c))


@pytest.mark.parametrize("F", [16, 64, 512])
def test_valued_max_forward_takes_the_values(hiplib, F):
    """torch_sparse spmm_max of a valued adjacency (DropAdj in training): max_k fl(v_ik * x_k)."""
    from ocn_amd import ops
    dense, mask, adj = _valued_graph(seed=9)
    x = torch.randn(dense.shape[0], F, generator=torch.Generator().manual_seed(3))
    ref, _ = _cpu_max(dense, mask, x)
    assert torch.equal(ops.spmm_csr(adj._rowptr, adj._col, x.to(DEV), mode="max", val=adj._value).cpu(), ref)


@pytest.mark.parametrize("kind", ["valued", "symmetric"])
@pytest.mark.parametrize("F", [32, 128])
def test_max_backward_matches_cpu_autograd(hiplib, kind, F):
    from ocn_amd.model import _spmm
    dense, mask, adj = _valued_graph() if kind == "valued" else _symmetric_graph()
    n = dense.shape[0]
    x = torch.randn(n, F, generator=torch.Generator().manual_seed(5))
    xr = x.clone().requires_grad_(True)
    ref, _ = _cpu_max(dense, mask, xr)
    w = torch.randn(n, F, generator=torch.Generator().manual_seed(1))
    (ref * w).sum().backward()
    grads = []
    for _ in range(2):
        xd = x.to(DEV).requires_grad_(True)
        out = _spmm(adj, xd, mode="max")
        assert torch.equal(out.detach().cpu(), ref.detach())
        (out * w.to(DEV)).sum().backward()
        grads.append(xd.grad)
    assert (grads[0].cpu() - xr.grad).abs().max().item() <= 2e-5
    assert torch.equal(grads[0], grads[1])                        # fixed summation order: bit-equal runs


@pytest.mark.parametrize("F", [32, 256])
def test_valued_mean_forward_and_backward_match_cpu_autograd(hiplib, F):
    from ocn_amd.model import _spmm
    dense, mask, adj = _valued_graph(seed=6)
    n = dense.shape[0]
    x = torch.randn(n, F, generator=torch.Generator().manual_seed(2))
    xr = x.clone().requires_grad_(True)
    cnt = mask.sum(1).clamp(min=1).float()
    ref = (dense @ xr) / cnt[:, None]
    w = torch.randn(n, F, generator=torch.Generator().manual_seed(1))
    (ref * w).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    out = _spmm(adj, xd, mode="mean")
    assert torch.allclose(out.detach().cpu(), ref.detach(), atol=2e-5, rtol=2e-5)
    (out * w.to(DEV)).sum().backward()
    assert torch.allclose(xd.grad.cpu(), xr.grad, atol=2e-5, rtol=2e-5), (xd.grad.cpu() - xr.grad).abs().max()


def test_max_under_autograd_refuses_row_scales(hiplib):
    from ocn_amd import ops
    from ocn_amd.model import _spmm
    _, _, adj = _symmetric_graph()
    xd = torch.randn(400, 32, device=DEV, requires_grad=True)
    nd = ops.deg_rsqrt(adj._rowptr, 1.0)
    with pytest.raises(ValueError):
        _spmm(adj, xd, mode="max", pre=nd)
    out = _spmm(adj, xd, mode="mean", post=nd)                    # the forward exists; its backward is not this operator's
    with pytest.raises(ValueError):
        out.sum().backward()


def test_max_entries_check_operand_rows(hiplib):
    from ocn_amd import ops
    _, _, adj = _symmetric_graph()
    x = torch.randn(400, 32, device=DEV)
    with pytest.raises(ValueError):
        ops.spmm_max_arg(adj._rowptr, adj._col, x[:399].contiguous(), n_cols=400)
    _, arg = ops.spmm_max_arg(adj._rowptr, adj._col, x, n_cols=400)
    with pytest.raises(ValueError):
        ops.spmm_max_backward(adj._rowptr, adj._col, arg[:399].contiguous(), x[:399].contiguous(), n_cols=400)
    with pytest.raises(ValueError):
        ops.spmm_max_backward(adj._rowptr, adj._col, arg, x[:, :16].contiguous(), n_cols=400)
