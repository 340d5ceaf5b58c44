"""GPU: every encoder whose aggregation is max or mean trains — GCN / GCN2 / GCN3 with puremax, max, sage, puremean,
GCN under DropAdj — against a CPU torch restatement of the encoder, and the example driver on the Citeseer shape."""
import importlib.util
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import close, make_graph, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONVS = ["puremax", "max", "sage", "puremean"]
MODE = {"puremax": "max", "max": "max", "sage": "mean", "puremean": "mean"}


def _dense(adj, n):
    """(values, pattern) of a product SparseTensor as dense CPU matrices (unvalued: values 1)."""
    r, c, v = adj.coo()
    r, c = r.cpu(), c.cpu()
    A = torch.zeros(n, n)
    A[r, c] = 1.0 if v is None else v.cpu().float()
    M = torch.zeros(n, n, dtype=torch.bool)
    M[r, c] = True
    return A, M


def _aggr(A, M, x, mode):
    """torch_sparse spmm_mean / spmm_max of a (valued) adjacency: Σ_k v_ik x_k / count_i, max_k v_ik x_k (empty row: 0)."""
    if mode == "mean":
        return (A @ x) / M.sum(1).clamp(min=1).float()[:, None]
    c = torch.where(M[:, :, None], A[:, :, None] * x[None], torch.full((), float("-inf")))
    return torch.where(M.any(1)[:, None], c.amax(1), torch.zeros(()))


def _encoder_cpu(cls, conv, sd, x, adjs, L):
    """GCN / GCN2 / GCN3 with ln, res and jk on, dropouts 0 (model.py:232-511)."""
    pure, mode = "pure" in conv, MODE[conv]
    if "xemb.1.weight" in sd:
        x = F.linear(x, sd["xemb.1.weight"], sd["xemb.1.bias"])
    jkx = []
    for i in range(L):
        A, M = adjs[i]
        if cls == "GCN" and not pure:                                 # GCNConv(aggr, normalize=False): lin, aggregate, + bias
            y = _aggr(A, M, F.linear(x, sd[f"convs.{i}.lin.weight"]), mode) + sd[f"convs.{i}.bias"]
        else:
            y = _aggr(A, M, x, mode)
            if not pure:                                              # PureConv2/3 use_lin: Linear(no bias) + ReLU
                y = torch.relu(F.linear(y, sd[f"convs.{i}.lin.0.weight"]))
        if not pure and (i == 0 or i < L - 1):
            w = sd[f"lins.{i}.0.weight"]
            y = torch.relu(F.layer_norm(y, (w.numel(),), w, sd[f"lins.{i}.0.bias"], 1e-5))
        x = y + x if y.shape[-1] == x.shape[-1] else y
        jkx.append(x)
    return torch.sum(torch.stack(jkx, 0) * sd["jkparams"].reshape(-1, 1, 1), dim=0)


def _check_grads(enc, sd, xd, xr):
    assert (xd.grad.cpu() - xr.grad).abs().max().item() <= 3e-5 * max(1.0, xr.grad.abs().max().item())
    for k, p in enc.named_parameters():
        g = sd[k].grad
        assert g is not None and p.grad is not None, k
        assert (p.grad.cpu() - g).abs().max().item() <= 3e-5 * max(1.0, g.abs().max().item()), k


@pytest.mark.parametrize("conv", CONVS)
@pytest.mark.parametrize("cls", ["GCN", "GCN2", "GCN3"])
def test_encoder_backward_matches_cpu_autograd(hiplib, cls, conv):
    import ocn_amd.model as M
    n, H, L = 300, 32, 2
    oadj = make_graph(n, 8, 60, 33, isolated=4)
    adj = to_product(oadj, DEV)
    torch.manual_seed(8)
    enc = getattr(M, cls)(H, H, H, L, 0.0, True, True, -1, conv, True).eval()
    sd = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in enc.state_dict().items()}
    x = torch.randn(n, H)
    xr = x.clone().requires_grad_(True)
    ref = _encoder_cpu(cls, conv, sd, xr, [_dense(adj, n)] * L, L)
    wgt = torch.randn(n, H, generator=torch.Generator().manual_seed(2))
    (ref * wgt).sum().backward()
    enc = enc.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    out = enc(xd, adj)
    assert close(out, ref, atol=2e-5, rtol=2e-5), (out.detach().cpu() - ref).abs().max()
    (out * wgt.to(DEV)).sum().backward()
    _check_grads(enc, sd, xd, xr)


@pytest.mark.parametrize("conv", CONVS)
def test_gcn_trains_through_dropadj(hiplib, conv):
    """Train mode, edrop = 0.3: every layer draws its own valued adjacency (surviving entries × 1/(1-p)); the CPU
    restatement runs on exactly the adjacencies DropAdj returned, and the same seed gives the same bits."""
    import ocn_amd.model as M
    n, H, L = 300, 32, 2
    oadj = make_graph(n, 8, 60, 35, isolated=4)
    adj = to_product(oadj, DEV)
    torch.manual_seed(8)
    enc = M.GCN(H, H, H, L, 0.0, True, True, -1, conv, True, 0.3).to(DEV).train()
    x = torch.randn(n, H)
    wgt = torch.randn(n, H, generator=torch.Generator().manual_seed(2))

    def run():
        enc.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        seen = []
        hook = enc.adjdrop.register_forward_hook(lambda m, i, o: seen.append(o))
        xd = x.to(DEV).requires_grad_(True)
        out = enc(xd, adj)
        hook.remove()
        (out * wgt.to(DEV)).sum().backward()
        return out.detach(), xd, {k: p.grad.clone() for k, p in enc.named_parameters()}, seen

    out, xd, grads, seen = run()
    assert len(seen) == L
    full = adj.coo()[1].numel()
    for a in seen:                                                # DropAdj handed the layers valued, thinned adjacencies
        assert a._value is not None and 0 < a.coo()[1].numel() < full
    sd = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in enc.state_dict().items()}
    xr = x.clone().requires_grad_(True)
    ref = _encoder_cpu("GCN", conv, sd, xr, [_dense(a, n) for a in seen], L)
    (ref * wgt).sum().backward()
    assert close(out, ref, atol=2e-5, rtol=2e-5), (out.cpu() - ref).abs().max()
    _check_grads(enc, sd, xd, xr)

    out2, xd2, grads2, _ = run()
    assert torch.equal(out2, out) and torch.equal(xd2.grad, xd.grad)
    assert all(torch.equal(grads2[k], grads[k]) for k in grads)


# ---- the example driver with the reference README's Citeseer encoder settings --------------------
CITESEER = ["--dataset", "citeseer", "--mplayers", "3", "--nnlayers", "1", "--hiddim", "64", "--gnnedp", "0.07", "--res",
            "--maskinput", "--batch_size", "384", "--epochs", "3"]


def _driver():
    spec = importlib.util.spec_from_file_location("run_like_reference", os.path.join(ROOT, "examples", "run_like_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("predictor,model", [("cn5", "puremean"), ("cn7", "puremean"), ("cn5", "puremax")])
def test_example_driver_trains_citeseer_through_dropadj(hiplib, predictor, model):
    out = _driver().main(CITESEER + ["--predictor", predictor, "--model", model])
    losses = [o[0] for o in out]
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    for hits in out[-1][1].values():
        assert all(0.0 <= v <= 1.0 for v in hits)
