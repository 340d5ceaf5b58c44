"""GPU: the encoder SpMM (ocn_spmm_csr, ocn_spmm_csr_rows, ocn_deg_rsqrt) bit for bit against the CPU mirror of its documented term
order (tests/spmm_mirror.py; checked on its own in tests/test_spmm_host.py): every width, sum / mean / max, every combination of
self term, row scales, edge scale, post scale and entry values, on a graph whose row lengths sit on every lane-group boundary and
whose rows hold explicit self loops.  Every comparison is ``torch.equal``: a difference is a defect of the kernel or of the
mirror's reading of the contract, never a reason for a tolerance.  Every id handed to a kernel is in range."""
import pytest
import torch

from tests import spmm_mirror as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROWS = [0, 22, 23, 260]                # row 0 (empty as well), the 200-entry row, an empty row, the last row

_cache = {}


def _dev():
    if "dev" not in _cache:
        g = M.fixed_graph()
        _cache["dev"] = {k: g[k].to(DEV) for k in ("rowptr", "col", "pre", "post", "val")}
    return _cache["dev"]


def _mirror(F, mode, i, form):
    """The mirror's product of one form on the fixed graph; kept for the widths the row-list test reads again."""
    key = (F, mode, i)
    if key not in _cache:
        g = M.fixed_graph()
        out = M.spmm(g["rowptr"], g["col"], M.fixed_x(F), mode=mode, **M.form_kwargs(form, g["pre"], g["post"], g["val"]))
        if F not in (16, 512):
            return out
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("F", M.WIDTHS)
def test_kernel_equals_mirror(hiplib, F, mode):
    from ocn_amd import ops
    d = _dev()
    x = M.fixed_x(F)
    xd = x.to(DEV)
    for i, form in enumerate(M.forms()):
        got = ops.spmm_csr(d["rowptr"], d["col"], xd, mode=mode, **M.form_kwargs(form, d["pre"], d["post"], d["val"]))
        want = _mirror(F, mode, i, form)
        bad = (got.cpu() != want).any(1).nonzero().flatten().tolist()
        assert torch.equal(got.cpu(), want), (F, mode, form, "rows", bad[:8], "lengths", [len(M.fixed_graph()["rows"][r]) for r in bad[:8]])
    assert torch.equal(xd.cpu(), x)


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("F", [16, 512])
def test_row_list_entry_equals_mirror_rows(hiplib, F, mode):
    """ocn_spmm_csr_rows against the mirror's rows directly — not against the full product of the same kernel."""
    from ocn_amd import ops
    d = _dev()
    g = M.fixed_graph()
    assert [len(g["rows"][r]) for r in ROWS] == [0, 200, 0, 7]
    x = M.fixed_x(F)
    xd = x.to(DEV)
    rows = torch.tensor(ROWS, device=DEV)
    for i, form in enumerate(M.forms()):
        got = ops.spmm_csr_rows(d["rowptr"], d["col"], xd, rows, mode=mode, **M.form_kwargs(form, d["pre"], d["post"], d["val"]))
        assert got.shape == (len(ROWS), F)
        assert torch.equal(got.cpu(), _mirror(F, mode, i, form)[ROWS]), (F, mode, form)
    assert torch.equal(xd.cpu(), x)


# ---- rectangular operators (self_mode = 0) ----------------------------------------------------------------------------------------
def _rect(n_rows, n_cols):
    lengths = [min(M.LENGTHS[r % len(M.LENGTHS)], n_cols) for r in range(n_rows)]
    rowptr, col = M.csr_from_rows(M.random_rows(n_rows, n_cols, lengths, seed=100 * n_rows + n_cols))
    g = torch.Generator().manual_seed(7 * n_rows + n_cols)
    # pre: one entry per COLUMN, the leading n_cols entries of a 128-entry allocation — no row id of either shape lies outside it
    return dict(rowptr=rowptr, col=col, val=torch.rand(col.numel(), generator=g) + 0.5, pre=(torch.rand(128, generator=g) + 0.1)[:n_cols],
                post=torch.rand(n_rows, generator=g) + 0.1)


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("F", [16, 512])
@pytest.mark.parametrize("shape", [(40, 70), (70, 40)], ids=["40x70", "70x40"])
def test_rectangular_operator_equals_mirror(hiplib, shape, F, mode):
    from ocn_amd import ops
    n_rows, n_cols = shape
    g = _rect(n_rows, n_cols)
    big = torch.zeros(128, device=DEV)
    big[:n_cols] = g["pre"].to(DEV)
    d = dict(rowptr=g["rowptr"].to(DEV), col=g["col"].to(DEV), val=g["val"].to(DEV), pre=big[:n_cols], post=g["post"].to(DEV))
    assert d["pre"].is_contiguous() and d["pre"].numel() == n_cols
    x = M.fixed_x(F, n=n_cols)
    xd = x.to(DEV)
    for names in ((), ("val",), ("pre",), ("pre", "val"), ("pre", "post", "val")):
        got = ops.spmm_csr(d["rowptr"], d["col"], xd, mode=mode, **{k: d[k] for k in names})
        want = M.spmm(g["rowptr"], g["col"], x, mode=mode, **{k: g[k] for k in names})
        assert got.shape == (n_rows, F)
        assert torch.equal(got.cpu(), want), (shape, F, mode, names)
    assert torch.equal(xd.cpu(), x)


def test_edge_scale_on_a_taller_operator_is_refused(hiplib):
    from ocn_amd import ops
    g = _rect(70, 40)
    xd = torch.zeros(40, 16, device=DEV)
    pre = g["pre"].to(DEV).contiguous()
    with pytest.raises(ValueError, match="edge_scale"):
        ops.spmm_csr(g["rowptr"].to(DEV), g["col"].to(DEV), xd, pre=pre, edge_scale=True)
    with pytest.raises(ValueError, match="edge_scale"):
        ops.spmm_csr_rows(g["rowptr"].to(DEV), g["col"].to(DEV), xd, torch.tensor([0, 69], device=DEV), pre=pre, edge_scale=True)


# ---- deg_rsqrt ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("add", [1.0, 0.0])
@pytest.mark.parametrize("valued", [False, True], ids=["unvalued", "valued"])
def test_deg_rsqrt_equals_mirror(hiplib, valued, add):
    from ocn_amd import ops
    d = _dev()
    g = M.fixed_graph()
    got = ops.deg_rsqrt(d["rowptr"], add, val=d["val"] if valued else None)
    want = M.deg_rsqrt(g["rowptr"], add, val=g["val"] if valued else None)
    assert torch.equal(got.cpu(), want), (got.cpu() - want).abs().max()
    assert (want == 0).sum().item() == (12 if add == 0.0 else 0)                   # the d <= 0 branch: the empty rows


# ---- the transposes under autograd -------------------------------------------------------------------------------------------------
def _symmetric():
    if "sym" not in _cache:
        rows = M.fixed_graph()["rows"]
        pairs = {(r, c) for r, cs in enumerate(rows) for c in cs}
        pairs |= {(c, r) for r, c in pairs}
        sym = [[] for _ in rows]
        for r, c in sorted(pairs):
            sym[r].append(c)
        _cache["sym"] = M.csr_from_rows(sym)
    return _cache["sym"]


def _model_calls(norm):
    """The five calls the model makes (model.py: PureConv gcn, GCNConv, PureConv2 gcn, plain sum, plain mean)."""
    return [("PureConv gcn", dict(pre=norm, post=norm, mode="sum", edge_scale=False, self_mode=1)),
            ("GCNConv", dict(pre=norm, mode="sum", edge_scale=True, self_mode=2)),
            ("PureConv2 gcn", dict(pre=norm, mode="sum", edge_scale=True)),
            ("sum", dict(mode="sum")),
            ("mean", dict(mode="mean"))]


@pytest.mark.parametrize("F", [16, 512])
@pytest.mark.parametrize("kind", ["symmetric", "valued"])
def test_forward_and_transpose_under_autograd_equal_mirror(hiplib, kind, F):
    """Forward = the mirror; the gradient of (out * w).sum() = the mirror applied as ``_SpmmFn.backward`` documents: the same form on
    w for a symmetric adjacency, the form over adj.t() for a valued one, for mean the sum form with pre = 1 / count."""
    from ocn_amd import ops
    from ocn_amd.model import _spmm
    from ocn_amd.sparse import SparseTensor
    g = M.fixed_graph()
    n = g["n"]
    if kind == "symmetric":
        rowptr, col = _symmetric()
        val = None
        rp_t, col_t, val_t = rowptr, col, None                                     # its own transpose
    else:
        rowptr, col, val = g["rowptr"], g["col"], g["val"]
        rp_t, col_t, val_t = M.transpose(rowptr, col, val, n)
    adj = SparseTensor(rowptr=rowptr.to(DEV), col=col.to(DEV), value=None if val is None else val.to(DEV), sparse_sizes=(n, n))
    norm_d = ops.deg_rsqrt(adj._rowptr, 1.0, val=adj._value)                       # as the model forms it
    norm = norm_d.cpu()
    assert torch.equal(norm, M.deg_rsqrt(rowptr, 1.0, val=val))
    x = M.fixed_x(F)
    w = torch.randn(n, F, generator=torch.Generator().manual_seed(77 + F))
    inv_cnt = torch.ones(()) / (rowptr[1:] - rowptr[:-1]).clamp(min=1).to(torch.float32)
    for (name, kw_d), (_, kw) in zip(_model_calls(norm_d), _model_calls(norm)):
        want = M.spmm(rowptr, col, x, val=val, **kw)
        if kw["mode"] == "mean":
            want_g = M.spmm(rp_t, col_t, w, pre=inv_cnt, mode="sum", val=val_t)
        else:
            want_g = M.spmm(rp_t, col_t, w, val=val_t, **kw)
        grads = []
        for _ in range(2):
            xd = x.to(DEV).clone().requires_grad_(True)
            out = _spmm(adj, xd, **kw_d)
            assert torch.equal(out.detach().cpu(), want), (kind, F, name, "forward")
            (out * w.to(DEV)).sum().backward()
            grads.append(xd.grad)
        assert torch.equal(grads[0].cpu(), want_g), (kind, F, name, "gradient")
        assert torch.equal(grads[0], grads[1]), (kind, F, name, "two runs")
