"""Refreshing the encoder output after an edge update, on the device (ocn_amd/update.py: ``EncoderState``;
``ocn_spmm_csr_rows``, ``ocn_rows_neighbourhood``, ``ocn_bitlist_count`` / ``_fill``).  The oracle of every case is the full
route on the same device — the rows of ``ops.spmm_csr``, ``model(x, adj_new)``, a freshly built state — or a numpy set
computation.  Everything is bit-exact (``torch.equal``): no tolerance anywhere."""
import itertools

import numpy as np
import pytest
import torch

from tests.helpers import random_graph as _graph, st as _st
from tests.test_graph_update_gpu import _hub_graph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- the row-list SpMM against rows of the full SpMM ------------------------------------------------------------------------
N1 = 200
_spmm_case = {}


def _spmm_graph():
    """N = 200, not symmetric: row 0 is a hub of 150 entries (several rounds at every lanes-per-row setting, 4 .. 64), rows 7
    and 100 are empty, row N - 1 is not; entry values and row scales; 37 random rows (no multiple of the rows per wave: 16,
    8, 4, 2, 1)."""
    if not _spmm_case:
        rng = np.random.default_rng(11)
        a = rng.random((N1, N1)) < 0.03
        a[0] = False
        a[0, rng.choice(N1, size=150, replace=False)] = True
        a[7] = a[100] = False
        a[N1 - 1, [0, 5, N1 - 1]] = True
        r, c = np.nonzero(a)
        adj = _st().from_edge_index(torch.from_numpy(np.stack([r, c]).astype(np.int64)).to(DEV), sparse_sizes=(N1, N1))
        rp = adj._rowptr
        assert int(rp[1] - rp[0]) == 150 and int(rp[8] - rp[7]) == 0 and int(rp[101] - rp[100]) == 0 and int(rp[N1] - rp[N1 - 1]) >= 3
        g = torch.Generator().manual_seed(5)
        lists = [[], [0], [N1 - 1], list(range(N1)), [7], sorted(rng.choice(N1, size=37, replace=False).tolist())]
        _spmm_case.update(adj=adj, val=(torch.rand(adj.nnz(), generator=g) + 0.5).to(DEV), scale=(torch.rand(N1, generator=g) + 0.1).to(DEV),
                          lists=[torch.tensor(l, dtype=torch.int64, device=DEV) for l in lists])
    return _spmm_case


@pytest.mark.parametrize("F", [16, 32, 64, 128, 256, 512])
def test_spmm_csr_rows_equals_rows_of_the_full_product(hiplib, F):
    """Every mode, the four scale forms of the convs (plain; PureConv gcn: pre + post + self after; GCNConv: pre + edge scale +
    self in place; PureConv2 gcn: pre + edge scale), with and without entry values, six row lists."""
    from ocn_amd import ops
    c = _spmm_graph()
    adj, s = c["adj"], c["scale"]
    x = torch.randn(N1, F, generator=torch.Generator().manual_seed(F)).to(DEV)
    x0 = x.clone()
    forms = (dict(), dict(pre=s, post=s, self_mode=1), dict(pre=s, edge_scale=True, self_mode=2), dict(pre=s, edge_scale=True))
    for mode, form, val in itertools.product(("sum", "mean", "max"), forms, (None, c["val"])):
        full = ops.spmm_csr(adj._rowptr, adj._col, x, mode=mode, val=val, **form)
        for rows in c["lists"]:
            got = ops.spmm_csr_rows(adj._rowptr, adj._col, x, rows, mode=mode, val=val, **form)
            assert got.shape == (rows.numel(), F) and got.dtype == torch.float32
            assert torch.equal(got, full[rows]), (mode, sorted(form), val is not None, rows.numel())
    assert torch.equal(x, x0)                                              # the input is only ever read


# ---- neighbourhood lists ----------------------------------------------------------------------------------------------------
def _np_closed(adj, seeds):
    rp, col = adj._rowptr.cpu().numpy(), adj._col.cpu().numpy()
    out = set(int(s) for s in seeds)
    for s in seeds:
        out |= set(col[rp[s]:rp[s + 1]].tolist())
    return sorted(out)


def _device_closed(adj, seeds):
    from ocn_amd import ops
    n = adj.size(0)
    bits = torch.zeros((n + 31) // 32, dtype=torch.int32, device=DEV)
    back = ops.rows_neighbourhood(adj._rowptr, adj._col, torch.tensor(seeds, dtype=torch.int64, device=DEV), bits)
    assert back is bits
    ids = ops.bits_to_list(bits, n)
    assert ids.dtype == torch.int64
    return ids.tolist(), bits


@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_rows_neighbourhood_word_boundaries(hiplib, n):
    rng = np.random.default_rng(200 + n)
    for symmetric in (True, False):
        adj = _graph(n, 0.1, n, symmetric=symmetric)
        for seeds in ([], [n - 1], [0], sorted(set(rng.integers(0, n, size=5).tolist())), list(range(n))):
            got, _ = _device_closed(adj, seeds)
            assert got == _np_closed(adj, seeds)                           # (a sorted list of a set: ascending, duplicate-free)


def test_rows_neighbourhood_hub_graph(hiplib):
    """A hub row of 2500 spans ten 256-element work items; the bits are OR-ed into, never cleared; unsorted seeds with
    duplicates are allowed."""
    from ocn_amd import ops
    n, rng, adj = _hub_graph()
    for seeds in ([], [0], [n - 1], sorted(set(rng.integers(0, n, size=100).tolist()))):
        got, _ = _device_closed(adj, seeds)
        assert got == _np_closed(adj, seeds) and len(set(got)) == len(got)
    assert _device_closed(adj, [n - 1])[0] == [n - 1]                      # the isolated node reaches itself alone
    assert len(_device_closed(adj, [0])[0]) >= 2501
    got, bits = _device_closed(adj, [17, 5, 17, n - 1, 5])
    assert got == _np_closed(adj, [5, 17, n - 1])
    ops.rows_neighbourhood(adj._rowptr, adj._col, torch.tensor([40], dtype=torch.int64, device=DEV), bits)
    assert ops.bits_to_list(bits, n).tolist() == _np_closed(adj, [5, 17, 40, n - 1])


# ---- end to end -------------------------------------------------------------------------------------------------------------
N3, HUB, ISO = 300, 0, 299
_e2e = {}


def _e2e_graph():
    """N = 300, symmetric, average degree about 6, node 0 a hub of 120, node 299 isolated; 32 input features; the updates: five
    edges to insert (isolated -> hub, one the graph has, one self loop), three of them to remove, two more to insert."""
    if not _e2e:
        rng = np.random.default_rng(3)
        a = rng.random((N3, N3)) < 3.0 / N3
        a[HUB, rng.choice(np.arange(1, N3 - 1), size=120, replace=False)] = True
        a = a | a.T
        np.fill_diagonal(a, False)
        a[ISO] = a[:, ISO] = False
        r, c = np.nonzero(a)
        adj = _st().from_edge_index(torch.from_numpy(np.stack([r, c]).astype(np.int64)).to(DEV), sparse_sizes=(N3, N3))
        assert int(adj.storage.rowcount()[HUB]) >= 120 and int(adj.storage.rowcount()[ISO]) == 0
        have = (int(r[len(r) // 2]), int(c[len(r) // 2]))
        ins = torch.tensor([[ISO, 41, have[0], 77, 150], [HUB, 205, have[1], 77, 151]], dtype=torch.int64, device=DEV)
        _e2e.update(adj=adj, ins=ins, rem=ins[:, [0, 2, 4]].contiguous(),
                    ins2=torch.tensor([[10, 250], [260, 11]], dtype=torch.int64, device=DEV),
                    x=torch.randn(N3, 32, generator=torch.Generator().manual_seed(1)).to(DEV),
                    ids=torch.randint(0, 10, (N3,), generator=torch.Generator().manual_seed(2)).to(DEV))
    return _e2e


def _model(cls, conv_fn, layers, hidden=32, **kw):
    from ocn_amd import model as M
    torch.manual_seed(100 * layers + 10 * len(cls) + len(conv_fn))
    m = getattr(M, cls)(32, hidden, hidden, layers, 0.0, conv_fn=conv_fn, **kw).to(DEV).eval()
    with torch.no_grad():
        for mod in m.modules():                                            # (fresh LayerNorms are the identity affine map, fresh biases zero)
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.uniform_(0.5, 1.5); mod.bias.uniform_(-0.5, 0.5)
            if getattr(mod, "bias", None) is not None and isinstance(mod, M.GCNConv):
                mod.bias.uniform_(-0.5, 0.5)
    return m


def _same_state(state, fresh):
    assert torch.equal(state.h, fresh.h)
    assert len(state.xs) == len(fresh.xs) and len(state.zs) == len(fresh.zs)
    for a, b in zip(state.xs, fresh.xs):
        assert torch.equal(a, b)
    for a, b in zip(state.zs, fresh.zs):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))


def _step(state, model, x, adj_new, edges, route, undirected=True):
    """One refresh: ``h`` equals the full pass, every cached layer a fresh state's, the rows returned are R_L, hold every row
    that changed and the device lists agree with ``affected_rows`` on CPU copies."""
    from ocn_amd.update import EncoderState, affected_rows
    old = state.h.clone()
    rows = state.refresh(adj_new, edges, undirected=undirected)
    assert state.route == route
    want = model(x, adj_new)
    assert torch.equal(state.h, want)
    _same_state(state, EncoderState(model, x, adj_new))
    L = len(state.convs)
    cpu_sets = affected_rows(adj_new.cpu(), edges.cpu(), L, state.normalised, undirected=undirected)
    assert len(state.row_sets) == L
    for got, w in zip(state.row_sets, cpu_sets):
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), w)
    assert torch.equal(rows, state.row_sets[-1])
    changed = torch.nonzero((old != want).any(dim=1)).reshape(-1)
    assert torch.isin(changed, rows).all()
    return rows


def _chain(model, x, undirected=True, adj=None, route="rows"):
    """Build, insert, remove, insert again, and the empty update, on one state."""
    from ocn_amd.update import EncoderState, insert_edges, remove_edges
    g = _e2e_graph()
    adj = g["adj"] if adj is None else adj
    state = EncoderState(model, x, adj)
    assert torch.equal(state.h, model(x, adj))
    adj, _ = insert_edges(adj, g["ins"], undirected=undirected)
    rows = _step(state, model, x, adj, g["ins"], route, undirected)
    assert rows.numel() >= 7 and bool((rows[1:] > rows[:-1]).all())
    adj, _ = remove_edges(adj, g["rem"], undirected=undirected)
    _step(state, model, x, adj, g["rem"], route, undirected)
    adj, _ = insert_edges(adj, g["ins2"], undirected=undirected)
    _step(state, model, x, adj, g["ins2"], route, undirected)
    before = state.h.clone()
    none = state.refresh(adj, torch.zeros(2, 0, dtype=torch.int64, device=DEV), undirected=undirected)
    assert none.numel() == 0 and none.dtype == torch.int64 and torch.equal(state.h, before)
    assert all(s.numel() == 0 for s in state.row_sets)
    return state


@pytest.fixture
def every_share(monkeypatch):
    """The graph is small and the updates touch its hub, so the rows of the later layers hold most of its entries: the
    default ``ops.refresh_full_share`` would send those refreshes down the full walk.  These tests are about the row walk:
    with the knob at 1 it is taken whatever the share (the rows can never hold more than every entry)."""
    from ocn_amd import ops
    monkeypatch.setattr(ops, "refresh_full_share", 1.0)


FLAGS = (dict(ln=True), dict(res=True), dict(jk=True), dict(ln=True, res=True, jk=True))
MODELS = [("GCN", "gcn"), ("GCN", "gin"), ("GCN", "sage"), ("GCN", "max"), ("GCN", "puregcn"), ("GCN", "puremean"),
          ("GCN2", "gcn"), ("GCN3", "gin")]


@pytest.mark.parametrize("layers", [1, 2, 3])
@pytest.mark.parametrize("cls,conv_fn", MODELS)
def test_refresh_is_bit_equal_to_the_full_pass(hiplib, every_share, cls, conv_fn, layers):
    g = _e2e_graph()
    with torch.no_grad():
        for flags in FLAGS:
            _chain(_model(cls, conv_fn, layers, **flags), g["x"])


def test_refresh_with_embedding_input(hiplib, every_share):
    g = _e2e_graph()
    with torch.no_grad():
        state = _chain(_model("GCN", "puregcn", 2, max_x=9), g["ids"])
    assert state.normalised and all(z is None for z in state.zs)


def test_refresh_takes_the_row_walk_at_the_default_share(hiplib):
    """One plain layer, edges away from the hub: a handful of rows, far below the default share."""
    from ocn_amd import ops
    from ocn_amd.update import EncoderState, insert_edges
    g = _e2e_graph()
    assert ops.refresh_full_share < 1.0
    with torch.no_grad():
        model = _model("GCN", "gin", 1)
        state = EncoderState(model, g["x"], g["adj"])
        adj, _ = insert_edges(g["adj"], g["ins2"])
        rows = _step(state, model, g["x"], adj, g["ins2"], "rows")
    assert rows.tolist() == [10, 11, 250, 260]


def test_refresh_directed(hiplib, every_share):
    """A non-symmetric adjacency with ``undirected=False``: the rows that read a column are the rows of the transpose."""
    g = _e2e_graph()
    adj = _graph(N3, 0.01, 9, symmetric=False)
    with torch.no_grad():
        for cls, conv_fn in (("GCN", "gcn"), ("GCN3", "gin"), ("GCN", "puregcn")):
            _chain(_model(cls, conv_fn, 2, ln=True, res=True), g["x"], undirected=False, adj=adj)


def test_refresh_falls_back_to_the_full_walk(hiplib, monkeypatch):
    """(a) an op whose bits may depend on the row count — the conv Linear at hidden width 16 is torch's; (b) the share knob."""
    from ocn_amd import ops
    g = _e2e_graph()
    default = ops.refresh_full_share
    with torch.no_grad():
        monkeypatch.setattr(ops, "refresh_full_share", 1.0)
        _chain(_model("GCN", "gcn", 2, hidden=16, ln=True), g["x"], route="full")
        monkeypatch.setattr(ops, "fast_linear", False)
        _chain(_model("GCN", "gin", 2), g["x"], route="full")
        monkeypatch.setattr(ops, "fast_linear", True)
        monkeypatch.setattr(ops, "refresh_full_share", 0.0)
        _chain(_model("GCN", "gin", 2, res=True), g["x"], route="full")
    monkeypatch.undo()
    assert ops.refresh_full_share == default and ops.fast_linear       # the knobs are back


def test_refresh_raises_value_errors_on_misuse(hiplib):
    from ocn_amd.update import EncoderState
    g = _e2e_graph()
    adj, ok = g["adj"], g["ins2"]
    with torch.no_grad():
        model = _model("GCN", "gcn", 2)
        state = EncoderState(model, g["x"], adj)
        h = state.h.clone()
        with pytest.raises(ValueError, match="valued"):
            state.refresh(adj.fill_value(1.0), ok)
        with pytest.raises(ValueError, match="the state holds 300 nodes"):
            state.refresh(_graph(64, 0.1, 1), ok)
        for bad in (torch.tensor([[0], [N3]], device=DEV), torch.tensor([[-1], [0]], device=DEV)):
            with pytest.raises(ValueError, match="out of range"):
                state.refresh(adj, bad)
        for bad in (ok[0], ok.reshape(1, -1), ok.to(torch.int32), ok.to(torch.float32), ok.tolist(), torch.zeros(3, 2, dtype=torch.int64, device=DEV)):
            with pytest.raises(ValueError, match=r"int64 tensor of shape \[2, E\]"):
                state.refresh(adj, bad)
        with pytest.raises(ValueError, match="edges on cpu"):
            state.refresh(adj, ok.cpu())
        model.train()
        with pytest.raises(ValueError, match="eval mode"):
            state.refresh(adj, ok)
        with pytest.raises(ValueError, match="eval mode"):
            EncoderState(model, g["x"], adj)
        model.eval()
        with pytest.raises(ValueError, match="without values"):
            EncoderState(model, g["x"], adj.fill_value(1.0))
        with pytest.raises(ValueError, match="x has 300 rows"):
            EncoderState(model, g["x"], _graph(64, 0.1, 1))
    with pytest.raises(ValueError, match="eval mode"):                     # grad enabled
        state.refresh(adj, ok)
    with pytest.raises(ValueError, match="eval mode"):
        EncoderState(model, g["x"], adj)
    assert torch.equal(state.h, h)                                         # a refused call changes nothing
