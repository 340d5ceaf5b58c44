"""The fused heads (ocn_heads_fused, csrc/heads.hip) held against references the kernel does not share code with.

The kernel's selection logic — which tiles run a branch, which rows count as zero rows, which constant a skipped branch adds —
is written once per form, and the two forms are otherwise only compared with each other.  Here:

1. every class boundary, both xcn2 forms (cn5: on the union, cn7: cn2 only), both kernel forms: the ranged kernel on rows whose
   missing inputs are NaN against the unranged kernel on rows whose missing inputs are zero, bit for bit; the unranged side is
   anchored to fp64;
2. the one-layer xijlin fold (tailact), panel scales far from their default exponents, a weight maximum that is a power of two:
   against fp64;
3. two and three rounds of the persistent grid with class ranges and a row map: against fp64, and bit for bit against the
   unranged kernel;
4. the C entry itself: ldx > H, destination rows, constants mode;
5. cn7 and tailact end to end at the fused widths against the oracle.

The accuracy bar is the project's (test_parity_gpu.py::test_heads_product_accuracy): the kernel's error against fp64 may be
1.5 x that of torch's own fp32 evaluation of the same modules.  Worst observed max-error ratio e_got / e_32 on an MI355X:

    (H, ln)          test 1   test 2   test 3
    (128, True)      0.703    0.655    0.787
    (128, False)     0.749    0.693    0.869
    (256, True)      0.698    0.877    0.674
    (256, False)     0.755    0.668    0.691

(test 2: the worst of its three variants, 0.877 is the one-layer xijlin; test 3: the worst of the two batch sizes.)  Test 5, worst
over its cases: err 3.8e-7 at a noise of 4.9e-7 .. 6.5e-7, against a bar of about 2e-5.
"""
import copy
import ctypes
from functools import partial
from types import SimpleNamespace

import pytest
import torch

from oracle import ocn_oracle as O
from ocn_amd import _lib
from tests.helpers import batch, make_graph, product_adj2, to_product

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FORMS = (0, 1 << 40)                        # ops.heads_small_batch bound: 128 candidates per workgroup | 32
WIDTHS = pytest.mark.parametrize("H,ln", [(128, True), (128, False), (256, True), (256, False)])


# ---- shared pieces ------------------------------------------------------------------------------------------------------------
def make_pred(H, ln, tailact=False, seed=0, edit=None):
    """The drivers' head with trained-looking weights (the recipe of test_heads_product_accuracy); ``edit(pred)`` changes
    parameters in place before anything is derived from them."""
    from ocn_amd.model import predictor_dict
    torch.manual_seed(seed)
    pred = partial(predictor_dict["cn5"], cndeg=-1)(H, H, 1, 3, 0.0, 0.0, ln, tailact=tailact).to(DEV).eval()
    with torch.no_grad():
        for p in pred.parameters():
            p.mul_(1.0 + 0.5 * torch.rand_like(p))
        if edit is not None:
            edit(pred)
    return pred


def pack_of(pred, H):
    from ocn_amd import ops
    pack = pred._fused_pack(H, DEV)
    scratch = ops.buf(pred._ws, "heads_scratch", int(_lib.lib().ocn_heads_scratch_bytes(H)) // 4, torch.float32, DEV)
    return pack, scratch


class Reference:
    """The plain torch modules: lin(s(a0) xcn1lin(x1) + s(a0) s(a1) xcn2lin(x2) + beta xijlin(xij)) in fp64 on a deep copy of the
    predictor, and in fp32 on the predictor itself.  Taken AFTER the parameters were edited."""

    def __init__(self, pred):
        self.p32, self.p64 = pred, copy.deepcopy(pred).double()

    def __call__(self, x1, x2, xij):
        with torch.no_grad():
            a = torch.sigmoid(self.p64.alpha).cumprod(-1)

            def head(m, dt):
                z = a.to(dt)[0] * m.xcn1lin(x1.to(dt)) + a.to(dt)[1] * m.xcn2lin(x2.to(dt)) + m.beta.to(dt) * m.xijlin(xij.to(dt))
                return m.lin(z)
            return head(self.p64, torch.float64), head(self.p32, torch.float32).double()


def accuracy_bar(got, ref64, ref32, what):
    """max |got - ref64| <= 1.5 max |ref32 - ref64| + 1e-7 max |ref64|,  rms(got - ref64) <= 1.5 rms(ref32 - ref64) + 1e-8;
    returns the max-error ratio e_got / e_32."""
    got = got.double()
    assert got.shape == ref64.shape and torch.isfinite(got).all(), what
    e_got, e_32 = (got - ref64).abs(), (ref32 - ref64).abs()
    mg, m32 = e_got.max().item(), e_32.max().item()
    rg, r32 = e_got.pow(2).mean().sqrt().item(), e_32.pow(2).mean().sqrt().item()
    ratio = mg / m32 if m32 > 0 else (0.0 if mg == 0 else float("inf"))
    print(f"heads-bar {what}: max {mg:.3e} / {m32:.3e} = {ratio:.3f}, rms {rg:.3e} / {r32:.3e}")
    assert mg <= 1.5 * m32 + 1e-7 * ref64.abs().max().item(), f"{what}: e_got / e_32 = {ratio:.3f} (max {mg:.3e} against {m32:.3e})"
    assert rg <= 1.5 * r32 + 1e-8, f"{what}: e_got / e_32 = {ratio:.3f} (rms {rg:.3e} against {r32:.3e})"
    return ratio


def ranges_of(m3, m32, m321, B):
    """ocn_class_order's table for class-major rows both | cn1 only | cn2 only | none with boundaries m3 <= m32 <= m321."""
    return torch.tensor([[0, m32], [0, m3], [m32, m321], [0, m321], [m321, B], [m3, m32], [0, B]], dtype=torch.int64)


def has1(slot, m):
    """Does the row at ``slot`` have a pooled xcn1 (``m`` = (m3, m32, m321); ``slot``: an int or a tensor of slots)."""
    return slot < m[1]


def has2(slot, on_union, m):
    """... a pooled xcn2: cn5 pools it on cn1 u cn2, cn7 on cn2 alone (the cn1-only class [m3, m32) has none)."""
    m3, m32, m321 = m
    return slot < m321 if on_union else (slot < m3) | ((slot >= m32) & (slot < m321))


def mixed_inputs(B, H, seed):
    """Rows of very different magnitude inside one wave's 32, columns of very different magnitude inside one row."""
    torch.manual_seed(seed)
    x1, x2, xij = (torch.randn(B, H, device=DEV) for _ in range(3))
    x1[::3] *= 1e-3
    x2[:, ::5] *= 1e3
    return x1, x2, xij


def masked(x1, x2, m, on_union, fill):
    """x1 / x2 with the rows that have no pooled input (has1 / has2 false) set to ``fill``: 0 is what such a row counts as,
    NaN stands for the stale row the pooling never wrote."""
    slot = torch.arange(x1.shape[0], device=x1.device)
    f = torch.full_like(x1, fill)
    return torch.where(has1(slot, m)[:, None], x1, f), torch.where(has2(slot, on_union, m)[:, None], x2, f)


def tile_has(has, rows):
    """Per slot: does ANY slot of its ``rows``-row tile have the input — the tiles that run the branch; the others take its constant."""
    B, n = has.numel(), (has.numel() + rows - 1) // rows
    padded = torch.zeros(n * rows, dtype=torch.bool, device=has.device)
    padded[:B] = has
    return padded.view(n, rows).any(1).repeat_interleave(rows)[:B]


def same(a, b):
    """torch.equal without the host round trip: a 0-d bool on the device."""
    return (a == b).all() if a.shape == b.shape else torch.zeros((), dtype=torch.bool, device=a.device)


# ---- 1. class boundaries against the unranged kernel, bit for bit -----------------------------------------------------------------
BOUNDS = (0, 1, 31, 32, 33, 64, 127, 128, 129, 256, 257, 384, 388, 389)      # around the 32- and 128-row tiles of B = 389
TRIPLES = [(a, b, c) for a in BOUNDS for b in BOUNDS for c in BOUNDS if a <= b <= c]
ANCHORS = [(0, 0, 0), (389, 389, 389), (33, 129, 257), (0, 128, 128), (128, 128, 256), (1, 1, 389)]


@WIDTHS
def test_class_boundaries_change_no_bit(hiplib, H, ln):
    """The kernel's contract (heads.hip): skipping changes no bit of any score, and rows without a pooled input count as zero
    rows.  For EVERY triple of boundaries around the tile edges, both xcn2 forms and both kernel forms: the ranged kernel with
    a row map, fed NaN where the ranges declare no input, returns what the unranged kernel returns on zeros there.  A predicate
    that hands a row with input the constant, or reads a row the ranges declare empty (the NaN passes the first ReLU as 0 where
    a zero row gives ReLU(bias)), fails the equality.  On six named triples the unranged side is held against fp64.

    Equal bits cannot tell a tile that ran a branch on zero rows from one that took the constant: WHICH tiles take it is pinned
    by handing the kernel a wrong constant for one branch at a time — exactly the rows of the tiles without any row that has
    the branch's input must change, at the form's own tile height."""
    from ocn_amd import ops
    B = 389                                                                     # 3 * 128 + 5 = 12 * 32 + 5
    assert len(TRIPLES) == 560 and all(t in TRIPLES for t in ANCHORS)
    pred = make_pred(H, ln, seed=100 + H + int(ln))
    ref = Reference(pred)
    pack, scratch = pack_of(pred, H)
    half = pack["cpark"].numel() // 2                                           # the park layout: branch a's share | branch b's
    wrong = []
    for br in (0, 1):
        c = pack["cpark"].clone()
        c[br * half:(br + 1) * half] = c[br * half:(br + 1) * half] * -2.0 + 0.5
        wrong.append(dict(pack, cpark=c))
    x1, x2, xij = mixed_inputs(B, H, 7)
    rowmap = torch.randperm(B, device=DEV)
    slot = torch.arange(B, device=DEV)
    tables = torch.stack([ranges_of(*m, B) for m in TRIPLES]).to(DEV)
    worst = 0.0
    prev = ops.heads_small_batch()
    try:
        with torch.no_grad():
            for k, m in enumerate(TRIPLES):
                ok, anchored = [], []
                for on_union in (True, False):
                    x1z, x2z = masked(x1, x2, m, on_union, 0.0)
                    x1n, x2n = masked(x1, x2, m, on_union, float("nan"))
                    for bound in FORMS:
                        ops.heads_small_batch(bound)
                        y0 = ops.heads_fused(x1z, x2z, xij, pack, None, None, on_union, scratch)
                        y1 = ops.heads_fused(x1n, x2n, xij, pack, tables[k], rowmap, on_union, scratch)
                        ok += [same(y1[rowmap], y0), torch.isfinite(y1).all()]
                        for br, has in ((0, has1(slot, m)), (1, has2(slot, on_union, m))):
                            yw = ops.heads_fused(x1n, x2n, xij, wrong[br], tables[k], None, on_union, scratch)
                            ok.append(same((yw != y0).view(-1), ~tile_has(has, 128 if bound == 0 else 32)))
                        if m in ANCHORS:
                            anchored.append((on_union, bound, y0, x1z, x2z))
                ok = torch.stack(ok).cpu().tolist()                             # the one synchronisation of this triple
                assert all(ok), f"m3, m32, m321 = {m}: [equal, finite, constant a, constant b] x (on_union, form) = {ok}"
                for on_union, bound, y0, x1z, x2z in anchored:
                    worst = max(worst, accuracy_bar(y0, *ref(x1z, x2z, xij), f"boundaries H={H} ln={ln} {m} on_union={on_union} form={bound}"))
    finally:
        ops.heads_small_batch(prev)
    print(f"heads-worst test1 H={H} ln={ln} {worst:.3f}")


# ---- 2. one-layer xijlin, panel scales, a power-of-two weight maximum: against fp64 -------------------------------------------------
def _edit_scaled(pred):
    pred.xcn1lin[0].weight.mul_(2.0 ** 12)
    pred.xcn2lin[3].weight.mul_(2.0 ** -12)


def _edit_pow2(pred):
    w = pred.xcn1lin[3].weight
    w.clamp_(-1.0, 1.0)
    w[5, 9] = 2.0


@WIDTHS
@pytest.mark.parametrize("variant", ["tailact", "scaled", "pow2"])
def test_xijlin_fold_and_panel_scales_against_fp64(hiplib, H, ln, variant):
    """tailact: xijlin is ONE layer, so the folded output matrix is Mc = beta * W0l (``_make_fused_pack``) — otherwise only ever
    compared fused against fused.  scaled: xcn1lin.0 times 2^12 and xcn2lin.3 times 2^-12 move two panel scales of
    ``ops.heads_panel`` twelve exponents away from where the initialisation leaves them.  pow2: a weight whose largest element
    is exactly 2.0, the edge of heads_panel's frexp."""
    from ocn_amd import ops
    B = 257
    pred = make_pred(H, ln, tailact=variant == "tailact", seed=200 + H + int(ln),
                     edit={"tailact": None, "scaled": _edit_scaled, "pow2": _edit_pow2}[variant])
    if variant == "tailact":
        assert len(pred._fused_plan(H)[2]) == 1
    else:
        assert len(pred._fused_plan(H)[2]) == 2
    if variant == "scaled":
        plain = make_pred(H, ln, seed=200 + H + int(ln))                        # the same weights before the edit
        for lin, e in ((lambda p: p.xcn1lin[0], 12), (lambda p: p.xcn2lin[3], -12)):
            assert ops.heads_panel(lin(pred).weight)[1] == ops.heads_panel(lin(plain).weight)[1] * 2.0 ** e
    if variant == "pow2":
        w = pred.xcn1lin[3].weight
        assert w.abs().max().item() == 2.0 and (w.abs() == 2.0).sum().item() == 1
        assert ops.heads_panel(w)[1] == 2.0 ** -12                              # 2.0 * 2^12 = 2^13, the lower edge of [2^13, 2^14)
    ref = Reference(pred)                                                       # (carries the edited weights)
    pack, scratch = pack_of(pred, H)
    x1, x2, xij = mixed_inputs(B, H, 11)
    ref64, ref32 = ref(x1, x2, xij)
    worst = 0.0
    prev = ops.heads_small_batch()
    try:
        for bound in FORMS:
            ops.heads_small_batch(bound)
            with torch.no_grad():
                got = ops.heads_fused(x1, x2, xij, pack, None, None, True, scratch)
            worst = max(worst, accuracy_bar(got, ref64, ref32, f"{variant} H={H} ln={ln} form={bound}"))
    finally:
        ops.heads_small_batch(prev)
    print(f"heads-worst test2 H={H} ln={ln} {worst:.3f} ({variant})")


# ---- 3. more than one round of the persistent grid: against fp64 -------------------------------------------------------------------
# The throughput form runs at most 256 workgroups; a batch of more than 256 * 128 rows takes further rounds, in snake order.
# (B, boundaries): all four classes present, every boundary inside a 128-row tile.  65 537 rows = 513 tiles: two full rounds and a
# one-tile third; 32 769 = 257 tiles: the second round holds one tile and runs in reverse order.
ROUNDS = [(65537, (20001, 33003, 50007)), (32769, (10001, 16503, 25007))]


@WIDTHS
@pytest.mark.parametrize("B,m", ROUNDS, ids=["B65537", "B32769"])
def test_persistent_rounds_against_fp64(hiplib, H, ln, B, m):
    """Snake order, the early break on a partial last round, the prefetch that reads this tile's rows once more when nothing
    follows, the park slots indexed by workgroup: the whole batch against fp64, and bit for bit against the same inputs
    without ranges or row map (the round structure alone) — also with NaN in the rows the ranges declare empty."""
    from ocn_amd import ops
    assert all(0 < b < B and b % 128 for b in m) and m[0] < m[1] < m[2] and (B + 127) // 128 > 256
    pred = make_pred(H, ln, seed=300 + H + int(ln))
    ref = Reference(pred)
    pack, scratch = pack_of(pred, H)
    x1, x2, xij = mixed_inputs(B, H, 13)
    rowmap = torch.randperm(B, device=DEV)
    r = ranges_of(*m, B).to(DEV)
    worst = 0.0
    prev = ops.heads_small_batch()
    try:
        ops.heads_small_batch(0)                                                # the 128-row form, whatever the batch
        for on_union in (True, False):
            with torch.no_grad():
                x1z, x2z = masked(x1, x2, m, on_union, 0.0)
                x1n, x2n = masked(x1, x2, m, on_union, float("nan"))
                y0 = ops.heads_fused(x1z, x2z, xij, pack, None, None, on_union, scratch)
                yr = ops.heads_fused(x1z, x2z, xij, pack, r, rowmap, on_union, scratch)
                yn = ops.heads_fused(x1n, x2n, xij, pack, r, rowmap, on_union, scratch)
                del x1n, x2n
                ref64, ref32 = ref(x1z, x2z, xij)
            worst = max(worst, accuracy_bar(yr[rowmap], ref64, ref32, f"rounds H={H} ln={ln} B={B} on_union={on_union}"))
            assert torch.equal(yr[rowmap], y0), (on_union, (yr[rowmap] - y0).abs().max().item())
            assert torch.isfinite(yn).all() and torch.equal(yn, yr), on_union
            del ref64, ref32, y0, yr, yn, x1z, x2z
    finally:
        ops.heads_small_batch(prev)
    print(f"heads-worst test3 H={H} ln={ln} {worst:.3f} (B={B})")


# ---- 4. the C entry directly -------------------------------------------------------------------------------------------------------
def c_call(pack, H, B, xs, ldx, scratch, y=None, dump=None, ranges=None, rowmap=None, on_union=True):
    """ocn_heads_fused on an OcnHeadsArgs filled the way ops.heads_fused fills it; ``xs``: three tensors whose data pointer is
    row 0, ``ldx`` their row stride in floats."""
    a = _lib.OcnHeadsArgs()
    for i in range(3):
        a.x[i] = xs[i].data_ptr()
        a.p_first[i] = pack["first"][i].data_ptr()
        a.p_out[i] = pack["out"][i].data_ptr()
    a.p_mid[0], a.p_mid[1] = pack["mid"][0].data_ptr(), pack["mid"][1].data_ptr()
    a.ldx, a.B, a.H = ldx, B, H
    a.vec = pack["vec"].data_ptr()
    a.ranges = None if ranges is None else ranges.data_ptr()
    a.y_row_map = None if rowmap is None else rowmap.data_ptr()
    a.y = None if y is None else y.data_ptr()
    a.dump = None if dump is None else dump.data_ptr()
    a.cpark = None if dump is not None else pack["cpark"].data_ptr()
    a.scratch = scratch.data_ptr()
    a.eps, a.ln, a.b_on_union = float(pack["eps"]), int(pack["ln"]), int(on_union)
    _lib.check(_lib.lib().ocn_heads_fused(ctypes.byref(a), _lib.stream_ptr()), "ocn_heads_fused")


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("H", [128, 256])
def test_c_entry_strides_destination_rows_and_constants(hiplib, H):
    from ocn_amd import ops
    B, GUARD, SENT = 161, 64, 0x7FC0BEEF                                        # (the sentinel: a NaN with a payload)
    pred = make_pred(H, True, seed=400 + H)
    pack, scratch = pack_of(pred, H)
    x = mixed_inputs(B, H, 17)
    m = (33, 97, 129)
    r, rowmap = ranges_of(*m, B).to(DEV), torch.randperm(B, device=DEV)
    x1z, x2z = masked(x[0], x[1], m, True, 0.0)
    nconst = int(_lib.lib().ocn_heads_const_bytes(H)) // 4
    prev = ops.heads_small_batch()
    try:
        for bound in FORMS:
            ops.heads_small_batch(bound)
            with torch.no_grad():
                want = ops.heads_fused(*x, pack, None, None, True, scratch)
                want_map = ops.heads_fused(x1z, x2z, x[2], pack, r, rowmap, True, scratch)
            # (a) the inputs are the left halves of [B, 2H] buffers whose right halves are NaN: ldx = 2H
            wide = [torch.full((B, 2 * H), float("nan"), device=DEV) for _ in range(3)]
            for wbuf, src in zip(wide, x):
                wbuf[:, :H] = src
            y = torch.full((B, 1), float("nan"), device=DEV)
            c_call(pack, H, B, wide, 2 * H, scratch, y=y)
            assert torch.equal(bits(y), bits(want)), (bound, "ldx = 2H")
            # (b) destination rows: a permutation of 0 .. B - 1 into a buffer with 64 guard floats behind it
            ybuf = torch.full((B + GUARD,), SENT, dtype=torch.int32, device=DEV)
            c_call(pack, H, B, [x1z, x2z, x[2]], H, scratch, y=ybuf, ranges=r, rowmap=rowmap)
            assert (ybuf[B:] == SENT).all(), (bound, "wrote past the batch")
            assert torch.equal(ybuf[:B], bits(want_map).view(-1)), (bound, "row map")
            assert not (ybuf[:B] == SENT).any()
            # (c) constants mode: one zero row in, the skipped branches' shares out; twice the same bits, and those of the pack
            z = torch.zeros(1, H, device=DEV)
            dumps = [torch.full((nconst,), f, device=DEV) for f in (float("nan"), 12345.0)]
            for d in dumps:
                c_call(pack, H, 1, [z, z, z], H, scratch, dump=d)
            assert torch.isfinite(dumps[0]).all()
            assert torch.equal(bits(dumps[0]), bits(dumps[1])) and torch.equal(bits(dumps[0]), bits(pack["cpark"])), bound
    finally:
        ops.heads_small_batch(prev)


# ---- 5. cn7 and tailact end to end at the fused widths -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph(hiplib):
    """The graph and batch of test_parity_gpu.py::test_fused_heads_every_width (graph seed 43, batch seed 19: all four classes
    are present — 871 both, 1 cn1 only, 461 cn2 only, 978 none), with the oracle's cn matrices."""
    n, B = 3000, 2311
    oadj = make_graph(n, 5, 60, 43, isolated=20)
    adj = to_product(oadj, DEV)
    adj2 = product_adj2(adj)
    e = batch(oadj, B, 19)
    c1, c2 = O.adjoverlap(oadj, oadj, e), O.adjoverlap(oadj, O.adj2_sparse(oadj), e)
    k1, k2 = torch.bincount(c1.row, minlength=B) > 0, torch.bincount(c2.row, minlength=B) > 0
    cls = k1.long() * 2 + k2.long()
    assert all((cls == c).sum().item() > 0 for c in range(4)), [(cls == c).sum().item() for c in range(4)]
    return SimpleNamespace(n=n, B=B, adj=adj, adj2=adj2, e=e, c1=c1, c2=c2)


@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("name,tailact", [("cn7", False), ("cn7", True), ("cn5", True)])
def test_cn7_and_tailact_end_to_end(graph, monkeypatch, name, tailact, H):
    """The predictor as the drivers call it, on class-major rows (ranges, row map, pooling that leaves the rows without entries
    unwritten) and in batch order: the same bits; against the oracle as test_configs_gpu.py compares a head without LayerNorm —
    as close to the fp64 evaluation of the heads on the oracle's fp32 pooled vectors as the oracle's own fp32 arithmetic is."""
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    from ocn_amd.utils import adjoverlap
    g, ln, sum_fill = graph, True, 2.74
    torch.manual_seed(5)
    x = torch.randn(g.n, H)
    pred = partial(predictor_dict[name], cndeg=-1)(H, H, 1, 3, 0.0, 0.0, ln, tailact=tailact).eval()
    if name == "cn5":
        with torch.no_grad():
            pred.innerprod.fill_(0.5)
    sd = {k: v.detach().clone() for k, v in pred.state_dict().items()}
    if name == "cn7":
        ref = O.cn7_forward(sd, x, g.c1, g.c2, g.e, sum_fill, ln, tailact)
        pool = O.cn7_pool(x, g.c1, g.c2, sum_fill)[:2]
    else:
        ref = O.cn5_forward(sd, x, g.c1, g.c2, g.e, ln, tailact)
        pool = O.cn5_pool(x, g.c1, g.c2, sd["innerprod"])[:2]
    ref64 = O._heads({k: v.double() for k, v in sd.items()}, x.double(), pool[0].double(), pool[1].double(), g.e, ln, tailact, False)

    pred, xd, ed = pred.to(DEV), x.to(DEV), g.e.to(DEV)
    assert pred._fused_plan(H) is not None and (len(pred._fused_plan(H)[2]) == 1) == tailact
    ordered, ranged = [], []
    real_order, real_heads = ops.class_order, ops.heads_fused
    monkeypatch.setattr(ops, "class_order", lambda *a, **k: (ordered.append(1), real_order(*a, **k))[1])

    def heads_fused(*a, **k):
        if k.get("dump") is None:                                               # (constants mode builds the pack: not a scoring call)
            ranged.append(a[4] is not None and a[5] is not None)
        return real_heads(*a, **k)
    monkeypatch.setattr(ops, "heads_fused", heads_fused)
    monkeypatch.setattr(ops, "skip_zero_min_batch", 0)                          # (the batch is smaller than the product's bound)
    args = SimpleNamespace(sum=sum_fill)
    outs = []
    was = ops.skip_zero_rows
    try:
        for skip in (False, True):
            ops.skip_zero_rows = skip
            with torch.no_grad():
                outs.append(pred(xd, g.adj, adjoverlap(g.adj, g.adj, ed), adjoverlap(g.adj, g.adj2, ed), ed, args))
            assert len(ordered) == (1 if skip else 0), "class-major order " + ("not taken" if skip else "taken without skipping")
            assert ranged == ([False, True] if skip else [False]), "the fused head did not run, or not with ranges and a row map"
    finally:
        ops.skip_zero_rows = was
    assert outs[0].shape == (g.B, 1) and torch.equal(outs[0], outs[1])
    noise = (ref.double() - ref64).abs().max().item()
    for out in outs:
        err = (out.cpu().double() - ref64).abs().max().item()
        print(f"heads-e2e {name} tailact={tailact} H={H}: err {err:.3e} noise {noise:.3e}")
        assert err <= 1e-5 + 1e-5 * ref.abs().max().item() + 2 * noise, (err, noise)
