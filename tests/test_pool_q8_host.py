"""Int8 embedding tables (ocn_cn_gather_q8, ``ops.Int8Table``, ``pipeline.embedding_table_int8``) without a GPU: the symbol and its
ABI entry, the argument checks of the C entry, the kernels' register budget, the quantisation bound of the table, the storage it
shares with an ``EmbeddingIndex`` and every Python refusal — each raised on CPU tensors, from the type alone, before a device
operand is reached."""
import io
import os
import re
import subprocess
from ctypes import c_void_p
from types import SimpleNamespace

import pytest
import torch

from ocn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32 = "fp32|float32"                       # every refusal names the requirement
WIDTHS = (16, 32, 64, 128, 256, 512)


# ---- the C entry ------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_everywhere_and_the_abi_is_still_9(hiplib):
    assert "ocn_cn_gather_q8" in _lib.SIGNATURES and hasattr(hiplib, "ocn_cn_gather_q8")
    hdr = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    m = re.search(r"int ocn_cn_gather_q8\((.*?)\);", hdr, re.S)
    assert m and len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == len(_lib.SIGNATURES["ocn_cn_gather_q8"][1])
    # ocn_cn_gather_h16's 23, (h16, fmt) -> (q8, row_stride, scale), then ocn_cn_gather_cap's (cap, seed, mult)
    assert len(_lib.SIGNATURES["ocn_cn_gather_q8"][1]) == 23 + 1 + 3
    history = re.search(r"/\* ABI history.*?\*/", hdr, re.S).group(0)
    later = history[history.index("Later additions to 9"):]
    assert "ocn_cn_gather_q8" in later
    assert "#define OCN_ABI_VERSION 9" in hdr and _lib.ABI_VERSION == 9 and hiplib.ocn_abi_version() == 9
    src = open(os.path.join(ROOT, "ocn_amd", "csrc", "cn_pool_q8.hip")).read()
    assert '#include "lane_group.h"' in src and "OCN_X_" not in src
    assert "atomic" not in src.split('#include "lane_group.h"')[1] and "__shared__" not in src


def test_entry_rejects_bad_arguments_before_any_hip_call(hiplib):
    """Every call but the empty batches is invalid, so none reaches a launch: the pointers are never dereferenced (no GPU here)."""
    P, Z = c_void_p(4096), c_void_p(0)

    def call(**kw):
        a = dict(rowptrA=P, colA=P, src=P, dst=P, order=Z, B=4, off=P, flags=P, wc=Z, weights=P, q8=P, stride=64, scale=P, H=64,
                 mrl=10, x1=P, x2=P, x3=P, out_row=Z, cnt1=Z, cnt2=Z, rec=Z, perm=Z, cap=0, seed=0, mult=Z)
        a.update(kw)
        return hiplib.ocn_cn_gather_q8(a["rowptrA"], a["colA"], a["src"], a["dst"], a["order"], a["B"], a["off"], a["flags"], a["wc"],
                                       a["weights"], a["q8"], a["stride"], a["scale"], a["H"], a["mrl"], a["x1"], a["x2"], a["x3"],
                                       a["out_row"], a["cnt1"], a["cnt2"], a["rec"], a["perm"], a["cap"], a["seed"], a["mult"], Z)

    for name in ("rowptrA", "colA", "src", "dst", "off", "flags", "weights", "q8", "scale", "x1", "x2", "x3"):
        assert call(**{name: Z}) == -1, name
        assert call(**{name: Z}, cap=3, mult=P) == -1, name
    assert call(B=-1) == -1 and call(B=-1, cap=2) == -1
    for H in (0, -64, 8, 24, 48, 100, 192, 1024):
        assert call(H=H, stride=1024) == -1 and call(H=H, stride=1024, cap=1) == -1, H
    for cap in (-1, -(1 << 31)):
        assert call(cap=cap) == -1 and call(cap=cap, mult=P) == -1, cap
    assert call(cap=0, mult=P) == -1                                                        # multipliers without a sample
    for stride in (0, -64, 16, 48, 63, 65, 72, 100):                                        # shorter than a row, or no multiple of 16
        assert call(stride=stride) == -1 and call(stride=stride, cap=4) == -1, stride
    assert call(H=16, stride=8) == -1 and call(H=512, stride=256) == -1
    # an empty batch's width, stride, cap and mult are still checked ...
    assert call(B=0, H=7) == -1 and call(B=0, stride=40) == -1 and call(B=0, cap=-1) == -1 and call(B=0, mult=P) == -1
    for H in WIDTHS:                                                                        # ... and a valid one launches nothing
        stride = max(H, 64)
        assert call(B=0, H=H, stride=stride) == 0 and call(B=0, H=H, stride=stride, cap=5, mult=P) == 0
        assert call(B=0, H=H, stride=H) == 0 and call(B=0, H=H, stride=stride + 16) == 0
    # (its tensors have no storage: the pointers of an empty batch are NULL, as for ocn_cn_gather)
    assert call(B=0, src=Z, dst=Z, off=Z, x1=Z, x2=Z, x3=Z) == 0


def test_kernels_do_not_spill(tmp_path):
    """Twelve instances (six widths, capped and uncapped) for gfx950, none with scratch, a spilled register or a dynamic stack;
    a lane's piece of a row is one dword (one dwordx2 at H = 512) load, never byte by byte."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "cn_pool_q8.s"
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ocn_amd", "csrc"),
                    os.path.join(ROOT, "ocn_amd", "csrc", "cn_pool_q8.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.vgpr_spill_count:\s+(\d+)", text, re.S):
        kernel, body, spills = m.group(1), m.group(2), int(m.group(3))
        if ".private_segment_fixed_size" in body:
            seen[kernel] = (spills, int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1)),
                            int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1)))
    assert len(seen) == 12 and all("cn_gather_q8_kernel" in k for k in seen), sorted(seen)
    assert sum("Lb1E" in k for k in seen) == 6 and sum("Lb0E" in k for k in seen) == 6          # capped / uncapped
    assert all(v == (0, 0, 0) for v in seen.values()), seen
    assert re.findall(r"\.wavefront_size:\s+(\d+)", text) == ["64"] * 12
    assert not re.search(r"global_load_sbyte|global_load_(u?short|sshort|short_d16)|global_load_[us]byte_d16", text)
    assert "global_load_dwordx2" in text and re.search(r"global_load_dword\s", text)
    assert not re.search(r"ds_(read|write)|global_atomic|flat_atomic", text.replace("ds_bpermute", ""))


# ---- the table --------------------------------------------------------------------------------------------------------------------
def _h():
    g = torch.Generator().manual_seed(0)
    h = torch.randn(37, 16, generator=g) * torch.tensor([1e-6, 1e-3, 1.0, 300.0]).repeat(4)
    h[5] = 0.0                                                                             # an all-zero row
    h[6] = torch.randn(16, generator=g) * 1e-30
    h[7] = torch.randn(16, generator=g) * 1e30
    return h


def test_int8_table_is_the_quantisation_of_its_rows(hiplib):
    from ocn_amd import ops, pipeline
    h = _h()
    t = pipeline.embedding_table_int8(h)
    assert isinstance(t, ops.Int8Table) and pipeline.Int8Table is ops.Int8Table
    q, s = ops.quantize_rows_i8(h)
    assert torch.equal(t.rows, q) and torch.equal(t.scale, s) and t.width == 16
    assert t.rows.dtype == torch.int8 and t.rows.shape == (37, 64) and t.scale.dtype == torch.float32 and t.scale.shape == (37,)
    assert t.shape == (37, 16) and t.dtype == torch.int8 and t.device == h.device and not t.is_cuda and t.dim() == 2
    assert t.contiguous() is t and not t.requires_grad
    d = t.float()
    assert d.dtype == torch.float32 and d.shape == h.shape
    assert torch.equal(d, q[:, :16].float() * s[:, None])
    # the fp32 division and product roundings at |x / scale| <= 127
    assert bool(((h - d).abs() <= s[:, None] * (0.5 + 2.0 ** -14)).all())
    assert float(s[5]) == 1.0 and not bool(q[5].any())
    assert int(q.abs().max()) == 127 and not bool(q[:, 16:].any())
    ids = torch.tensor([7, 0, 36, 7])
    assert torch.equal(t.float_rows(ids), d[ids])
    tt = pipeline.embedding_table_int8(h.t().contiguous().t())                            # a strided h: the same table
    assert torch.equal(tt.rows, q) and torch.equal(tt.scale, s)
    for bad in (float("inf"), float("-inf"), float("nan")):
        x = h.clone()
        x[3, 2] = bad
        with pytest.raises(ValueError, match="finite"):
            pipeline.embedding_table_int8(x)
    for bad in (h.double(), h.bfloat16(), h[0], None):
        with pytest.raises(ValueError, match="float32"):
            pipeline.embedding_table_int8(bad)


def test_int8_table_is_a_plain_object(hiplib):
    from ocn_amd import ops, pipeline
    t = pipeline.embedding_table_int8(_h())
    f = io.BytesIO()
    torch.save(t, f)
    f.seek(0)
    back = torch.load(f, weights_only=True)
    assert isinstance(back, ops.Int8Table) and torch.equal(back.rows, t.rows) and torch.equal(back.scale, t.scale) and back.width == 16
    moved = t.to("cpu")
    assert isinstance(moved, ops.Int8Table) and torch.equal(moved.float(), t.float())
    for rows, scale, width in ((t.rows.float(), t.scale, 16), (t.rows, t.scale.double(), 16), (t.rows, t.scale[:-1], 16),
                               (t.rows, t.scale, 0), (t.rows, t.scale, 65), (t.rows, t.scale, True), (t.rows[:, ::2], t.scale, 16),
                               (t.rows[0], t.scale, 16)):
        with pytest.raises(ValueError):
            ops.Int8Table(rows, scale, width)


def test_table_and_index_share_storage(hiplib):
    from ocn_amd import ops, pipeline
    from ocn_amd.recommend import EmbeddingIndex
    h = _h()
    t = pipeline.embedding_table_int8(h)
    ix = EmbeddingIndex.from_table(t)
    assert ix.keys_q.data_ptr() == t.rows.data_ptr() and ix.kscale.data_ptr() == t.scale.data_ptr()
    assert (ix.n, ix.width, ix.normalize) == (37, 16, False)
    made = EmbeddingIndex(h)
    assert torch.equal(made.keys_q, ix.keys_q) and torch.equal(made.kscale, ix.kscale)
    back = ops.Int8Table.from_index(made)
    assert back.rows.data_ptr() == made.keys_q.data_ptr() and back.scale.data_ptr() == made.kscale.data_ptr()
    assert back.shape == (37, 16) and torch.equal(back.float(), t.float())
    with pytest.raises(ValueError, match="normalize"):
        ops.Int8Table.from_index(EmbeddingIndex(h, normalize=True))
    with pytest.raises(ValueError, match="Int8Table"):
        EmbeddingIndex.from_table(h)


# ---- refusals, on CPU tensors -----------------------------------------------------------------------------------------------------
def _tiny():
    from ocn_amd.pipeline import embedding_table_int8
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.utils import adjoverlap
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(4, 4))
    e = torch.tensor([[0, 2], [2, 0]])
    return adj, e, (adjoverlap(adj, adj, e), adjoverlap(adj, adj, e)), embedding_table_int8(torch.randn(4, 16))


@pytest.mark.parametrize("cap", [None, 3], ids=["exact", "capped"])
@pytest.mark.parametrize("name", ["cn5", "cn7", "cn8"])
def test_predictors_refuse_an_int8_table_outside_the_eval_path(hiplib, name, cap):
    from ocn_amd.model import predictor_dict
    adj, e, (cn1, cn2), x = _tiny()
    args = SimpleNamespace(sum=1.0)
    pred = predictor_dict[name](16, 16, 1, 3, 0.0)
    call = (lambda x: pred(x, adj, cn1, cn2, e)) if name == "cn5" else (lambda x: pred.multidomainforward(x, adj, cn1, cn2, e, args))
    pred.train()
    with torch.no_grad(), pytest.raises(TypeError, match=FP32):                   # training mode
        call(x)
    pred.eval()
    with pytest.raises(TypeError, match=FP32):                                    # grad mode
        call(x)
    pred.set_edge_sharding(None, True)
    with torch.no_grad(), pytest.raises(TypeError, match=FP32):                   # edge-sharded
        call(x)
    with torch.no_grad(), pytest.raises(TypeError, match=FP32):                   # ... through begin / finish too
        pred.begin(x, adj, cn1, cn2, e, args=args)
    pred.set_edge_sharding(None, False)
    # eval under no_grad is the path that takes it, capped or not: the call gets as far as the device check (no CPU path)
    pred.set_cn_cap(cap)
    with torch.no_grad(), pytest.raises(_lib.OcnHipError, match="no CPU path"):
        call(x)
    with torch.no_grad(), pytest.raises(_lib.OcnHipError, match="no CPU path"):
        pred.begin(x, adj, cn1, cn2, e, args=args)


def test_cn6_refuses_an_int8_table(hiplib):
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import score_edges
    from ocn_amd.recommend import recommend_links
    adj, e, (cn1, cn2), x = _tiny()
    pred = predictor_dict["cn6"](16, 16, 1, 3, 0.0).eval()
    with torch.no_grad(), pytest.raises(TypeError, match=FP32):
        pred(x, adj, cn1, cn2, cn1, e)
    with pytest.raises(TypeError, match=FP32):
        score_edges(pred, x, adj, adj, e.t().contiguous(), 2)
    with pytest.raises(TypeError, match=FP32):
        score_edges(pred, x, adj, adj, e.t().contiguous()[:0], 2)               # ... an empty request too
    with pytest.raises(TypeError, match=FP32):
        recommend_links(pred, x, adj, adj, torch.tensor([0, 1]), 2, 2)
    w = torch.zeros(4, 4)
    with pytest.raises(TypeError, match=FP32):
        ops.cn_gather3(adj._rowptr, adj._col, e[0], e[1], torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.uint8),
                       torch.zeros(2, dtype=torch.uint8), w, w, torch.zeros(1), x)


def test_explanations_refuse_an_int8_table(hiplib):
    from ocn_amd.explain import explain_link_edges, explain_links
    from ocn_amd.model import predictor_dict
    adj, e, _, x = _tiny()
    edges = e.t().contiguous()
    for name in ("cn5", "cn8"):
        pred = predictor_dict[name](16, 16, 1, 3, 0.0).eval()
        with pytest.raises(TypeError, match=FP32):
            explain_links(pred, x, adj, adj, edges, m=2)
        with pytest.raises(TypeError, match=FP32):
            explain_links(pred, x, adj, None, edges, m=2)
        encoder = SimpleNamespace(training=False, convs=[SimpleNamespace(aggr="sum")])
        with pytest.raises(TypeError, match=FP32):
            explain_link_edges(encoder, pred, x, adj, adj, edges, 0, top=2)


def test_a_cosine_stage_without_an_index_refuses_an_int8_table(hiplib):
    from ocn_amd.model import predictor_dict
    from ocn_amd.ranking import rank_links
    from ocn_amd.recommend import EmbeddingNeighbours, ShortListUnion, recommend_links
    adj, e, _, x = _tiny()
    pred = predictor_dict["cn5"](16, 16, 1, 3, 0.0).eval()
    sources = torch.tensor([0, 1])
    truth = (torch.tensor([0, 1, 2]), torch.tensor([2, 3]))
    for pf in (EmbeddingNeighbours(4, normalize=True), ShortListUnion(("ra", 4), EmbeddingNeighbours(4, normalize=True))):
        with pytest.raises(TypeError, match=FP32):
            recommend_links(pred, x, adj, adj, sources, 2, 2, prefilter=pf)
        with pytest.raises(TypeError, match=FP32):
            recommend_links(pred, x, adj, None, sources, 2, 2, prefilter=pf)
        with pytest.raises(TypeError, match=FP32):
            rank_links(pred, x, adj, adj, sources, truth, 2, prefilter=pf)
    # normalize=False takes the table itself as its index: no TypeError, the request gets as far as the device check
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        recommend_links(pred, x, adj, adj, sources, 2, 2, prefilter=EmbeddingNeighbours(4))


def test_ops_helpers(hiplib):
    from ocn_amd import ops
    from ocn_amd.pipeline import embedding_table_int8
    t = embedding_table_int8(torch.randn(4, 16))
    assert not ops.is_half_table(t) and ops.is_compact_table(t)
    assert ops.is_compact_table(torch.zeros(1).half()) and ops.is_compact_table(torch.zeros(1).bfloat16())
    assert not ops.is_compact_table(torch.zeros(1)) and not ops.is_compact_table(None) and not ops.is_compact_table(torch.zeros(1, dtype=torch.int8))
    assert ops.HALF_TABLE_FMT == {torch.bfloat16: 0, torch.float16: 1}
    ops.refuse_half_table(t, "x")                                                           # (keeps its meaning: half tables only)
    ops.refuse_compact_table(torch.zeros(1), "x")
    with pytest.raises(TypeError, match=FP32):
        ops.refuse_compact_table(t, "x")
    with pytest.raises(TypeError, match=FP32):
        ops.refuse_compact_table(torch.zeros(1).half(), "x")
    # a CPU table is stopped by the device check of either wrapper, an unsupported width by the wrapper itself
    one = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.cn_gather(None, None, one, None, None, None, None, torch.zeros(4, 4), t)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.cn_gather_cap(None, None, one, None, None, None, None, torch.zeros(4, 4), t, 3)
    with pytest.raises(ValueError, match="cap"):
        ops.cn_gather_cap(None, None, one, None, None, None, None, torch.zeros(4, 4), t, 0)
