"""Half-precision embedding tables (ocn_cn_gather_h16, ``pipeline.embedding_table``) without a GPU: the symbol and its ABI
entry, the argument checks of the C entry, the kernels' register budget, the rounding of ``embedding_table`` and every Python
refusal of a bf16 / f16 table — each raised on CPU tensors, from the dtype alone, before a device operand is reached."""
import os
import re
import subprocess
from ctypes import c_void_p
from types import SimpleNamespace

import pytest
import torch

from ocn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = [torch.bfloat16, torch.float16]
FP32 = "fp32|float32"                       # every refusal names the requirement


# ---- the C entry ------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_everywhere_and_the_abi_is_still_9(hiplib):
    assert "ocn_cn_gather_h16" in _lib.SIGNATURES and hasattr(hiplib, "ocn_cn_gather_h16")
    hdr = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    m = re.search(r"int ocn_cn_gather_h16\((.*?)\);", hdr, re.S)
    assert m and len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == len(_lib.SIGNATURES["ocn_cn_gather_h16"][1])
    assert len(_lib.SIGNATURES["ocn_cn_gather_h16"][1]) == 23
    history = re.search(r"/\* ABI history.*?\*/", hdr, re.S).group(0)
    later = history[history.index("Later additions to 9"):]
    assert "ocn_cn_gather_h16" in later
    assert "#define OCN_ABI_VERSION 9" in hdr and _lib.ABI_VERSION == 9 and hiplib.ocn_abi_version() == 9
    # the unit builds on lane_group.h by including it
    src = open(os.path.join(ROOT, "ocn_amd", "csrc", "cn_pool_h16.hip")).read()
    assert '#include "lane_group.h"' in src and "OCN_X_" not in src


def test_entry_rejects_bad_arguments_before_any_hip_call(hiplib):
    """Every call but the last is invalid, so none reaches a launch: the pointers are never dereferenced (no GPU here)."""
    P, Z = c_void_p(4096), c_void_p(0)

    def call(**kw):
        a = dict(rowptrA=P, colA=P, src=P, dst=P, order=Z, B=4, off=P, flags=P, wc=Z, weights=P, h16=P, fmt=0, H=64, mrl=10,
                 x1=P, x2=P, x3=P, out_row=Z, cnt1=Z, cnt2=Z, rec=Z, perm=Z)
        a.update(kw)
        return hiplib.ocn_cn_gather_h16(a["rowptrA"], a["colA"], a["src"], a["dst"], a["order"], a["B"], a["off"], a["flags"], a["wc"],
                                        a["weights"], a["h16"], a["fmt"], a["H"], a["mrl"], a["x1"], a["x2"], a["x3"], a["out_row"],
                                        a["cnt1"], a["cnt2"], a["rec"], a["perm"], Z)

    for name in ("rowptrA", "src", "dst", "off", "weights", "h16", "x1", "x2", "x3"):
        assert call(**{name: Z}) == -1, name
        assert call(**{name: Z}, fmt=1) == -1, name
    assert call(B=-1) == -1
    for H in (0, -64, 8, 24, 48, 100, 192, 1024):
        assert call(H=H) == -1 and call(H=H, fmt=1) == -1, H
    for fmt in (-1, 2, 3, 16):
        assert call(fmt=fmt) == -1, fmt
    assert call(B=0, H=7) == -1 and call(B=0, fmt=2) == -1                                  # an empty batch's width and format are still checked
    for H in (16, 32, 64, 128, 256, 512):
        assert call(B=0, H=H) == 0 and call(B=0, H=H, fmt=1) == 0                          # ... and a valid one launches nothing
    # (its tensors have no storage: the pointers of an empty batch are NULL, as for ocn_cn_gather)
    assert call(B=0, src=Z, dst=Z, off=Z, x1=Z, x2=Z, x3=Z) == 0


def test_kernels_do_not_spill(tmp_path):
    """Twelve instances (six widths, two formats) for gfx950, none with scratch, a spilled register or a dynamic stack; the
    rows are loaded in 8- or 16-byte pieces, never element by element."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "cn_pool_h16.s"
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ocn_amd", "csrc"),
                    os.path.join(ROOT, "ocn_amd", "csrc", "cn_pool_h16.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.vgpr_spill_count:\s+(\d+)", text, re.S):
        kernel, body, spills = m.group(1), m.group(2), int(m.group(3))
        if ".private_segment_fixed_size" in body:
            seen[kernel] = (spills, int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1)))
    assert len(seen) == 12 and all("cn_gather_h16_kernel" in k for k in seen), sorted(seen)
    assert all(v == (0, 0) for v in seen.values()), seen
    assert re.findall(r"\.wavefront_size:\s+(\d+)", text) == ["64"] * 12
    assert not re.search(r"global_load_(u?short|sshort|ubyte_d16|short_d16)", text)
    assert "global_load_dwordx2" in text and "global_load_dwordx4" in text


# ---- embedding_table --------------------------------------------------------------------------------------------------------------
def test_embedding_table_rounds_as_torch_does():
    from ocn_amd.pipeline import embedding_table
    g = torch.Generator().manual_seed(0)
    h = torch.randn(37, 16, generator=g) * torch.tensor([1e-6, 1e-3, 1.0, 300.0]).repeat(4)
    h[0, :6] = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 65519.99, 2.0 ** -25])        # (65519.99 still rounds to 65504)
    assert embedding_table(h, "fp32") is h
    for name, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        t = embedding_table(h, name)
        assert t.dtype == dt and t.is_contiguous() and t.device == h.device and t.shape == h.shape
        assert torch.equal(t.view(torch.int16), h.to(dt).view(torch.int16))
        tt = embedding_table(h.t().contiguous().t(), name)                                # a strided h: a contiguous table
        assert tt.is_contiguous() and torch.equal(tt.view(torch.int16), t.view(torch.int16))
    assert h.dtype == torch.float32 and not h.requires_grad


def test_embedding_table_refusals():
    from ocn_amd.pipeline import embedding_table
    h = torch.randn(8, 16)
    big = h.clone()
    big[3, 5] = 65520.0                                      # the first fp32 value that rounds to infinity in f16
    with pytest.raises(ValueError, match="infinity"):
        embedding_table(big, "f16")
    assert torch.isfinite(embedding_table(big, "bf16").float()).all()
    inf = h.clone()
    inf[0, 0] = float("inf")                                 # an infinity that was one already is no overflow
    assert torch.isinf(embedding_table(inf, "f16")[0, 0])
    for bad in ("fp16", "half", "int8", torch.bfloat16, None):
        with pytest.raises(ValueError, match="dtype"):
            embedding_table(h, bad)
    with pytest.raises(ValueError, match="float32"):
        embedding_table(h.double(), "bf16")
    with pytest.raises(ValueError, match="float32"):
        embedding_table(h.bfloat16(), "bf16")
    with pytest.raises(ValueError, match="float32"):
        embedding_table(h[0], "bf16")


# ---- refusals, on CPU tensors -----------------------------------------------------------------------------------------------------
def _tiny():
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.utils import adjoverlap
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(4, 4))
    e = torch.tensor([[0, 2], [2, 0]])
    return adj, e, (adjoverlap(adj, adj, e), adjoverlap(adj, adj, e))


@pytest.mark.parametrize("dt", HALF, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", ["cn5", "cn7", "cn8"])
def test_predictors_refuse_a_half_table_outside_the_eval_path(hiplib, name, dt):
    from ocn_amd.model import predictor_dict
    adj, e, (cn1, cn2) = _tiny()
    args = SimpleNamespace(sum=1.0)
    x = torch.randn(4, 16).to(dt)
    pred = predictor_dict[name](16, 16, 1, 3, 0.0)
    call = (lambda x: pred(x, adj, cn1, cn2, e)) if name == "cn5" else (lambda x: pred.multidomainforward(x, adj, cn1, cn2, e, args))
    pred.train()
    with torch.no_grad(), pytest.raises(TypeError, match=FP32):                   # training mode
        call(x)
    pred.eval()
    with pytest.raises(TypeError, match=FP32):                                    # grad mode
        call(x)
    with torch.no_grad(), pytest.raises(TypeError, match=FP32):                   # a table that asks for a gradient
        call(x.clone().requires_grad_())
    pred.set_edge_sharding(None, True)
    with torch.no_grad(), pytest.raises(TypeError, match=FP32):                   # edge-sharded
        call(x)
    with torch.no_grad(), pytest.raises(TypeError, match=FP32):                   # ... through begin / finish too
        pred.begin(x, adj, cn1, cn2, e, args=args)
    pred.set_edge_sharding(None, False)
    # eval under no_grad is the path that takes it: the call gets as far as the device check (no CPU path), not a TypeError
    with torch.no_grad(), pytest.raises(_lib.OcnHipError, match="no CPU path"):
        call(x)
    with torch.no_grad(), pytest.raises(_lib.OcnHipError, match="no CPU path"):
        pred.begin(x, adj, cn1, cn2, e, args=args)


@pytest.mark.parametrize("dt", HALF, ids=["bf16", "f16"])
def test_cn6_refuses_a_half_table(hiplib, dt):
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import score_edges
    from ocn_amd.recommend import recommend_links
    adj, e, (cn1, cn2) = _tiny()
    x = torch.randn(4, 16).to(dt)
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


@pytest.mark.parametrize("dt", HALF, ids=["bf16", "f16"])
def test_explanations_refuse_a_half_table(hiplib, dt):
    from ocn_amd.explain import explain_link_edges, explain_links
    from ocn_amd.model import predictor_dict
    adj, e, _ = _tiny()
    x = torch.randn(4, 16).to(dt)
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


@pytest.mark.parametrize("dt", HALF, ids=["bf16", "f16"])
def test_embedding_stage_without_an_index_refuses_a_half_table(hiplib, dt):
    from ocn_amd.model import predictor_dict
    from ocn_amd.ranking import rank_links
    from ocn_amd.recommend import EmbeddingNeighbours, ShortListUnion, recommend_links
    adj, e, _ = _tiny()
    x = torch.randn(4, 16).to(dt)
    pred = predictor_dict["cn5"](16, 16, 1, 3, 0.0).eval()
    sources = torch.tensor([0, 1])
    truth = (torch.tensor([0, 1, 2]), torch.tensor([2, 3]))
    for pf in (EmbeddingNeighbours(4), EmbeddingNeighbours(4, normalize=True), ShortListUnion(("ra", 4), EmbeddingNeighbours(4))):
        with pytest.raises(TypeError, match=FP32):
            recommend_links(pred, x, adj, adj, sources, 2, 2, prefilter=pf)
        with pytest.raises(TypeError, match=FP32):
            recommend_links(pred, x, adj, None, sources, 2, 2, prefilter=pf)
        with pytest.raises(TypeError, match=FP32):
            rank_links(pred, x, adj, adj, sources, truth, 2, prefilter=pf)


def test_the_index_keeps_refusing_rows_that_are_not_fp32():
    from ocn_amd.recommend import EmbeddingIndex, EmbeddingNeighbours
    for dt in HALF:
        with pytest.raises(ValueError, match="float32"):
            EmbeddingIndex(torch.randn(4, 16).to(dt))
        with pytest.raises(ValueError, match="float32"):
            EmbeddingNeighbours(4, keys=torch.randn(4, 16).to(dt))


def test_ops_helpers():
    from ocn_amd import ops
    assert ops.HALF_TABLE_FMT == {torch.bfloat16: 0, torch.float16: 1}
    assert ops.is_half_table(torch.zeros(1, dtype=torch.bfloat16)) and ops.is_half_table(torch.zeros(1, dtype=torch.float16))
    assert not ops.is_half_table(torch.zeros(1)) and not ops.is_half_table(None) and not ops.is_half_table(torch.zeros(1).double())
    ops.refuse_half_table(torch.zeros(1), "x")
    with pytest.raises(TypeError, match=FP32):
        ops.refuse_half_table(torch.zeros(1).half(), "x")
    # a half table of another width than the lane-group kernels' is refused by the wrapper, a CPU one by the device check
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.cn_gather(None, None, torch.zeros(1, dtype=torch.int64), None, None, None, None, torch.zeros(4, 4), torch.zeros(4, 16).half())
