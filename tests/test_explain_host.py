"""Explaining a link without a GPU: the symbol and the argument checks of ``ocn_cn_attribution``, its kernels' register
budget, the refusals of ``explain_links`` that happen before any device work, and ``LinkExplanation`` as a plain object."""
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


def test_attribution_symbol_is_declared_everywhere(hiplib):
    assert "ocn_cn_attribution" in _lib.SIGNATURES and hasattr(hiplib, "ocn_cn_attribution")
    hdr = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    m = re.search(r"int ocn_cn_attribution\((.*?)\);", hdr, re.S)
    assert m and len(strip(m.group(1)).split(",")) == len(_lib.SIGNATURES["ocn_cn_attribution"][1]) == 17
    history = hdr[:hdr.index("#define OCN_ABI_VERSION")]
    assert "ocn_cn_attribution" in history[history.index("Later additions to 9"):]
    assert "#define OCN_ABI_VERSION 9" in hdr
    assert hiplib.ocn_abi_version() == 9 == _lib.ABI_VERSION


def test_attribution_rejects_bad_arguments_before_any_hip_call(hiplib):
    """Every call but the last is invalid, so none reaches a launch: the pointers are never dereferenced (no GPU in this test)."""
    P = c_void_p(4096)         # a non-NULL, 16-byte aligned address that is never read
    Z = c_void_p(0)
    names = ("rowptrA", "colA", "src", "order", "B", "off", "flags", "wc", "cap", "w", "h", "H", "g1", "g2", "attr", "rank")

    def call(**kw):
        a = dict(rowptrA=P, colA=P, src=P, order=Z, B=4, off=P, flags=P, wc=Z, cap=64, w=P, h=P, H=64, g1=P, g2=P, attr=P, rank=P)
        a.update(kw)
        return hiplib.ocn_cn_attribution(*[a[n] for n in names], Z)

    for name in ("rowptrA", "colA", "src", "off", "flags", "w", "h", "g1", "g2", "attr", "rank"):
        assert call(**{name: Z}) == -1, name
    assert call(B=-1) == -1 and call(cap=-1) == -1
    for H in (0, 8, 48, 100, 1024, -64):
        assert call(H=H) == -1, H
    for name in ("w", "h", "g1", "g2"):                                 # read 16 bytes at a time
        assert call(**{name: c_void_p(4096 + 8)}) == -1, name
        assert call(**{name: c_void_p(4096 + 4)}) == -1, name
    assert call(attr=c_void_p(4096 + 4)) == -1                          # written 8 bytes at a time
    assert call(B=0, H=7) == -1 and call(B=0, w=Z) == -1 and call(B=0, attr=c_void_p(4100)) == -1   # (an empty batch is still checked)
    assert call(B=0) == 0                                               # ... and a valid one launches nothing
    assert call(B=0, order=P, wc=P, cap=0, attr=c_void_p(4096 + 8)) == 0


def test_attribution_kernels_do_not_spill(tmp_path):
    """The unit compiled for gfx950: six instances (one per width), none with scratch or a spilled register, none with LDS."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "cn_attr.s"
    src = os.path.join(ROOT, "ocn_amd", "csrc", "cn_attr.hip")
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ocn_amd", "csrc"), src, "-o", str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.vgpr_spill_count:\s+(\d+)", text, re.S):
        kernel, body, spills = m.group(1), m.group(2), int(m.group(3))
        if ".private_segment_fixed_size" in body:
            seen[kernel] = (spills, int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1)))
    assert len(seen) == 6 and all("cn_attr_kernel" in k for k in seen), sorted(seen)
    assert all(v == (0, 0) for v in seen.values()), seen
    assert re.findall(r"\.wavefront_size:\s+(\d+)", text) == ["64"] * 6
    assert re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text) == ["0"] * 6
    assert "atomic" not in open(src).read().split("#include")[1]        # (the code; the header comment says "no atomics")


def tiny():
    from ocn_amd.sparse import SparseTensor
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(3, 3))
    return adj, torch.tensor([[0, 1]]), torch.randn(3, 16)


def test_explain_links_refuses_before_any_device_work(hiplib):
    from ocn_amd.explain import explain_links
    from ocn_amd.model import predictor_dict
    adj, edges, h = tiny()
    cn5 = predictor_dict["cn5"](16, 16, 1, 3, 0.0).eval()
    with pytest.raises(NotImplementedError, match="cn6"):
        explain_links(predictor_dict["cn6"](16, 16, 1, 3, 0.0).eval(), h, adj, adj, edges)
    with pytest.raises(TypeError):
        explain_links(torch.nn.Linear(2, 2), h, adj, adj, edges)
    with pytest.raises(RuntimeError, match="eval"):
        explain_links(cn5.train(), h, adj, adj, edges)
    cn5.eval()
    cn5.set_edge_sharding(None, True)
    with pytest.raises(RuntimeError, match="sharded"):
        explain_links(cn5, h, adj, adj, edges)
    cn5.set_edge_sharding(None, False)
    top = int(hiplib.ocn_segment_topk_max_k())
    for m in (0, -1, top + 1, 2.0, True, None):
        with pytest.raises(ValueError, match="m must be"):
            explain_links(cn5, h, adj, adj, edges, m=m)
    for rank in ("abs", "", None, 1):
        with pytest.raises(ValueError, match="rank must be"):
            explain_links(cn5, h, adj, adj, edges, rank=rank)
    for bad in (edges[:0], edges.t().contiguous()[:1], edges.to(torch.int32), edges[0], [[0, 1]]):
        with pytest.raises(ValueError, match="edges"):
            explain_links(cn5, h, adj, adj, bad)
    with pytest.raises(ValueError, match="h must be"):
        explain_links(cn5, torch.randn(3, 24), adj, adj, edges)
    with pytest.raises(ValueError, match="args"):
        explain_links(predictor_dict["cn7"](16, 16, 1, 3, 0.0).eval(), h, adj, adj, edges)
    # nothing above changed the predictor, and a valid request on CPU tensors reaches the device layer — on both routes
    assert not cn5.training and cn5._frozen is None and all(p.grad is None for p in cn5.parameters())
    for adj2 in (adj, None):
        with pytest.raises(_lib.OcnHipError, match="no CPU path"):
            explain_links(cn5, h, adj, adj2, edges, m=top)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        explain_links(predictor_dict["cn7"](16, 16, 1, 3, 0.0).eval(), h, adj, adj, edges, args=SimpleNamespace(sum=1.0))


def test_attribution_wrapper_checks_shapes_before_the_library(monkeypatch):
    """``ops.cn_attribution`` bounds what the kernel indexes.  The device check is patched out: these are host-side shape
    errors, raised before any library call."""
    from ocn_amd import ops
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    rp, col = torch.tensor([0, 1, 2, 2]), torch.tensor([1, 0], dtype=torch.int32)
    src, off, flags = torch.tensor([0, 1]), torch.tensor([0, 1, 2]), torch.zeros(2, dtype=torch.uint8)
    h, w, g = torch.randn(3, 16), torch.randn(3, 4), torch.randn(2, 16)
    with pytest.raises(ValueError, match=r"off: \[B \+ 1\]"):
        ops.cn_attribution(rp, col, src, off[:2], flags, None, w, h, g, g)
    with pytest.raises(ValueError, match="wc: one walk count"):
        ops.cn_attribution(rp, col, src, off, flags, torch.zeros(1, dtype=torch.int32), w, h, g, g)
    with pytest.raises(ValueError, match=r"weights must be \[N, 4\]"):
        ops.cn_attribution(rp, col, src, off, flags, None, torch.randn(4, 4), h, g, g)
    with pytest.raises(ValueError, match=r"weights must be \[N, 4\]"):
        ops.cn_attribution(rp, col, src, off, flags, None, torch.randn(3, 3), h, g, g)
    with pytest.raises(ValueError, match=r"g1 must be \[B, H\]"):
        ops.cn_attribution(rp, col, src, off, flags, None, w, h, torch.randn(3, 16), g)
    with pytest.raises(ValueError, match=r"g2 must be \[B, H\]"):
        ops.cn_attribution(rp, col, src, off, flags, None, w, h, g, torch.randn(2, 32))
    with pytest.raises(ValueError, match="order: one entry per candidate"):
        ops.cn_attribution(rp, col, src, off, flags, None, w, h, g, g, order=torch.tensor([0]))
    with pytest.raises(NotImplementedError):
        ops.cn_attribution(rp, col, src, off, flags, None, w, torch.randn(3, 24), torch.randn(2, 24), torch.randn(2, 24))


def test_link_explanation_is_a_plain_dataclass_that_survives_torch_save():
    import dataclasses
    from ocn_amd.explain import LinkExplanation
    B, m = 3, 2
    exp = LinkExplanation(score=torch.randn(B), nodes=torch.tensor([[4, 1], [2, -1], [-1, -1]]), contrib=torch.randn(B, m, 2),
                          kind=torch.tensor([[1, 3], [2, 0], [0, 0]], dtype=torch.uint8), pooled=torch.randn(B, 2),
                          pair=torch.randn(B), cnt1=torch.tensor([2, 0, 0], dtype=torch.int32),
                          cnt2=torch.tensor([1, 1, 0], dtype=torch.int32), drop=torch.full((B, m), float("nan")),
                          flat=(torch.tensor([0, 2, 3, 3]), torch.randn(3, 2), torch.randn(3)))
    assert dataclasses.is_dataclass(exp) and exp._grads is None
    public = [f.name for f in dataclasses.fields(exp) if not f.name.startswith("_")]
    assert public == ["score", "nodes", "contrib", "kind", "pooled", "pair", "cnt1", "cnt2", "drop", "flat"]
    blob = io.BytesIO()
    torch.save(exp, blob)
    blob.seek(0)
    back = torch.load(blob)
    assert isinstance(back, LinkExplanation)
    for name in public[:-2]:
        assert torch.equal(getattr(back, name), getattr(exp, name)), name
    assert torch.equal(back.drop.isnan(), exp.drop.isnan())
    assert all(torch.equal(a, b) for a, b in zip(back.flat, exp.flat))
    bare = LinkExplanation(exp.score, exp.nodes, exp.contrib, exp.kind, exp.pooled, exp.pair, exp.cnt1, exp.cnt2)
    assert bare.drop is None and bare.flat is None
