"""cn8 (CNLinkPredictorbaselearnablation, model.py:3233-3449) without a GPU: registry, signatures, checkpoint keys, the
argument checks of ``ocn_cn8_pool`` and its kernels' register budget."""
import inspect
import os
import re
import subprocess
from ctypes import c_void_p

import pytest
import torch

from ocn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cn8_is_registered_with_cn7s_constructor_and_calls():
    from ocn_amd.model import CNLinkPredictorbaselearnablation, _CNPredictorBase, predictor_dict
    assert predictor_dict["cn8"] is CNLinkPredictorbaselearnablation and issubclass(predictor_dict["cn8"], _CNPredictorBase)
    c7, c8 = predictor_dict["cn7"], predictor_dict["cn8"]
    assert list(inspect.signature(c8.__init__).parameters) == list(inspect.signature(c7.__init__).parameters)
    assert list(inspect.signature(c8.forward).parameters)[1:] == ["x", "adj", "cn1", "cn2", "tar_ei", "filled1"]
    assert list(inspect.signature(c8.multidomainforward).parameters)[1:] == [
        "x", "adj", "cn1", "cn2", "tar_ei", "args", "filled1", "cndropprobs"]
    assert c8._xcn2_on_union is False


@pytest.mark.parametrize("kw", [dict(), dict(ln=True), dict(tailact=True), dict(twolayerlin=True, ln=True), dict(use_xlin=True)],
                         ids=lambda kw: "+".join(sorted(kw)) or "plain")
def test_cn8_state_dict_keys_equal_cn7s(kw):
    from ocn_amd.model import predictor_dict
    k7 = set(predictor_dict["cn7"](16, 16, 1, 3, 0.1, 0.0, **kw).state_dict())
    p8 = predictor_dict["cn8"](16, 16, 1, 3, 0.1, 0.0, **kw)
    assert set(p8.state_dict()) == k7 and "innerprod" in k7
    assert p8.innerprod.tolist() == [0.0] and p8.n == 0
    p = predictor_dict["cn8"](8, 8, 1, 3, 0.0, beta=0.33)
    assert p.beta.item() == pytest.approx(0.33) and p.alpha.tolist() == [1, 1, 1]


def test_cn8_pool_symbol_is_declared_everywhere(hiplib):
    assert "ocn_cn8_pool" in _lib.SIGNATURES and hasattr(hiplib, "ocn_cn8_pool")
    hdr = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    m = re.search(r"int ocn_cn8_pool\((.*?)\);", hdr, re.S)
    assert m and len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == len(_lib.SIGNATURES["ocn_cn8_pool"][1])
    assert hiplib.ocn_abi_version() == 9


def test_cn8_pool_rejects_bad_arguments_before_any_hip_call(hiplib):
    """Every call here is invalid, so none reaches a launch: the pointers are never dereferenced (no GPU in this test)."""
    P = c_void_p(4096)         # a non-NULL address that is never read
    Z = c_void_p(0)

    def call(**kw):
        a = dict(rowptrA=P, colA=P, rp1=P, c1=P, rp2=P, c2=P, bm1=Z, s1=0, bm2=Z, s2=0, src=P, dst=P, order=Z, B=4, n_cols=64,
                 h=P, H=64, x1=P, x2=P, x3=P, cnt1=P, cnt2=P)
        a.update(kw)
        return hiplib.ocn_cn8_pool(a["rowptrA"], a["colA"], a["rp1"], a["c1"], a["rp2"], a["c2"], a["bm1"], a["s1"], a["bm2"], a["s2"],
                                   a["src"], a["dst"], a["order"], a["B"], a["n_cols"], a["h"], a["H"], a["x1"], a["x2"], a["x3"],
                                   a["cnt1"], a["cnt2"], Z)

    for name in ("rowptrA", "colA", "src", "dst", "h", "x1", "x2", "x3", "cnt1", "cnt2"):
        assert call(**{name: Z}) == -1, name
    assert call(B=-1) == -1
    for H in (0, 8, 48, 100, 1024, -64):
        assert call(H=H) == -1, H
    assert call(rp1=Z, c1=Z) == -1 and call(c1=Z) == -1              # T1: neither CSR nor bit rows
    assert call(rp2=Z, c2=Z) == -1 and call(rp2=Z) == -1              # T2 likewise
    assert call(rp1=Z, c1=Z, rp2=Z, c2=Z) == -1
    assert call(bm1=P, s1=1) == -1 and call(bm2=P, s2=1) == -1        # bit rows shorter than the columns
    assert call(B=0, H=7) == -1                                        # (an empty batch is still checked)
    assert call(B=0) == 0                                              # ... and a valid one launches nothing


def test_cn8_pool_kernels_do_not_spill(tmp_path):
    """The unit of the one-pass kernel compiled for gfx950: six instances (one per width), none with scratch or a spilled
    register, none with a dynamic stack."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "cn8_pool.s"
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ocn_amd", "csrc"),
                    os.path.join(ROOT, "ocn_amd", "csrc", "cn8_pool.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.vgpr_spill_count:\s+(\d+)", text, re.S):
        kernel, body, spills = m.group(1), m.group(2), int(m.group(3))
        if ".private_segment_fixed_size" in body:
            seen[kernel] = (spills, int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1)))
    assert len(seen) == 6 and all("cn8_pool_kernel" in k for k in seen), sorted(seen)
    assert all(v == (0, 0) for v in seen.values()), seen
    assert re.findall(r"\.wavefront_size:\s+(\d+)", text) == ["64"] * 6
    assert "OCN_X_" not in open(os.path.join(ROOT, "ocn_amd", "csrc", "cn8_pool.hip")).read()


def test_cn8_eval_default_is_the_unit_weight_route():
    """The one-pass pooling is opt-in (OCN_CN8_FUSED=1) until a measurement puts its range below the chain's."""
    from ocn_amd import ops
    assert ops.cn8_fused_eval == (os.environ.get("OCN_CN8_FUSED", "0") == "1")
    assert "OCN_CN8_FUSED" in os.environ or ops.cn8_fused_eval is False


@pytest.mark.parametrize("fused", [False, True], ids=["unit_weights", "one_pass"])
def test_cn8_product_path_refuses_cpu_tensors(hiplib, monkeypatch, fused):
    from types import SimpleNamespace
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.utils import adjoverlap, get_cn1_cn2
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(3, 3))
    e = torch.tensor([[0], [1]])
    pred = predictor_dict["cn8"](16, 16, 1, 3, 0.0).eval()
    args = SimpleNamespace(sum=1.0)
    monkeypatch.setattr(ops, "cn8_fused_eval", fused)
    with torch.no_grad(), pytest.raises(_lib.OcnHipError, match="no CPU path"):
        pred(torch.randn(3, 16), adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj, e), e, args)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):           # autograd on: the flag pass refuses as well
        pred(torch.randn(3, 16), adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj, e), e, args)
    with torch.no_grad(), pytest.raises(_lib.OcnHipError, match="no CPU path"):
        pred(torch.randn(3, 16), adj, *get_cn1_cn2(adj, e), e, args)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.cn8_pool(adj._rowptr, adj._col, (adj._rowptr, adj._col), (adj._rowptr, adj._col), e[0], e[1], torch.randn(3, 16))


def test_cn8_pool_wrapper_checks_shapes_before_the_library(monkeypatch):
    """``ops.cn8_pool`` bounds what the kernel indexes: bit rows of T1 and T2 with one row count (``dst`` is checked against
    it), wide enough for the columns, and an ``h`` with one row per column.  The device check is patched out: these are
    host-side shape errors, raised before any library call."""
    from ocn_amd import ops
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    rp, col = torch.tensor([0, 1, 2, 2]), torch.tensor([1, 0], dtype=torch.int32)
    src, dst, h = torch.tensor([0]), torch.tensor([2]), torch.randn(3, 16)
    bm3, bm2 = torch.zeros(3, 1, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="T1 has 3 rows, T2 2"):
        ops.cn8_pool(rp, col, (rp, col), None, src, dst, h, t2_bitmap=bm2)
    with pytest.raises(ValueError, match="T1 has 2 rows, T2 3"):
        ops.cn8_pool(rp, col, None, (rp, col), src, dst, h, t1_bitmap=bm2)
    with pytest.raises(ValueError, match="does not match"):
        ops.cn8_pool(rp, col, (rp, col), (rp, col), src, dst, h, t1_bitmap=bm2)
    with pytest.raises(ValueError, match="does not match"):
        ops.cn8_pool(rp, col, (rp, col), None, src, dst, torch.randn(40, 16), t2_bitmap=bm3)       # 32 bits for 40 columns
    with pytest.raises(ValueError, match="3 rows, the adjacency 5 columns"):
        ops.cn8_pool(rp, col, (rp, col), (rp, col), src, dst, h, n_cols=5)
    with pytest.raises(ValueError, match="needs its CSR arrays or its bit rows"):
        ops.cn8_pool(rp, col, (rp, col), None, src, dst, h)
    with pytest.raises(NotImplementedError):
        ops.cn8_pool(rp, col, (rp, col), (rp, col), src, dst, torch.randn(3, 24))


def test_cn8_handles_must_describe_one_batch():
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.utils import adjoverlap, fuse8, get_cn1_cn2
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(3, 3))
    other = SparseTensor.from_edge_index(torch.tensor([[0, 2], [2, 0]]), sparse_sizes=(3, 3))
    e, e2 = torch.tensor([[0], [1]]), torch.tensor([[1], [2]])
    assert fuse8(*get_cn1_cn2(adj, e), e) is None                       # walk handles take the flag form
    with pytest.raises(NotImplementedError):
        fuse8(adjoverlap(adj, adj, e), adjoverlap(other, adj, e), e)
    with pytest.raises(NotImplementedError):
        fuse8(adjoverlap(adj, adj, e), adjoverlap(adj, adj, e2), e)
    with pytest.raises(ValueError):
        fuse8(adjoverlap(adj, adj, e), adjoverlap(adj, adj, e), torch.tensor([[0, 1], [1, 2]]))
    st = fuse8(adjoverlap(adj, adj, e), adjoverlap(adj, other, e), e)
    assert st.B == 1 and st.N == 3 and st.cnt1 is None and st.cnt2 is None and st.t2 is other
