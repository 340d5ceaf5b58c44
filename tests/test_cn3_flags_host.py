"""cn6 without a stored A³ (``ocn_cn3_flags``, ``utils.adjoverlap_3hop``) without a GPU: the entry is declared everywhere, its
unit compiles alone, its argument checks come before any HIP call, and the Python layer refuses what it cannot serve."""
import os
import re
import subprocess
from ctypes import c_void_p

import pytest
import torch

from ocn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _graphs():
    from ocn_amd.sparse import SparseTensor
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    adj = SparseTensor.from_edge_index(ei, sparse_sizes=(3, 3))
    adj2 = SparseTensor.from_edge_index(torch.tensor([[0, 0, 1, 2, 2], [0, 2, 1, 0, 2]]), sparse_sizes=(3, 3))
    return adj, adj2


def test_cn3_flags_symbol_is_declared_everywhere(hiplib):
    assert "ocn_cn3_flags" in _lib.SIGNATURES and hasattr(hiplib, "ocn_cn3_flags")
    hdr = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    m = re.search(r"int ocn_cn3_flags\((.*?)\);", hdr, re.S)
    assert m and len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == len(_lib.SIGNATURES["ocn_cn3_flags"][1])
    assert "#define OCN_ABI_VERSION 9" in hdr and hiplib.ocn_abi_version() == 9 and _lib.ABI_VERSION == 9
    later = hdr[hdr.index("Later additions to 9"):hdr.index("#define OCN_ABI_VERSION")]
    assert "ocn_cn3_flags" in later


def test_cn3_flags_unit_compiles_alone_for_gfx950(tmp_path):
    """One kernel, wave64, no scratch, no spilled register, no dynamic stack."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "cn3_flags.s"
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ocn_amd", "csrc"),
                    os.path.join(ROOT, "ocn_amd", "csrc", "cn3_flags.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.vgpr_spill_count:\s+(\d+)", text, re.S):
        kernel, body, spills = m.group(1), m.group(2), int(m.group(3))
        if ".private_segment_fixed_size" in body:
            seen[kernel] = (spills, int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1)))
    assert len(seen) == 1 and all("cn3_flags_kernel" in k for k in seen), sorted(seen)
    assert all(v == (0, 0) for v in seen.values()), seen
    assert re.findall(r"\.wavefront_size:\s+(\d+)", text) == ["64"]


def test_cn3_flags_rejects_bad_arguments_before_any_hip_call(hiplib):
    """Every call here is invalid or empty, so none reaches a launch: the pointers are never dereferenced."""
    P, Z = c_void_p(4096), c_void_p(0)

    def call(**kw):
        a = dict(rowptrA=P, colA=P, rowptrT=P, colT=P, bm=P, stride=2, src=P, dst=P, order=Z, B=4, n_cols=64, off=P, flags=P,
                 cap=16, hist=P, cnt3=P, status=P, nds=Z, chunk_off=P)
        a.update(kw)
        return hiplib.ocn_cn3_flags(a["rowptrA"], a["colA"], a["rowptrT"], a["colT"], a["bm"], a["stride"], a["src"], a["dst"],
                                    a["order"], a["B"], a["n_cols"], a["off"], a["flags"], a["cap"], a["hist"], a["cnt3"],
                                    a["status"], a["nds"], a["chunk_off"], Z)

    for name in ("rowptrA", "rowptrT", "bm", "src", "dst", "off", "flags", "hist", "cnt3", "status", "chunk_off"):
        assert call(**{name: Z}) == -1, name
    assert call(B=-1) == -1 and call(n_cols=-1) == -1 and call(cap=-1) == -1 and call(stride=-1) == -1
    assert call(B=1 << 21) == -1                                       # the histogram's field width
    assert call(stride=1) == -1                                        # 32 bits for 64 columns
    assert call(B=0, stride=1) == -1                                   # (an empty batch is still checked)
    assert call(B=0) == 0 and call(B=0, src=Z, dst=Z) == 0             # ... and a valid one launches nothing


@pytest.mark.parametrize("what", ["non_square", "size_mismatch"])
def test_three_hop_handles_refuse_shapes_that_are_no_adj_and_adj2(what):
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.utils import CNState3, adjoverlap_3hop
    adj, adj2 = _graphs()
    e = torch.tensor([[0], [1]])
    if what == "non_square":
        adj = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 3]]), sparse_sizes=(3, 4))
        adj2 = SparseTensor.from_edge_index(torch.tensor([[0], [1]]), sparse_sizes=(3, 4))
    else:
        adj2 = SparseTensor.from_edge_index(torch.tensor([[0], [1]]), sparse_sizes=(4, 4))
    with pytest.raises(ValueError):
        adjoverlap_3hop(adj, adj2, e)
    with pytest.raises(ValueError):
        CNState3(adj, adj2, None, e)
    with pytest.raises(ValueError):
        adjoverlap_3hop(*_graphs(), torch.tensor([0, 1]))              # tarei must be [2, B]


def test_fuse3_takes_a_hop3_handle_of_the_same_adj2_only():
    from ocn_amd.utils import adjoverlap, adjoverlap_3hop, fuse3
    adj, adj2 = _graphs()
    _, other = _graphs()                                               # the same matrix, another object
    e = torch.tensor([[0], [1]])
    cn1, cn2 = adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e)
    with pytest.raises(NotImplementedError, match="adj2 object"):
        fuse3(cn1, cn2, adjoverlap_3hop(adj, other, e), e)
    with pytest.raises(NotImplementedError):                           # hop3 is the third handle, nothing else
        fuse3(cn1, adjoverlap_3hop(adj, adj2, e), adjoverlap_3hop(adj, adj2, e), e)
    with pytest.raises(NotImplementedError):
        fuse3(cn1, cn2, adjoverlap_3hop(adj, adj2, torch.tensor([[1], [2]])), e)
    h3 = adjoverlap_3hop(adj, adj2, e, undirected=False)
    assert h3.mode == "hop3" and h3.undirected is False and h3.sizes() == [1, 3] and h3.fused is None
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):         # the matching handle goes on to the device pass
        fuse3(cn1, cn2, adjoverlap_3hop(adj, adj2, e), e)


def test_cn3_flags_wrapper_checks_shapes_before_the_library(monkeypatch):
    from ocn_amd import ops
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    rp, col = torch.tensor([0, 1, 2, 2]), torch.tensor([1, 0], dtype=torch.int32)
    src, dst, off = torch.tensor([0]), torch.tensor([2]), torch.tensor([0, 1])
    ok = torch.zeros(3, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="does not match the adjacency"):
        ops.cn3_flags(rp, col, rp, col, torch.zeros(2, 1, dtype=torch.int32), src, dst, 3, off, None, 1)      # rows != n
    with pytest.raises(ValueError, match="does not match the adjacency"):
        ops.cn3_flags(rp, col, torch.zeros(41, dtype=torch.int64), col, ok, src, dst, 40, off, None, 1)       # 32 bits for 40 columns
    with pytest.raises(ValueError, match="transpose"):
        ops.cn3_flags(rp, col, rp[:-1], col, ok, src, dst, 3, off, None, 1)
    with pytest.raises(ValueError, match="off"):
        ops.cn3_flags(rp, col, rp, col, ok, src, dst, 3, off[:1], None, 1)
    with pytest.raises(ValueError, match="order"):
        ops.cn3_flags(rp, col, rp, col, ok, src, dst, 3, off, torch.tensor([0, 1]), 1)
    with pytest.raises(ValueError, match="nds"):
        ops.cn3_flags(rp, col, rp, col, ok, src, dst, 3, off, None, 1, nds=torch.tensor([1]))
    with pytest.raises(ValueError, match="length mismatch"):
        ops.cn3_flags(rp, col, rp, col, ok, src, torch.tensor([1, 2]), 3, off, None, 1)


def test_scoring_loop_and_recommender_refuse_what_cn6_cannot_do(hiplib):
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import score_edges
    from ocn_amd.recommend import recommend_links
    adj, adj2 = _graphs()
    pred = predictor_dict["cn6"](16, 16, 1, 3, 0.0).eval()
    h, edges = torch.randn(3, 16), torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="one GPU"):
        score_edges(pred, h, adj, adj2, edges, 2, group=True)
    with pytest.raises(ValueError, match="adj2"):
        score_edges(pred, h, adj, None, edges, 2)
    with pytest.raises(ValueError, match="no 3-hop form"):
        recommend_links(pred, h, adj, None, torch.tensor([0, 1]), 2, 2)
