"""Link heuristics (ocn_amd/heuristics.py, ``ocn_cn_node_sums``) without a GPU: the entry's declaration, its argument checks,
the wrapper's shape checks, the public module's refusals and the kernel's register budget."""
import os
import re
import subprocess
from ctypes import c_void_p

import pytest
import torch

from ocn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = os.path.join(ROOT, "ocn_amd", "csrc", "cn_heur.hip")


def test_cn_node_sums_symbol_is_declared_everywhere(hiplib):
    assert "ocn_cn_node_sums" in _lib.SIGNATURES and hasattr(hiplib, "ocn_cn_node_sums")
    hdr = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    m = re.search(r"int ocn_cn_node_sums\((.*?)\);", hdr, re.S)
    assert m and len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == len(_lib.SIGNATURES["ocn_cn_node_sums"][1]) == 22
    assert hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9           # an addition to ABI 9
    assert "ocn_cn8_pool" in _lib.SIGNATURES                            # ... beside the entry it is modelled on


def test_cn_node_sums_rejects_bad_arguments_before_any_hip_call(hiplib):
    """Every call here but the last is invalid, so none reaches a launch: the pointers are never dereferenced (no GPU here)."""
    P = c_void_p(4096)         # a non-NULL address that is never read
    Z = c_void_p(0)

    def call(**kw):
        a = dict(rowptrA=P, colA=P, rp1=P, c1=P, rp2=P, c2=P, bm1=Z, s1=0, bm2=Z, s2=0, src=P, dst=P, order=Z, B=4, n_cols=64,
                 w=P, sum1=P, sum2=P, cnt1=P, cnt2=P, deg=P)
        a.update(kw)
        return hiplib.ocn_cn_node_sums(a["rowptrA"], a["colA"], a["rp1"], a["c1"], a["rp2"], a["c2"], a["bm1"], a["s1"], a["bm2"],
                                       a["s2"], a["src"], a["dst"], a["order"], a["B"], a["n_cols"], a["w"], a["sum1"], a["sum2"],
                                       a["cnt1"], a["cnt2"], a["deg"], Z)

    for name in ("rowptrA", "colA", "src", "dst", "w", "sum1", "sum2", "cnt1", "cnt2"):
        assert call(**{name: Z}) == -1, name
    assert call(B=-1) == -1 and call(n_cols=-1) == -1
    assert call(rp1=Z, c1=Z, deg=Z) == -1 and call(c1=Z) == -1          # T1: neither CSR nor bit rows
    assert call(rp2=Z) == -1 and call(c2=Z) == -1                       # T2: half a CSR and no bit rows
    assert call(bm1=P, s1=1) == -1 and call(bm2=P, s2=1) == -1          # bit rows narrower than the columns
    assert call(bm1=P, s1=-2, n_cols=0) == -1
    assert call(rp1=Z, c1=Z, bm1=P, s1=2) == -1                         # deg needs T1's row pointers
    assert call(B=0, w=Z) == -1                                         # (an empty batch is still checked)
    assert call(B=0) == 0                                               # ... and a valid one launches nothing
    assert call(B=0, rp2=Z, c2=Z) == 0                                  # all of T2 may be NULL
    assert call(B=0, rp1=Z, c1=Z, bm1=P, s1=2, deg=Z) == 0              # T1 as bit rows alone, without deg
    assert call(B=0, rp2=Z, c2=Z, bm2=P, s2=2, deg=Z) == 0


def test_cn_node_sums_wrapper_refuses_cpu_tensors_and_wrong_dtypes(hiplib, monkeypatch):
    from ocn_amd import ops
    from ocn_amd.sparse import SparseTensor
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(3, 3))
    e = torch.tensor([[0], [1]])
    csr = (adj._rowptr, adj._col)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.cn_node_sums(adj._rowptr, adj._col, csr, csr, e[0], e[1], torch.zeros(3, 4))
    # dtype and rank are checked by ``_req`` after the device: patch the device test out, keep the rest
    real = ops._req

    class _Cuda(torch.Tensor):
        is_cuda = True

    def req(t, dtype, name, ndim=None):
        return real(t.as_subclass(_Cuda) if isinstance(t, torch.Tensor) else t, dtype, name, ndim)
    monkeypatch.setattr(ops, "_req", req)
    with pytest.raises(TypeError, match="w: expected torch.float32"):
        ops.cn_node_sums(adj._rowptr, adj._col, csr, csr, e[0], e[1], torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(TypeError, match="src: expected torch.int64"):
        ops.cn_node_sums(adj._rowptr, adj._col, csr, csr, e[0].int(), e[1], torch.zeros(3, 4))
    with pytest.raises(TypeError, match="colA: expected torch.int32"):
        ops.cn_node_sums(adj._rowptr, adj._col.long(), csr, csr, e[0], e[1], torch.zeros(3, 4))
    with pytest.raises(ValueError, match="w: expected 2-d"):
        ops.cn_node_sums(adj._rowptr, adj._col, csr, csr, e[0], e[1], torch.zeros(12))
    with pytest.raises(TypeError, match="t2_bitmap: expected torch.int32"):
        ops.cn_node_sums(adj._rowptr, adj._col, csr, None, e[0], e[1], torch.zeros(3, 4), t2_bitmap=torch.zeros(3, 1))


def test_cn_node_sums_wrapper_checks_shapes_before_the_library(monkeypatch):
    """What the kernel indexes is bounded on the host: T1 and T2 with one row count (``dst`` is checked against it), bit rows
    wide enough for the columns, a table with four weights per column.  Host-side errors, raised before any library call."""
    from ocn_amd import ops
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    rp, col = torch.tensor([0, 1, 2, 2]), torch.tensor([1, 0], dtype=torch.int32)
    src, dst, w = torch.tensor([0]), torch.tensor([2]), torch.zeros(3, 4)
    bm3, bm2 = torch.zeros(3, 1, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="T1 has 3 rows, T2 2"):
        ops.cn_node_sums(rp, col, (rp, col), None, src, dst, w, t2_bitmap=bm2)
    with pytest.raises(ValueError, match="T1 has 2 rows, T2 3"):
        ops.cn_node_sums(rp, col, None, (rp, col), src, dst, w, t1_bitmap=bm2)
    with pytest.raises(ValueError, match="does not match"):
        ops.cn_node_sums(rp, col, (rp, col), (rp, col), src, dst, w, t1_bitmap=bm2)
    with pytest.raises(ValueError, match="does not match"):
        ops.cn_node_sums(rp, col, (rp, col), None, src, dst, torch.zeros(40, 4), t2_bitmap=bm3)      # 32 bits for 40 columns
    with pytest.raises(ValueError, match="3 rows, the adjacency 5 columns"):
        ops.cn_node_sums(rp, col, (rp, col), (rp, col), src, dst, w, n_cols=5)
    with pytest.raises(ValueError, match="T1: needs its CSR arrays or its bit rows"):
        ops.cn_node_sums(rp, col, None, (rp, col), src, dst, w)
    with pytest.raises(ValueError, match=r"w must be \[N, 4\]"):
        ops.cn_node_sums(rp, col, (rp, col), (rp, col), src, dst, torch.zeros(3, 2))
    with pytest.raises(ValueError, match="src/dst length mismatch"):
        ops.cn_node_sums(rp, col, (rp, col), None, src, torch.tensor([1, 2]), w)
    with pytest.raises(ValueError, match="order: one entry per candidate"):
        ops.cn_node_sums(rp, col, (rp, col), None, src, dst, w, order=torch.tensor([0, 1]))


def test_link_heuristics_refuses_unknown_kinds_missing_adj2_and_cpu_graphs(hiplib):
    from ocn_amd import heuristics as Hx
    from ocn_amd.sparse import SparseTensor
    assert Hx.KINDS == ("cn", "aa", "ra", "jaccard", "pa", "cn2", "aa2", "ra2")
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(3, 3))
    e = torch.tensor([[0], [1]])
    with pytest.raises(ValueError, match="unknown heuristic 'katz'"):
        Hx.link_heuristics(adj, adj, e, kinds=("cn", "katz"))
    for kind in ("cn2", "aa2", "ra2"):
        with pytest.raises(ValueError, match=f"'{kind}'"):
            Hx.link_heuristics(adj, None, e, kinds=("cn", kind))
        with pytest.raises(ValueError, match=f"'{kind}'"):
            Hx.score_edges_heuristic(adj, None, e.t(), 8, kind)
    with pytest.raises(ValueError, match="unknown heuristic"):
        Hx.score_edges_heuristic(adj, adj, e.t(), 8, "common")
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):          # the product path has no CPU form
        Hx.link_heuristics(adj, None, e, kinds=("cn",))
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        Hx.weighted_cn(adj, None, e, torch.ones(3))
    with pytest.raises(ValueError, match="needs node_weight"):
        Hx.weighted_cn(adj, None, e, None)


def test_cn_heur_kernels_do_not_spill(tmp_path):
    """The unit compiled for gfx950: two instances (with and without a 2-hop matrix), neither with scratch, a spilled
    register or a dynamic stack; wave64."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "cn_heur.s"
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ocn_amd", "csrc"), UNIT, "-o", str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.vgpr_spill_count:\s+(\d+)", text, re.S):
        kernel, body, spills = m.group(1), m.group(2), int(m.group(3))
        if ".private_segment_fixed_size" in body:
            seen[kernel] = (spills, int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1)))
    assert len(seen) == 2 and all("cn_node_sums_kernel" in k for k in seen), sorted(seen)
    assert all(v == (0, 0) for v in seen.values()), seen
    assert re.findall(r"\.wavefront_size:\s+(\d+)", text) == ["64"] * 2
    assert re.findall(r"\.sgpr_spill_count:\s+(\d+)", text) == ["0"] * 2
    assert "global_atomic" not in text and "ds_add" not in text          # no atomics, no LDS histogram


def test_cn_heur_source_names_no_experiment_switch():
    src = open(UNIT).read()
    for word in ("OCN_X_", "ocn_debug_", "s_memtime"):
        assert word not in src, word
