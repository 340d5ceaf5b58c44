"""Frozen column weights without a GPU: the argument checks of ``ocn_cn_pool_frozen``, its binding and its kernels' register
budget, the knob, ``FrozenColumns`` as a plain object, and the refusals that happen before any device work."""
import io
import os
import re
import subprocess
import sys
from ctypes import c_void_p
from types import SimpleNamespace

import pytest
import torch

from ocn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pool_frozen_symbol_is_declared_everywhere(hiplib):
    assert "ocn_cn_pool_frozen" in _lib.SIGNATURES and hasattr(hiplib, "ocn_cn_pool_frozen")
    hdr = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    m = re.search(r"int ocn_cn_pool_frozen\((.*?)\);", hdr, re.S)
    m8 = re.search(r"int ocn_cn8_pool\((.*?)\);", hdr, re.S)
    assert m and len(strip(m.group(1)).split(",")) == len(_lib.SIGNATURES["ocn_cn_pool_frozen"][1])
    # the signature of ocn_cn8_pool plus the table
    assert len(_lib.SIGNATURES["ocn_cn_pool_frozen"][1]) == len(_lib.SIGNATURES["ocn_cn8_pool"][1]) + 1
    assert "const float* weights" in strip(m.group(1)) and "weights" not in strip(m8.group(1))
    assert "ocn_cn_pool_frozen" in hdr[:hdr.index("#define OCN_ABI_VERSION")]          # ... listed among the additions to 9
    assert hiplib.ocn_abi_version() == 9 == _lib.ABI_VERSION


def test_pool_frozen_rejects_bad_arguments_before_any_hip_call(hiplib):
    """Every call here is invalid, so none reaches a launch: the pointers are never dereferenced (no GPU in this test)."""
    P = c_void_p(4096)         # a non-NULL, 16-byte aligned address that is never read
    Z = c_void_p(0)

    def call(**kw):
        a = dict(rowptrA=P, colA=P, rp1=P, c1=P, rp2=P, c2=P, bm1=Z, s1=0, bm2=Z, s2=0, src=P, dst=P, order=Z, B=4, n_cols=64,
                 w=P, h=P, H=64, x1=P, x2=P, x3=P, cnt1=P, cnt2=P)
        a.update(kw)
        return hiplib.ocn_cn_pool_frozen(a["rowptrA"], a["colA"], a["rp1"], a["c1"], a["rp2"], a["c2"], a["bm1"], a["s1"], a["bm2"],
                                         a["s2"], a["src"], a["dst"], a["order"], a["B"], a["n_cols"], a["w"], a["h"], a["H"],
                                         a["x1"], a["x2"], a["x3"], a["cnt1"], a["cnt2"], Z)

    for name in ("rowptrA", "colA", "src", "dst", "w", "h", "x1", "x2", "x3", "cnt1", "cnt2"):
        assert call(**{name: Z}) == -1, name
    assert call(B=-1) == -1 and call(n_cols=-1) == -1
    for H in (0, 8, 48, 100, 1024, -64):
        assert call(H=H) == -1, H
    assert call(w=c_void_p(4096 + 8)) == -1                            # the table is read 16 bytes at a time
    assert call(rp1=Z, c1=Z) == -1 and call(c1=Z) == -1              # T1: neither CSR nor bit rows
    assert call(rp2=Z, c2=Z) == -1 and call(rp2=Z) == -1              # T2 likewise
    assert call(rp1=Z, c1=Z, rp2=Z, c2=Z) == -1
    assert call(bm1=P, s1=1) == -1 and call(bm2=P, s2=1) == -1        # bit rows narrower than the columns
    assert call(B=0, H=7) == -1 and call(B=0, w=Z) == -1              # (an empty batch is still checked)
    assert call(B=0) == 0                                              # ... and a valid one launches nothing
    assert call(B=0, rp1=Z, c1=Z, bm1=P, s1=2, rp2=Z, c2=Z, bm2=P, s2=2) == 0


def test_pool_frozen_kernels_do_not_spill(tmp_path):
    """The unit of the one-pass kernel compiled for gfx950: six instances (one per width), none with scratch or a spilled
    register, none with a dynamic stack."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "cn_pool_frozen.s"
    src = os.path.join(ROOT, "ocn_amd", "csrc", "cn_pool_frozen.hip")
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ocn_amd", "csrc"), src, "-o", str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.vgpr_spill_count:\s+(\d+)", text, re.S):
        kernel, body, spills = m.group(1), m.group(2), int(m.group(3))
        if ".private_segment_fixed_size" in body:
            seen[kernel] = (spills, int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1)))
    assert len(seen) == 6 and all("cn_pool_frozen_kernel" in k for k in seen), sorted(seen)
    assert all(v == (0, 0) for v in seen.values()), seen
    assert re.findall(r"\.wavefront_size:\s+(\d+)", text) == ["64"] * 6
    assert "OCN_X_" not in open(src).read()


def test_frozen_one_pass_is_opt_in():
    """The one pass is opt-in (OCN_FROZEN_FUSED=1) until a measurement puts its range below the chain's; cn8's knob
    is its own."""
    from ocn_amd import ops
    assert ops.frozen_fused_eval == (os.environ.get("OCN_FROZEN_FUSED", "0") == "1")
    assert "OCN_FROZEN_FUSED" in os.environ or ops.frozen_fused_eval is False
    code = "from ocn_amd import ops; print(int(ops.frozen_fused_eval), int(ops.cn8_fused_eval))"      # (one fresh interpreter: the knob is read at import)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env={**os.environ, "OCN_FROZEN_FUSED": "1"}, check=True,
                         capture_output=True, text=True).stdout.split()
    assert out == ["1", str(int(ops.cn8_fused_eval))]


def table(kind="cn5", n=6, **kw):
    from ocn_amd.frozen import FrozenColumns
    base = dict(innerprod=0.0) if kind == "cn5" else dict(sum_fill=1.5, polyfirst=0, polysecond=0)
    base.update(kw)
    return FrozenColumns(weights=torch.arange(4.0 * n).reshape(n, 4), kind=kind, n_cols=n, valued=False, ref_size=3, **base)


def test_frozen_columns_is_a_plain_object_outside_the_state_dict():
    from ocn_amd.frozen import FrozenColumns
    from ocn_amd.model import predictor_dict
    fc = table("cn7")
    blob = io.BytesIO()
    torch.save(fc, blob)
    blob.seek(0)
    back = torch.load(blob)
    assert isinstance(back, FrozenColumns) and torch.equal(back.weights, fc.weights)
    assert (back.kind, back.n_cols, back.valued, back.ref_size, back.innerprod, back.sum_fill, back.polyfirst, back.polysecond) == \
        ("cn7", 6, False, 3, None, 1.5, 0, 0)
    moved = fc.to("cpu")
    assert moved is not fc and moved.kind == "cn7" and torch.equal(moved.weights, fc.weights)
    pred = predictor_dict["cn7"](8, 8, 1, 3, 0.0).eval()
    keys = set(pred.state_dict())
    assert pred.set_frozen_columns(fc) is None and pred.set_frozen_columns(fc, SimpleNamespace(sum=1.5)) is fc
    assert set(pred.state_dict()) == keys == set(predictor_dict["cn7"](8, 8, 1, 3, 0.0).state_dict())
    assert pred.set_frozen_columns(None) is fc and pred.set_frozen_columns(None) is None


def test_set_frozen_columns_checks_the_table_against_the_predictor():
    from ocn_amd.model import predictor_dict
    cn5 = predictor_dict["cn5"](8, 8, 1, 3, 0.0).eval()
    cn7 = predictor_dict["cn7"](8, 8, 1, 3, 0.0).eval()
    with pytest.raises(ValueError, match="batch-independent"):
        predictor_dict["cn8"](8, 8, 1, 3, 0.0).set_frozen_columns(table())
    with pytest.raises(NotImplementedError):
        predictor_dict["cn6"](8, 8, 1, 3, 0.0).set_frozen_columns(table())
    with pytest.raises(TypeError):
        cn5.set_frozen_columns(torch.zeros(6, 4))
    with pytest.raises(ValueError, match="cn7 table"):
        cn5.set_frozen_columns(table("cn7"))
    with pytest.raises(ValueError, match="cn5 table"):
        cn7.set_frozen_columns(table("cn5"))
    with pytest.raises(ValueError, match="innerprod"):
        cn5.set_frozen_columns(table(innerprod=0.37))
    with pytest.raises(ValueError, match="polysecond"):
        cn7.set_frozen_columns(table("cn7", polysecond=2))
    with pytest.raises(ValueError, match="sum_fill"):
        cn7.set_frozen_columns(table("cn7"), SimpleNamespace(sum=2.0))
    bad = table()
    bad.weights = bad.weights[:, :3]
    with pytest.raises(ValueError, match=r"\[n_cols, 4\]"):
        cn5.set_frozen_columns(bad)
    assert cn5._frozen is None and cn7._frozen is None
    cn7.polysecond = 2
    cn7.set_frozen_columns(table("cn7", polysecond=2))


def test_freeze_columns_refuses_before_any_device_work():
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.model import predictor_dict
    from ocn_amd.sparse import SparseTensor
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(3, 3))
    ref = torch.tensor([[0, 1]])
    cn5 = predictor_dict["cn5"](8, 8, 1, 3, 0.0).eval()
    with pytest.raises(ValueError, match="batch-independent"):
        freeze_columns(predictor_dict["cn8"](8, 8, 1, 3, 0.0).eval(), adj, adj, ref)
    with pytest.raises(NotImplementedError):
        freeze_columns(predictor_dict["cn6"](8, 8, 1, 3, 0.0).eval(), adj, adj, ref)
    with pytest.raises(TypeError):
        freeze_columns(torch.nn.Linear(2, 2), adj, adj, ref)
    cn5.set_edge_sharding(None, True)
    with pytest.raises(RuntimeError, match="sharded"):
        freeze_columns(cn5, adj, adj, ref)
    cn5.set_edge_sharding(None, False)
    with pytest.raises(RuntimeError, match="eval"):
        freeze_columns(cn5.train(), adj, adj, ref)
    cn5.eval()
    for bad in (ref[:0], ref.t().contiguous()[:1], ref.to(torch.int32), ref[0], [[0, 1]]):
        with pytest.raises(ValueError):
            freeze_columns(cn5, adj, adj, bad)
    with pytest.raises(ValueError, match="args"):
        freeze_columns(predictor_dict["cn7"](8, 8, 1, 3, 0.0).eval(), adj, adj, ref)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):         # ... and a valid request on CPU tensors reaches the device layer
        freeze_columns(cn5, adj, adj, ref)


@pytest.mark.parametrize("fused", [False, True], ids=["chain", "one_pass"])
def test_frozen_predictor_refuses_training_autograd_and_cpu_tensors(hiplib, monkeypatch, fused):
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.utils import adjoverlap
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(3, 3))
    e = torch.tensor([[0], [1]])
    pred = predictor_dict["cn5"](16, 16, 1, 3, 0.0).eval()
    pred.set_frozen_columns(table(n=3))
    monkeypatch.setattr(ops, "frozen_fused_eval", fused)
    x = torch.randn(3, 16)
    with pytest.raises(RuntimeError, match="eval path"):                # autograd on
        pred(x, adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj, e), e)
    pred.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="eval path"):
        pred(x, adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj, e), e)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no-grad scoring path"):
        pred.begin(x, adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj, e), e)
    pred.eval()
    assert pred.n == 0
    pred.set_edge_sharding(None, True)
    with torch.no_grad(), pytest.raises(RuntimeError, match="sharded"):
        pred(x, adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj, e), e)
    pred.set_edge_sharding(None, False)
    with torch.no_grad(), pytest.raises(_lib.OcnHipError, match="no CPU path"):
        pred(x, adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj, e), e)


def test_pool_frozen_wrapper_checks_shapes_before_the_library(monkeypatch):
    """``ops.cn_pool_frozen`` bounds what the kernel indexes, as ``ops.cn8_pool`` does, and the table with it: one row per row
    of ``h``, four columns.  The device check is patched out: these are host-side shape errors, raised before any library call."""
    from ocn_amd import ops
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    rp, col = torch.tensor([0, 1, 2, 2]), torch.tensor([1, 0], dtype=torch.int32)
    src, dst, h, w = torch.tensor([0]), torch.tensor([2]), torch.randn(3, 16), torch.randn(3, 4)
    bm3, bm2 = torch.zeros(3, 1, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"weights must be \[N, 4\]"):
        ops.cn_pool_frozen(rp, col, (rp, col), (rp, col), src, dst, h, torch.randn(4, 4))
    with pytest.raises(ValueError, match=r"weights must be \[N, 4\]"):
        ops.cn_pool_frozen(rp, col, (rp, col), (rp, col), src, dst, h, torch.randn(3, 3))
    with pytest.raises(ValueError, match="T1 has 3 rows, T2 2"):
        ops.cn_pool_frozen(rp, col, (rp, col), None, src, dst, h, w, t2_bitmap=bm2)
    with pytest.raises(ValueError, match="does not match"):
        ops.cn_pool_frozen(rp, col, (rp, col), None, src, dst, torch.randn(40, 16), torch.randn(40, 4), t2_bitmap=bm3)
    with pytest.raises(ValueError, match="3 rows, the adjacency 5 columns"):
        ops.cn_pool_frozen(rp, col, (rp, col), (rp, col), src, dst, h, w, n_cols=5)
    with pytest.raises(ValueError, match="needs its CSR arrays or its bit rows"):
        ops.cn_pool_frozen(rp, col, (rp, col), None, src, dst, h, w)
    with pytest.raises(NotImplementedError):
        ops.cn_pool_frozen(rp, col, (rp, col), (rp, col), src, dst, torch.randn(3, 24), w)
