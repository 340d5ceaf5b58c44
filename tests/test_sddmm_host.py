"""The SDDMM entry without a GPU: the symbol of ``ocn_sddmm_csr`` in the header, the library and ``_lib``, its argument checks
(every refusal before any HIP call), the shape errors of ``ops.sddmm_csr`` (before the library) and the register budget of the
unit compiled for gfx950."""
import os
import re
import subprocess
from ctypes import c_void_p

import pytest
import torch

from ocn_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sddmm_symbol_is_declared_everywhere(hiplib):
    assert "ocn_sddmm_csr" in _lib.SIGNATURES and hasattr(hiplib, "ocn_sddmm_csr")
    hdr = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    m = re.search(r"int ocn_sddmm_csr\((.*?)\);", hdr, re.S)
    assert m and len(strip(m.group(1)).split(",")) == len(_lib.SIGNATURES["ocn_sddmm_csr"][1]) == 14
    # the parameters are those of ocn_spmm_csr, with g in front of x
    spmm = [a.split()[-1] for a in strip(re.search(r"int ocn_spmm_csr\((.*?)\);", hdr, re.S).group(1)).split(",")]
    mine = [a.split()[-1] for a in strip(m.group(1)).split(",")]
    assert [a for a in mine if a != "g"] == [a.replace("y", "out") if a == "y" else a for a in spmm]
    history = hdr[:hdr.index("#define OCN_ABI_VERSION")]
    assert "ocn_sddmm_csr" in history[history.index("Later additions to 9"):]
    assert "#define OCN_ABI_VERSION 9" in hdr
    assert hiplib.ocn_abi_version() == 9 == _lib.ABI_VERSION
    assert os.path.join(_lib.CSRC, "sddmm.hip") in _lib.sources()


def test_sddmm_rejects_bad_arguments_before_any_hip_call(hiplib):
    """Every call but the last ones is invalid, so none reaches a launch: the pointers are never dereferenced (no GPU in this
    test).  The valid ones have n_rows == 0 and launch nothing."""
    P = c_void_p(4096)         # a non-NULL, 16-byte aligned address that is never read
    Z = c_void_p(0)
    names = ("rowptr", "col", "val", "n", "g", "x", "F", "pre", "post", "mode", "edge_scale", "self_mode", "out")

    def call(**kw):
        a = dict(rowptr=P, col=P, val=Z, n=5, g=P, x=P, F=64, pre=Z, post=Z, mode=0, edge_scale=0, self_mode=0, out=P)
        a.update(kw)
        return hiplib.ocn_sddmm_csr(*[a[n] for n in names], Z)

    for F in (0, 8, 24, 48, 100, 1024, -64):
        assert call(F=F) == -1, F
    assert call(mode=2) == -1 and call(mode=3) == -1 and call(mode=-1) == -1
    assert call(mode=1, pre=P) == -1 and call(mode=1, post=P) == -1
    assert call(mode=1, self_mode=1) == -1 and call(mode=1, self_mode=2) == -1
    assert call(self_mode=3) == -1 and call(self_mode=-1) == -1
    for name in ("rowptr", "col", "g", "x", "out"):
        assert call(**{name: Z}) == -1, name
    for name in ("g", "x"):                                             # read 16 bytes at a time
        assert call(**{name: c_void_p(4096 + 8)}) == -1, name
        assert call(**{name: c_void_p(4096 + 4)}) == -1, name
    assert call(n=-1) == -1
    # an empty operator is still checked ...
    assert call(n=0, F=7) == -1 and call(n=0, mode=2) == -1 and call(n=0, g=Z) == -1 and call(n=0, x=c_void_p(4100)) == -1
    assert call(n=0, mode=1, pre=P) == -1
    # ... and a valid one launches nothing
    assert call(n=0) == 0
    assert call(n=0, val=P, pre=P, post=P, edge_scale=1, self_mode=2, F=512, out=c_void_p(4100)) == 0
    assert call(n=0, mode=1, val=P, F=16) == 0


def test_sddmm_wrapper_checks_shapes_before_the_library(monkeypatch):
    """``ops.sddmm_csr`` bounds what the kernel indexes.  The device check is patched out: these are host-side shape errors,
    raised before any library call."""
    from ocn_amd import ops
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    rp, col = torch.tensor([0, 1, 2, 2]), torch.tensor([1, 0], dtype=torch.int32)
    g, x = torch.randn(3, 16), torch.randn(3, 16)
    v3, v2 = torch.rand(3), torch.rand(2)
    with pytest.raises(ValueError, match=r"g must be \[n_rows, F\]"):
        ops.sddmm_csr(rp, col, torch.randn(2, 16), x)
    with pytest.raises(ValueError, match=r"g must be \[n_rows, F\]"):
        ops.sddmm_csr(rp, col, torch.randn(3, 32), x)
    with pytest.raises(ValueError, match="unsupported width"):
        ops.sddmm_csr(rp, col, torch.randn(3, 24), torch.randn(3, 24))
    with pytest.raises(ValueError, match="mode must be sum or mean"):
        ops.sddmm_csr(rp, col, g, x, mode="max")
    with pytest.raises(ValueError, match="mode must be sum or mean"):
        ops.sddmm_csr(rp, col, g, x, mode="min")
    for kw in (dict(pre=v3), dict(post=v3), dict(self_mode=1)):
        with pytest.raises(ValueError, match="mean takes no"):
            ops.sddmm_csr(rp, col, g, x, mode="mean", **kw)
    with pytest.raises(ValueError, match="self_mode must be"):
        ops.sddmm_csr(rp, col, g, x, self_mode=3)
    with pytest.raises(ValueError, match="pre must have one entry per row of x"):
        ops.sddmm_csr(rp, col, g, x, pre=v2)
    with pytest.raises(ValueError, match="edge_scale reads"):
        ops.sddmm_csr(rp, col, g, torch.randn(2, 16), pre=v2, edge_scale=True)
    with pytest.raises(ValueError, match="post must have one entry per output row"):
        ops.sddmm_csr(rp, col, g, x, post=v2)
    with pytest.raises(ValueError, match="square"):
        ops.sddmm_csr(rp, col, g, torch.randn(4, 16), self_mode=2)
    with pytest.raises(ValueError, match="val must have one entry per stored column"):
        ops.sddmm_csr(rp, col, g, x, val=v3)
    with pytest.raises(ValueError, match="out must hold"):
        ops.sddmm_csr(rp, col, g, x, out=torch.zeros(1))
    # no entry at all: nothing to launch, an empty result
    empty = ops.sddmm_csr(torch.zeros(4, dtype=torch.int64), col[:0], g, x)
    assert empty.shape == (0,) and empty.dtype == torch.float32


def test_sddmm_without_a_device_is_an_error_not_a_fallback(hiplib):
    from ocn_amd import ops
    rp, col = torch.tensor([0, 1, 2, 2]), torch.tensor([1, 0], dtype=torch.int32)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.sddmm_csr(rp, col, torch.randn(3, 16), torch.randn(3, 16))


def test_sddmm_kernels_do_not_spill(tmp_path):
    """The unit compiled for gfx950: six instances (one per width), wave64, none with scratch, a spilled register or LDS, and
    no atomic in the code."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "sddmm.s"
    src = os.path.join(ROOT, "ocn_amd", "csrc", "sddmm.hip")
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ocn_amd", "csrc"), src, "-o", str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.vgpr_spill_count:\s+(\d+)", text, re.S):
        kernel, body, spills = m.group(1), m.group(2), int(m.group(3))
        if ".private_segment_fixed_size" in body:
            seen[kernel] = (spills, int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1)),
                            int(re.search(r"\.sgpr_spill_count:\s+(\d+)", body).group(1)))
    assert len(seen) == 6 and all("sddmm_csr_kernel" in k for k in seen), sorted(seen)
    assert all(v == (0, 0, 0) for v in seen.values()), seen
    assert re.findall(r"\.wavefront_size:\s+(\d+)", text) == ["64"] * 6
    assert re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text) == ["0"] * 6
    assert "buffer_atomic" not in text and "global_atomic" not in text and "flat_atomic" not in text
    assert "atomic" not in open(src).read().split("#include")[1]        # (the code; the header comment says "no atomics")
