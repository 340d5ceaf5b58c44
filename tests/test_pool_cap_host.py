"""The capped pooling (ocn_cn_gather_cap, ``ops.cn_gather_cap``, ``predictor.set_cn_cap``) without a GPU: the symbol and its
ABI entry, the argument checks of the C entry, the kernels' register budget, the wrapper's shape checks, the structure and the
unbiasedness of the sample as tests/pool_cap_mirror.py states it, and the setter with every refusal that happens before a
device operand is reached."""
import math
import os
import re
import subprocess
from ctypes import c_void_p
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ocn_amd import _lib
from tests import pool_cap_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C entry ------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_everywhere_and_the_abi_is_still_9(hiplib):
    assert "ocn_cn_gather_cap" in _lib.SIGNATURES and hasattr(hiplib, "ocn_cn_gather_cap")
    hdr = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)
    m = re.search(r"int ocn_cn_gather_cap\((.*?)\);", hdr, re.S)
    assert m and len(strip(m.group(1)).split(",")) == len(_lib.SIGNATURES["ocn_cn_gather_cap"][1])
    # ocn_cn_gather's arguments without rowsum, plus cap, seed and mult
    assert len(_lib.SIGNATURES["ocn_cn_gather_cap"][1]) == len(_lib.SIGNATURES["ocn_cn_gather"][1]) - 1 + 3
    args = strip(m.group(1))
    assert "rowsum" not in args and "int32_t cap" in args and "uint64_t seed" in args and "int32_t* mult" in args
    history = re.search(r"/\* ABI history.*?\*/", hdr, re.S).group(0)
    assert "ocn_cn_gather_cap" in history[history.index("Later additions to 9"):]
    assert "#define OCN_ABI_VERSION 9" in hdr and _lib.ABI_VERSION == 9 and hiplib.ocn_abi_version() == 9
    src = open(os.path.join(ROOT, "ocn_amd", "csrc", "cn_pool_cap.hip")).read()
    assert '#include "lane_group.h"' in src and '#include "philox.h"' in src and "OCN_X_" not in src
    assert "SAMPLE_STREAM_CN_CAP = 7u" in open(os.path.join(ROOT, "ocn_amd", "csrc", "philox.h")).read()
    assert M.STREAM_CN_CAP == 7


def test_entry_rejects_bad_arguments_before_any_hip_call(hiplib):
    """Every call but the last ones is invalid, so none reaches a launch: the pointers are never dereferenced (no GPU here)."""
    P, Z = c_void_p(4096), c_void_p(0)

    def call(**kw):
        a = dict(rowptrA=P, colA=P, src=P, dst=P, order=Z, B=4, off=P, flags=P, wc=Z, weights=P, h=P, H=64, mrl=10,
                 x1=P, x2=P, x3=P, out_row=Z, cnt1=Z, cnt2=Z, rec=Z, perm=Z, cap=8, seed=3, mult=Z)
        a.update(kw)
        return hiplib.ocn_cn_gather_cap(a["rowptrA"], a["colA"], a["src"], a["dst"], a["order"], a["B"], a["off"], a["flags"], a["wc"],
                                        a["weights"], a["h"], a["H"], a["mrl"], a["x1"], a["x2"], a["x3"], a["out_row"], a["cnt1"],
                                        a["cnt2"], a["rec"], a["perm"], a["cap"], a["seed"], a["mult"], Z)

    for name in ("rowptrA", "colA", "src", "dst", "off", "flags", "weights", "h", "x1", "x2", "x3"):
        assert call(**{name: Z}) == -1, name
        assert call(**{name: Z}, mult=P) == -1, name
    assert call(B=-1) == -1
    for cap in (0, -1, -(1 << 31)):
        assert call(cap=cap) == -1, cap
    for H in (0, -64, 8, 24, 48, 100, 192, 1024):
        assert call(H=H) == -1, H
    assert call(B=0, H=7) == -1 and call(B=0, cap=0) == -1                # an empty batch's width and cap are still checked
    for H in (16, 32, 64, 128, 256, 512):
        assert call(B=0, H=H) == 0 and call(B=0, H=H, cap=1, seed=(1 << 64) - 1, mult=P) == 0
    assert call(B=0, src=Z, dst=Z, off=Z, flags=Z, x1=Z, x2=Z, x3=Z) == 0      # (an empty batch's tensors have no storage)


def test_kernels_do_not_spill(tmp_path):
    """Six instances (one per width) for gfx950, none with scratch, a spilled register or a dynamic stack."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = tmp_path / "cn_pool_cap.s"
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ocn_amd", "csrc"),
                    os.path.join(ROOT, "ocn_amd", "csrc", "cn_pool_cap.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)(.*?)\.vgpr_spill_count:\s+(\d+)", text, re.S):
        kernel, body, spills = m.group(1), m.group(2), int(m.group(3))
        if ".private_segment_fixed_size" in body:
            seen[kernel] = (spills, int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", body).group(1)))
    assert len(seen) == 6 and all("cn_gather_cap_kernel" in k for k in seen), sorted(seen)
    assert all(v == (0, 0) for v in seen.values()), seen
    assert re.findall(r"\.wavefront_size:\s+(\d+)", text) == ["64"] * 6
    assert re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text) == ["0"] * 6          # no LDS
    assert not re.search(r"(global|flat|buffer)_atomic", text)


# ---- the wrapper ------------------------------------------------------------------------------------------------------------------
def test_wrapper_checks_before_the_library(monkeypatch):
    """``ops.cn_gather_cap``: the table's dtype and shape, the cap, the seed and ``mult`` are checked on the host.  The device
    check is patched out: these are host-side errors, raised before any library call."""
    from ocn_amd import ops
    rp, col = torch.tensor([0, 1, 2, 2]), torch.tensor([1, 0], dtype=torch.int32)
    src, dst, off, flags = torch.tensor([0]), torch.tensor([2]), torch.tensor([0, 1]), torch.zeros(1, dtype=torch.uint8)
    h, w = torch.randn(3, 16), torch.randn(3, 4)
    call = lambda h=h, w=w, cap=4, seed=0, **kw: ops.cn_gather_cap(rp, col, src, dst, off, flags, None, w, h, cap, seed, **kw)
    for dt in (torch.bfloat16, torch.float16):                                   # (before the device check: from the dtype alone)
        with pytest.raises(TypeError, match="fp32|float32"):
            call(h=h.to(dt))
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        call()
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    with pytest.raises(ValueError, match=r"weights must be \[N,4\]"):
        call(w=torch.randn(4, 4))
    with pytest.raises(ValueError, match=r"weights must be \[N,4\]"):
        call(w=torch.randn(3, 3))
    for cap in (0, -3, 1 << 31):
        with pytest.raises(ValueError, match="cap"):
            call(cap=cap)
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            call(seed=seed)
    with pytest.raises(NotImplementedError, match="widths"):
        call(h=torch.randn(3, 24))
    with pytest.raises(ValueError, match="mult"):
        call(mult=torch.zeros(0, dtype=torch.int32))


# ---- the sample's structure -------------------------------------------------------------------------------------------------------
def test_strata_tile_the_ranks():
    for u in range(2, 200):
        for d in range(1, u):
            st = M.strata(u, d)
            assert len(st) == d and st[0][0] == 0 and st[-1][1] == u
            assert all(st[t][1] == st[t + 1][0] for t in range(d - 1))
            assert {hi - lo for lo, hi in st} <= {u // d, -(-u // d)} and min(hi - lo for lo, hi in st) >= 1
            for t, (lo, hi) in enumerate(st):
                assert M.stratum_of(lo, u, d) == t and M.stratum_of(hi - 1, u, d) == t


def test_multipliers_sum_to_u_and_select_min_u_d():
    rng = np.random.default_rng(0)
    for trial in range(300):
        n = int(rng.integers(1, 90))
        member = rng.random(n) < rng.random()
        u, d = int(member.sum()), int(rng.integers(1, 40))
        s = M.multipliers(member, int(rng.integers(0, 1000)), int(rng.integers(0, 1000)), d, int(rng.integers(0, 1 << 62)))
        assert len(s) == n and sum(s) == u and sum(v > 0 for v in s) == min(u, d)
        assert all(v == 0 for v, m in zip(s, member) if not m)
        if u <= d:
            assert s == [int(m) for m in member]
        else:                                                                     # one per stratum, carrying its size
            ranks = [r for r, p in enumerate(np.flatnonzero(member)) if s[p]]
            for t, (lo, hi) in enumerate(M.strata(u, d)):
                assert lo <= ranks[t] < hi and s[np.flatnonzero(member)[ranks[t]]] == hi - lo
    # fixed by (seed, i, j, members): the same call twice; non-members in between change positions, not ranks
    a = M.multipliers([1] * 37, 3, 11, 5, 9)
    assert a == M.multipliers([1] * 37, 3, 11, 5, 9)
    b = M.multipliers([1, 0] * 37, 3, 11, 5, 9)
    assert b[0::2] == a and not any(b[1::2])
    assert any(M.multipliers([1] * 37, 3, 11, 5, sd) != a for sd in range(1, 4))
    assert M.multipliers([1] * 37, 4, 11, 5, 9) != a or M.multipliers([1] * 37, 3, 12, 5, 9) != a


def test_the_estimate_is_unbiased():
    """Seeds 0 .. 4095, candidate (3, 11), u = 37, d = 5, x_r = r + 1 (sum 703): the mean of the estimate within 4 standard
    errors of 703 — the standard error from the exact stratified variance sum_t s_t^2 Var_t — and every member's inclusion
    frequency within 4 binomial standard errors of 1 / s_t.  Deterministic: the seeds are fixed."""
    u, d, n = 37, 5, 4096
    x = np.arange(1, u + 1, dtype=np.float64)
    est, hits = np.zeros(n), np.zeros(u)
    for seed in range(n):
        s = np.array(M.multipliers([1] * u, 3, 11, d, seed), dtype=np.float64)
        est[seed] = (s * x).sum()
        hits += s > 0
    var = sum((hi - lo) ** 2 * x[lo:hi].var() for lo, hi in M.strata(u, d))      # (population variance of one uniform draw)
    z = (est.mean() - 703.0) / math.sqrt(var / n)
    print("z of the mean:", z)
    assert abs(z) <= 4
    zmax = 0.0
    for lo, hi in M.strata(u, d):
        p = 1.0 / (hi - lo)
        for r in range(lo, hi):
            zmax = max(zmax, abs(hits[r] / n - p) / math.sqrt(p * (1 - p) / n))
    print("max |z| of the inclusion frequencies:", zmax)
    assert zmax <= 4


# ---- the setter -------------------------------------------------------------------------------------------------------------------
def _tiny():
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.utils import adjoverlap
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(4, 4))
    e = torch.tensor([[0, 2], [2, 0]])
    return adj, e, (adjoverlap(adj, adj, e), adjoverlap(adj, adj, e))


@pytest.mark.parametrize("name", ["cn5", "cn7", "cn8"])
def test_set_cn_cap_and_its_refusals(hiplib, monkeypatch, name):
    from ocn_amd import ops
    from ocn_amd.explain import explain_link_edges, explain_links
    from ocn_amd.model import predictor_dict
    adj, e, (cn1, cn2) = _tiny()
    args = SimpleNamespace(sum=1.0)
    pred = predictor_dict[name](16, 16, 1, 3, 0.0).eval()
    keys = set(pred.state_dict())
    assert pred.set_cn_cap(8) is None and pred.set_cn_cap(4, seed=7) == (8, 0) and pred.set_cn_cap(None) == (4, 7)
    assert pred.set_cn_cap(None) is None
    for bad in (0, -1, 2.0, "8", True, 1 << 31):
        with pytest.raises(ValueError, match="cap"):
            pred.set_cn_cap(bad)
    for bad in (-1, 1 << 64, 0.5, True):
        with pytest.raises(ValueError, match="seed"):
            pred.set_cn_cap(4, seed=bad)
    assert pred._cn_cap is None
    pred.set_cn_cap(2, seed=5)
    assert set(pred.state_dict()) == keys == set(predictor_dict[name](16, 16, 1, 3, 0.0).state_dict())
    x = torch.randn(4, 16)
    call = (lambda x: pred(x, adj, cn1, cn2, e)) if name == "cn5" else (lambda x: pred.multidomainforward(x, adj, cn1, cn2, e, args))
    for fused in (False, True):                                                   # (asked for or not: refused before the one-pass forms)
        monkeypatch.setattr(ops, "cn8_fused_eval", fused)
        monkeypatch.setattr(ops, "frozen_fused_eval", fused)
        with pytest.raises(RuntimeError, match="eval path"):                      # autograd on
            call(x)
        pred.train()
        with torch.no_grad(), pytest.raises(RuntimeError, match="eval path"):
            call(x)
        with torch.no_grad(), pytest.raises(RuntimeError, match="no-grad scoring path"):
            pred.begin(x, adj, cn1, cn2, e, args=args)
        pred.eval()
        pred.set_edge_sharding(None, True)
        with torch.no_grad(), pytest.raises(RuntimeError, match="sharded"):
            call(x)
        with torch.no_grad(), pytest.raises(RuntimeError, match="sharded"):
            pred.begin(x, adj, cn1, cn2, e, args=args)
        pred.set_edge_sharding(None, False)
        for dt in (torch.bfloat16, torch.float16):
            with torch.no_grad(), pytest.raises(TypeError, match="fp32|float32"):
                call(x.to(dt))
            with torch.no_grad(), pytest.raises(TypeError, match="fp32|float32"):
                pred.begin(x.to(dt), adj, cn1, cn2, e, args=args)
        # eval under no_grad is the path that takes it: the call gets as far as the device check (no CPU path)
        with torch.no_grad(), pytest.raises(_lib.OcnHipError, match="no CPU path"):
            call(x)
    edges = e.t().contiguous()
    with pytest.raises(RuntimeError, match="exact pooling"):
        explain_links(pred, x, adj, adj, edges, m=2, args=args)
    encoder = SimpleNamespace(training=False, convs=[SimpleNamespace(aggr="sum")])
    with pytest.raises(RuntimeError, match="exact pooling"):
        explain_link_edges(encoder, pred, x, adj, adj, edges, 0, top=2, args=args)
    pred.set_cn_cap(None)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):                    # (... and explains again)
        explain_links(pred, x, adj, adj, edges, m=2, args=args)


def test_cn6_refuses_a_cap():
    from ocn_amd.model import predictor_dict
    pred = predictor_dict["cn6"](16, 16, 1, 3, 0.0).eval()
    with pytest.raises(NotImplementedError, match="cn6"):
        pred.set_cn_cap(8)
    assert pred.set_cn_cap(None) is None


def test_adjoverlap_keeps_refusing_the_reference_knob():
    """``cnsampledeg`` has the reference's semantics (column sums of the sample, ``torch.rand`` draws), not these."""
    from ocn_amd.utils import adjoverlap
    adj, e, _ = _tiny()
    with pytest.raises(NotImplementedError):
        adjoverlap(adj, adj, e, cnsampledeg=8)
