"""The dense entries of the heads (linear.hip: ``ocn_linear_grouped``, ``ocn_linear_split_weight``, ``ocn_linear_panel_bytes``;
mlp_glue.hip: ``ocn_fill_rows``) without a GPU: every argument the entries refuse is refused before their first HIP call, and
the wrapper ``ops.linear_grouped`` refuses what it can see on the host."""
import ctypes
from ctypes import c_void_p

import pytest
import torch

from ocn_amd import _lib

P = c_void_p(4096)             # a non-NULL, 16-byte aligned address that is never read: every call below returns before its first HIP call
Z = c_void_p(0)


def _group(**kw):
    """A valid group of M = 0 rows (pointers set, strides 0 = packed); ``kw`` overrides fields."""
    g = _lib.OcnLinearGroup()
    g.X, g.Wp, g.Y, g.M = 4096, 4096, 4096, 0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _call(hiplib, groups, K=64, N=64, n=None):
    arr = (_lib.OcnLinearGroup * max(len(groups), 1))(*groups)
    return hiplib.ocn_linear_grouped(ctypes.cast(arr, c_void_p), len(groups) if n is None else n, K, N, Z)


def test_linear_grouped_rejects_bad_launch_arguments(hiplib):
    ok = [_group()]
    assert _call(hiplib, ok) == 0                                          # valid, every M = 0: launches nothing
    assert _call(hiplib, [_group() for _ in range(5)]) == 0
    assert hiplib.ocn_linear_grouped(Z, 1, 64, 64, Z) == -1                # NULL group array
    assert _call(hiplib, ok, n=0) == -1
    assert _call(hiplib, [_group() for _ in range(6)]) == -1
    for K in (0, 8, 24, -16):
        assert _call(hiplib, ok, K=K) == -1, K
    for N in (0, 48, 512, -32, 96):
        assert _call(hiplib, ok, N=N) == -1, N                            # ... although every M is 0
        assert _call(hiplib, [_group(M=1)], N=N) == -1, N
    for K in (16, 48, 64, 80, 512):
        for N in (32, 64, 128, 256):
            assert _call(hiplib, ok, K=K, N=N) == 0, (K, N)


def test_linear_grouped_rejects_bad_groups(hiplib):
    def one(**kw):
        return _call(hiplib, [_group(**kw)])

    assert one(M=-1) == -1
    for name in ("X", "Wp", "Y"):
        assert one(M=1, **{name: 0}) == -1, name
        assert one(**{name: 0}) == 0, name                                 # (nothing to read or write with M = 0)
    assert one(gamma=4096) == -1 and one(beta=4096) == -1                  # LayerNorm needs both
    assert one(gamma=4096, beta=4096) == 0
    assert one(ldX=60) == -1 and one(ldX=63) == -1 and one(ldX=66) == -1   # < K; not a multiple of 4
    assert one(ldX=64) == 0 and one(ldX=68) == 0
    assert one(ldY=60) == -1 and one(ldY=66) == -1
    assert one(ldY=64) == 0 and one(ldY=128) == 0
    assert one(ldY=1, dotw=4096) == 0 and one(ldY=66, dotw=4096) == 0      # the dot epilogue writes [M]: no row stride
    assert one(addend=4096, ldAdd=60) == -1 and one(addend=4096, ldAdd=66) == -1
    assert one(addend=4096) == 0 and one(addend=4096, ldAdd=68) == 0 and one(addend=4096, add_bcast=1) == 0
    assert one(addend=4096, dotw=4096) == -1                               # the dot epilogue adds nothing
    assert one(addend=4096, dotw=4096, add_bcast=1) == -1
    assert one(y_row_map=4096) == -1                                       # only the dot epilogue maps rows
    assert one(y_row_map=4096, dotw=4096) == 0
    assert one(row_range=4096) == 0 and one(row_range=4096, dotw=4096, y_row_map=4096) == 0
    for off in (4, 8, 12, 1):                                              # float4 accesses
        assert one(X=4096 + off) == -1, off
        assert one(Y=4096 + off) == -1, off
        assert one(addend=4096 + off) == -1, off
    assert one(Y=4096 + 4, dotw=4096) == 0                                 # one float per row
    # a bad group is found wherever it stands, and with M > 0 as well
    for pos in range(5):
        gs = [_group() for _ in range(5)]
        gs[pos] = _group(y_row_map=4096)
        assert _call(hiplib, gs) == -1, pos
    assert one(M=300, addend=4096, dotw=4096) == -1 and one(M=300, y_row_map=4096) == -1 and one(M=300, X=4100) == -1


def test_split_weight_fill_rows_and_panel_bytes_check_their_arguments(hiplib):
    sw = hiplib.ocn_linear_split_weight
    assert sw(Z, 64, 64, P, Z) == -1 and sw(P, 64, 64, Z, Z) == -1
    for N in (0, -32, 16, 48 + 8, 100):
        assert sw(P, N, 64, P, Z) == -1, N
    for K in (0, -16, 8, 24, 100):
        assert sw(P, 64, K, P, Z) == -1, K
    fr = hiplib.ocn_fill_rows
    for n_cols in (0, 6, -4):
        assert fr(P, 64, n_cols, P, P, 10, Z) == -1, n_cols
    assert fr(P, 28, 32, P, P, 10, Z) == -1 and fr(P, 34, 32, P, P, 10, Z) == -1     # ld < n_cols; ld % 4
    assert fr(P, 64, 32, P, P, -1, Z) == -1
    assert fr(Z, 64, 32, P, P, 10, Z) == -1 and fr(P, 64, 32, Z, P, 10, Z) == -1 and fr(P, 64, 32, P, Z, 10, Z) == -1
    assert fr(P, 64, 32, P, P, 0, Z) == 0 and fr(Z, 64, 32, Z, Z, 0, Z) == 0
    assert fr(P, 28, 32, P, P, 0, Z) == -1                                 # (an empty call is still checked)
    for N, K in ((32, 16), (64, 48), (256, 512), (128, 80)):
        assert hiplib.ocn_linear_panel_bytes(N, K) == 6 * N * K


def test_linear_grouped_wrapper_refusals(hiplib, monkeypatch):
    from ocn_amd import ops
    g = dict(x=torch.zeros(3, 64), weight=torch.zeros(64, 64), y=torch.zeros(3, 64))
    with pytest.raises(ValueError, match="1..5 groups"):
        ops.linear_grouped([], 64, 64)
    with pytest.raises(ValueError, match="1..5 groups"):
        ops.linear_grouped([g] * 6, 64, 64)
    with pytest.raises(ValueError, match="device tensor"):                 # no CPU path
        ops.linear_grouped([g], 64, 64)
    # the remaining checks come before any device work: let CPU tensors through the device check to reach them
    monkeypatch.setattr(ops, "_req_strided", lambda t, name: None)
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    monkeypatch.setattr(ops, "linear_panel", lambda w: (_ for _ in ()).throw(AssertionError("reached the device")))
    for bad in (dict(g, x=torch.zeros(3, 48)), dict(g, weight=torch.zeros(64, 48)), dict(g, weight=torch.zeros(32, 64)),
                dict(g, y=torch.zeros(4, 64))):
        with pytest.raises(ValueError, match="shape mismatch"):
            ops.linear_grouped([bad, g], 64, 64)
    for add in (torch.zeros(3, 64), torch.zeros(64), torch.zeros(1, 32), torch.zeros(2, 64)):
        with pytest.raises(ValueError, match=r"addend must be \[1, N\]"):
            ops.linear_grouped([dict(g, addend=add, add_bcast=True)], 64, 64)
    dot = (torch.zeros(1, 64), None)
    with pytest.raises(ValueError, match="takes no addend"):
        ops.linear_grouped([dict(g, y=torch.zeros(3, 1), dot=dot, addend=torch.zeros(3, 64))], 64, 64)
    with pytest.raises(ValueError, match="y_row_map needs the dot epilogue"):
        ops.linear_grouped([dict(g, y_row_map=torch.arange(3))], 64, 64)
    with pytest.raises(ValueError, match="y_row_map needs the dot epilogue"):
        ops.linear(torch.zeros(3, 64), torch.zeros(64, 64), y_row_map=torch.arange(3))
    with pytest.raises(AssertionError, match="reached the device"):       # (a valid group passes every host check)
        ops.linear_grouped([g], 64, 64)
