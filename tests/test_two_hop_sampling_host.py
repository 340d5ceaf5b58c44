"""The 2-hop hard-negative sampler (``ocn_sample_two_hop``, ``ocn_sample_two_hop_window_cols``; ocn_amd/sampling.py:
``two_hop_negative_targets``, ``two_hop_negative_edges``) without a GPU: the entries in the header and the binding, their
argument checks, the refusals of the Python layers, and the known answers of the CPU mirror the GPU tests compare against."""
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from ocn_amd import _lib
from tests import sampling_mirror as SM
from tests import two_hop_sampling_mirror as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = c_void_p(4096)             # a non-NULL address that is never read: every call below returns before its first HIP call
Z = c_void_p(0)
ENTRIES = ("ocn_sample_two_hop_window_cols", "ocn_sample_two_hop")


def test_two_hop_sampler_entries_are_later_additions_to_abi_9(hiplib):
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(hiplib, name)
    assert hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9
    with open(os.path.join(ROOT, "include", "ocn_hip.h")) as f:
        header = f.read()
    assert "#define OCN_ABI_VERSION 9" in header
    later = header[header.index("Later additions to 9"):header.index("#define OCN_ABI_VERSION")]
    for name in ENTRIES:
        assert name in later, name
        assert re.search(r"\b(int|int64_t) " + name + r"\(", header), name
    w = hiplib.ocn_sample_two_hop_window_cols()
    assert w > 0 and w % 64 == 0 and w < hiplib.ocn_two_hop_window_cols()      # the prefix table takes LDS from the bitmap


def _call(lib, **kw):
    a = dict(rpA=P, colA=P, rpM=P, colM=P, n=100, rows=P, Q=4, drop_self=1, window=0, sptr=P, sid=Z, q0=0, seed=7, count=Z, out=P)
    a.update(kw)
    return lib.ocn_sample_two_hop(a["rpA"], a["colA"], a["rpM"], a["colM"], a["n"], a["rows"], a["Q"], a["drop_self"], a["window"],
                                  a["sptr"], a["sid"], a["q0"], a["seed"], a["count"], a["out"], Z)


def test_two_hop_sampler_rejects_bad_arguments_before_any_hip_call(hiplib):
    for name in ("rpA", "colA", "rpM", "colM", "rows", "sptr", "out"):
        assert _call(hiplib, **{name: Z}) == -1, name
        assert _call(hiplib, Q=0, **{name: Z}) == -1, name            # an empty call is still checked
    assert _call(hiplib, Q=-1) == -1 and _call(hiplib, q0=-1) == -1 and _call(hiplib, Q=0, q0=-1) == -1
    for n in (0, -5, 1 << 31, 1 << 40):
        assert _call(hiplib, n=n) == -1 and _call(hiplib, Q=0, n=n) == -1, n
    limit = hiplib.ocn_sample_two_hop_window_cols()
    for window in (-64, 1, 63, 100, limit + 64, hiplib.ocn_two_hop_window_cols()):
        assert _call(hiplib, window=window) == -1 and _call(hiplib, Q=0, window=window) == -1, window
    # sid and count may be NULL or given; a valid empty call launches nothing
    assert _call(hiplib, Q=0) == 0 and _call(hiplib, Q=0, sid=P, count=P) == 0
    assert _call(hiplib, Q=0, window=64) == 0 and _call(hiplib, Q=0, window=limit) == 0
    assert _call(hiplib, Q=0, n=(1 << 31) - 1, q0=1 << 40, seed=(1 << 64) - 1, drop_self=0) == 0


def _tiny():
    from ocn_amd.sparse import SparseTensor
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(4, 4))
    wide = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(4, 5))
    big = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(5, 5))
    return adj, wide, big


def test_two_hop_samplers_refuse_operands_of_other_sizes(hiplib):
    from ocn_amd import sampling as S
    adj, wide, big = _tiny()
    src, pos = torch.tensor([0, 2]), torch.tensor([[0, 2], [1, 1]])
    for a, k in ((wide, None), (adj, wide), (adj, big)):
        with pytest.raises(ValueError, match="expected the square size"):
            S.two_hop_negative_targets(a, src, 3, 1, known=k)
        with pytest.raises(ValueError, match="expected the square size"):
            S.two_hop_negative_edges(a, pos, 1, known=k)


def test_two_hop_samplers_refuse_bad_sources_per_fallback_and_first(hiplib):
    from ocn_amd import sampling as S
    adj, _, _ = _tiny()
    for bad in (torch.tensor([0, 2], dtype=torch.int32), torch.tensor([[0, 2]]), [0, 2]):
        with pytest.raises(ValueError, match="sources must be a 1-d int64"):
            S.two_hop_negative_targets(adj, bad, 3, 1)
    for bad in (torch.tensor([[0, 2], [1, 1]], dtype=torch.int32), torch.tensor([0, 2]), torch.tensor([[0, 1, 2]]), [[0], [1]]):
        with pytest.raises(ValueError, match=r"pos_edges must be an int64 \[2, E\]"):
            S.two_hop_negative_edges(adj, bad, 1)
    for per in (0, -3):
        with pytest.raises(ValueError, match="per must be at least 1"):
            S.two_hop_negative_targets(adj, torch.tensor([0, 2]), per, 1)
    for fb in ("none", "Uniform", 0, True):
        with pytest.raises(ValueError, match="fallback must be 'uniform' or None"):
            S.two_hop_negative_targets(adj, torch.tensor([0, 2]), 3, 1, fallback=fb)
        with pytest.raises(ValueError, match="fallback must be 'uniform' or None"):
            S.two_hop_negative_edges(adj, torch.tensor([[0, 2], [1, 1]]), 1, fallback=fb)
    with pytest.raises(ValueError, match="first must not be negative"):
        S.two_hop_negative_edges(adj, torch.tensor([[0, 2], [1, 1]]), 1, first=-1)
    assert S.two_hop_negative_edges(adj, torch.zeros(2, 0, dtype=torch.int64), 1).shape == (2, 0)


def test_two_hop_samplers_have_no_cpu_path(hiplib):
    from ocn_amd import ops, sampling as S
    adj, _, _ = _tiny()
    src = torch.tensor([0, 2])
    for call in (lambda: S.two_hop_negative_targets(adj, src, 3, 1),
                 lambda: S.two_hop_negative_edges(adj, torch.tensor([[0, 2], [1, 1]]), 1),
                 lambda: ops.sample_two_hop(adj._rowptr, adj._col, adj._rowptr, adj._col, src, torch.tensor([0, 2, 4]), 1)):
        with pytest.raises(_lib.OcnHipError, match="no CPU path"):
            call()


def test_sample_two_hop_wrapper_checks_its_arguments_before_the_library(hiplib, monkeypatch):
    from ocn_amd import ops
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    monkeypatch.setattr(ops, "validate_indices", False)
    rp, col, rows = torch.tensor([0, 1, 2, 2]), torch.tensor([1, 0], dtype=torch.int32), torch.tensor([0, 1])
    sptr = torch.tensor([0, 2, 4])
    for window in (-64, 63, ops.sample_two_hop_window_cols() + 64):
        with pytest.raises(ValueError, match="window_cols must be 0 or a multiple of 64"):
            ops.sample_two_hop(rp, col, rp, col, rows, sptr, 1, window_cols=window)
    with pytest.raises(ValueError, match="sptr: one entry per query and the total"):
        ops.sample_two_hop(rp, col, rp, col, rows, torch.tensor([0, 2]), 1, total=2)
    with pytest.raises(ValueError, match="first must not be negative"):
        ops.sample_two_hop(rp, col, rp, col, rows, sptr, 1, first=-1, total=4)
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed must be in 0"):
            ops.sample_two_hop(rp, col, rp, col, rows, sptr, seed, total=4)
    with pytest.raises(ValueError, match="sid: one sample id per slot"):
        ops.sample_two_hop(rp, col, rp, col, rows, sptr, 1, sid=torch.tensor([0, 1, 2]), total=4)
    with pytest.raises(ValueError, match="P has 3 rows, M 2"):
        ops.sample_two_hop(rp, col, torch.tensor([0, 1, 2]), col, rows, sptr, 1, total=4)


def test_mirror_candidate_sets_of_the_hand_cases():
    for name, n, rows, want in TM.hand_cases():
        rowptr, col = TM.csr_of(n, rows)
        for s, h in want.items():
            assert TM.candidates(rowptr, col, s) == h, (name, s)
    # path 0-1-2-3-4 as the issue states it
    name, n, rows, _ = TM.hand_cases()[0]
    rowptr, col = TM.csr_of(n, rows)
    assert TM.candidates(rowptr, col, 0) == [2] and TM.candidates(rowptr, col, 2) == [0, 4]
    assert TM.candidates(rowptr, col, 2, drop_self=False) == [0, 2, 4]          # 2 - 1 - 2: the source is its own 2-hop neighbour
    # known != adj: a superset removes members, and only members
    k_rowptr, k_col = TM.csr_of(n, {**rows, 2: [0, 1, 3]})
    assert TM.candidates(rowptr, col, 2, k_rowptr, k_col) == [4]


def test_mirror_counters_and_selection():
    seed = (0x5EED << 32) | 0x1234
    # the two streams are those of the contract: counter words spelled out here once more
    for q, j, c in ((0, 0, 7), (3, 300, 50), ((1 << 33) + 5, 2, 1000)):
        w = SM.philox4x32((j, q & SM.MASK32, q >> 32, 3), SM.key_of(seed))
        assert TM.rank_slot(seed, q, j, c) == ((w[0] | (w[1] << 32)) * c) >> 64
    for sid, c in ((0, 7), (12345, 50), ((1 << 35) + 9, 1000)):
        w = SM.philox4x32((sid & SM.MASK32, sid >> 32, 0, 4), SM.key_of(seed))
        assert TM.rank_id(seed, sid, c) == ((w[0] | (w[1] << 32)) * c) >> 64
    # independent of the uniform samplers' streams 1 and 2 for the same index
    assert [TM.rank_slot(seed, 0, j, 1 << 40) for j in range(4)] != [SM.rank_rows(seed, 0, j, 1 << 40) for j in range(4)]
    assert [TM.rank_id(seed, t, 1 << 40) for t in range(4)] != [SM.rank_pairs(seed, t, 1 << 40) for t in range(4)]
    # through the sampler on the star: leaves draw other leaves, the centre has nothing; ragged and empty slot ranges
    name, n, rows, want = TM.hand_cases()[1]
    rowptr, col = TM.csr_of(n, rows)
    src = [1, 0, 3, 1, 5]
    sptr = [0, 40, 43, 43, 83, 90]                                              # query 2 owns no slot
    out, count = TM.sample_two_hop(rowptr, col, src, sptr, seed)
    assert count.tolist() == [4, 0, 4, 4, 4]
    assert (out[40:43] == -1).all() and set(out[:40].tolist()) == {2, 3, 4, 5} and set(out[43:83].tolist()) == {2, 3, 4, 5}
    assert out[:40].tolist() != out[43:83].tolist()                            # the same source at another position
    assert set(out[83:].tolist()) <= {1, 2, 3, 4}
    # a sample does not depend on the other queries or slots: query 3 alone at q0 = 3
    alone, _ = TM.sample_two_hop(rowptr, col, [1], [0, 40], seed, q0=3)
    assert alone.tolist() == out[43:83].tolist()
    # with sample ids a slot is fixed by its id, wherever it sits
    a, _ = TM.sample_two_hop(rowptr, col, [1, 3], [0, 2, 4], seed, sid=[10, 11, 12, 13])
    b, _ = TM.sample_two_hop(rowptr, col, [1], [0, 2], seed, sid=[11, 10], q0=99)
    assert a[:2].tolist() == b[::-1].tolist()


def test_mirror_layers_fallback_prefix_and_chunks():
    seed = 20250101
    name, n, rows, want = TM.hand_cases()[1]                                    # the star: the centre has no candidate
    rowptr, col = TM.csr_of(n, rows)
    src = np.array([1, 0, 2, 0], dtype=np.int64)
    hard = TM.two_hop_negative_targets(rowptr, col, n, src, 6, seed, fallback=None)
    both = TM.two_hop_negative_targets(rowptr, col, n, src, 6, seed)
    uni = SM.negative_targets(rowptr, col, n, src, 6, seed)
    assert (hard[[1, 3]] == -1).all() and (hard[[0, 2]] >= 1).all()
    assert np.array_equal(both[[0, 2]], hard[[0, 2]]) and np.array_equal(both[[1, 3]], uni[[1, 3]])
    # the centre is linked to every other node: the uniform sampler has nothing either, so -1 stays
    assert (both[[1, 3]] == -1).all()
    # on the path the end's only candidate is node 2 and nothing falls back
    name, n, rows, want = TM.hand_cases()[0]
    rowptr, col = TM.csr_of(n, rows)
    src = np.array([0, 2, 4, 2], dtype=np.int64)
    long = TM.two_hop_negative_targets(rowptr, col, n, src, 9, seed)
    assert (long[0] == 2).all() and (long[2] == 2).all() and set(long[1].tolist()) == {0, 4}
    assert np.array_equal(long[:, :4], TM.two_hop_negative_targets(rowptr, col, n, src, 4, seed))
    assert np.array_equal(long[1:], TM.two_hop_negative_targets(rowptr, col, n, src[1:], 9, seed, first=1))
    pos = np.array([[2, 0, 2, 2, 4], [1, 1, 3, 1, 3]], dtype=np.int64)
    e = TM.two_hop_negative_edges(rowptr, col, n, pos, seed)
    assert np.array_equal(e[0], pos[0]) and e[1, 1] == 2 and e[1, 4] == 2 and set(e[1, [0, 2, 3]].tolist()) <= {0, 4}
    assert np.array_equal(e[:, 2:], TM.two_hop_negative_edges(rowptr, col, n, pos[:, 2:], seed, first=2))
    # an isolated node falls back to the uniform sample of its own index
    rows6 = dict(rows)
    rowptr6, col6 = TM.csr_of(6, rows6)                                         # node 5: no neighbour
    pos = np.array([[5, 0, 5], [0, 1, 1]], dtype=np.int64)
    e = TM.two_hop_negative_edges(rowptr6, col6, 6, pos, seed, first=10)
    assert e[1, 0] == SM.negative_targets(rowptr6, col6, 6, [5], 1, seed, 10)[0, 0]
    assert e[1, 2] == SM.negative_targets(rowptr6, col6, 6, [5], 1, seed, 12)[0, 0] and e[1, 1] == 2
    assert TM.two_hop_negative_edges(rowptr6, col6, 6, pos, seed, first=10, fallback=None)[1].tolist() == [-1, 2, -1]
