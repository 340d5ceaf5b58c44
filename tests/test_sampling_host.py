"""Structured negative sampling (``ocn_philox4x32``, ``ocn_complement_count``, ``ocn_sample_complement_rows`` / ``_pairs``,
ocn_amd/sampling.py) without a GPU: the entries' argument checks, the CPU mirror the GPU tests compare against (its generator
against the published known answers, its selection against brute-force enumeration, its uniformity), and the refusals of the
Python layers."""
import math
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from ocn_amd import _lib
from tests import sampling_mirror as SM

P = c_void_p(4096)             # a non-NULL, 16-byte aligned address that is never read: every call below returns before its first HIP call
Z = c_void_p(0)
ENTRIES = ("ocn_philox4x32", "ocn_complement_count", "ocn_sample_stage_cols", "ocn_sample_complement_rows",
           "ocn_sample_complement_pairs")


def test_sampling_entries_are_additions_to_abi_9(hiplib):
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(hiplib, name)
    assert hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9
    assert hiplib.ocn_sample_stage_cols() >= 64


def _philox(lib, **kw):
    a = dict(ctr=P, k0=1, k1=2, n=4, out=P)
    a.update(kw)
    return lib.ocn_philox4x32(a["ctr"], a["k0"], a["k1"], a["n"], a["out"], Z)


def _count(lib, **kw):
    a = dict(rp=P, col=P, n=100, count=P)
    a.update(kw)
    return lib.ocn_complement_count(a["rp"], a["col"], a["n"], a["count"], Z)


def _rows(lib, **kw):
    a = dict(rp=P, col=P, n=100, rows=P, Q=4, per=3, q0=0, seed=7, out=P)
    a.update(kw)
    return lib.ocn_sample_complement_rows(a["rp"], a["col"], a["n"], a["rows"], a["Q"], a["per"], a["q0"], a["seed"], a["out"], Z)


def _pairs(lib, **kw):
    a = dict(rp=P, col=P, n=100, cptr=P, T=4, t0=0, seed=7, out=P)
    a.update(kw)
    return lib.ocn_sample_complement_pairs(a["rp"], a["col"], a["n"], a["cptr"], a["T"], a["t0"], a["seed"], a["out"], Z)


def test_sampling_entries_reject_bad_arguments_before_any_hip_call(hiplib):
    for call, pointers in ((_philox, ("ctr", "out")), (_count, ("rp", "col", "count")),
                           (_rows, ("rp", "col", "rows", "out")), (_pairs, ("rp", "col", "cptr", "out"))):
        for name in pointers:
            assert call(hiplib, **{name: Z}) == -1, (call.__name__, name)
    assert _philox(hiplib, n=-1) == -1 and _rows(hiplib, Q=-1) == -1 and _pairs(hiplib, T=-1) == -1
    assert _rows(hiplib, q0=-1) == -1 and _pairs(hiplib, t0=-1) == -1
    for call in (_count, _rows, _pairs):
        for n in (0, -5, 1 << 31, 1 << 40):
            assert call(hiplib, n=n) == -1, (call.__name__, n)
    for per in (0, -1, 1 << 31, 1 << 40):
        assert _rows(hiplib, per=per) == -1, per
    # an empty call is still checked ...
    assert _philox(hiplib, n=0, ctr=Z) == -1 and _philox(hiplib, n=0, out=Z) == -1
    assert _rows(hiplib, Q=0, rows=Z) == -1 and _rows(hiplib, Q=0, n=0) == -1 and _rows(hiplib, Q=0, per=0) == -1
    assert _rows(hiplib, Q=0, per=1 << 31) == -1 and _rows(hiplib, Q=0, n=1 << 31) == -1
    assert _pairs(hiplib, T=0, cptr=Z) == -1 and _pairs(hiplib, T=0, n=0) == -1 and _pairs(hiplib, T=0, n=1 << 31) == -1
    # ... and a valid one launches nothing
    assert _philox(hiplib, n=0) == 0
    assert _rows(hiplib, Q=0) == 0 and _rows(hiplib, Q=0, n=(1 << 31) - 1, per=(1 << 31) - 1, q0=1 << 40, seed=(1 << 64) - 1) == 0
    assert _pairs(hiplib, T=0) == 0 and _pairs(hiplib, T=0, n=(1 << 31) - 1, t0=1 << 40, seed=(1 << 64) - 1) == 0


def test_mirror_generator_gives_the_known_answers():
    for ctr, key, want in SM.KNOWN_ANSWERS:
        assert SM.philox4x32(ctr, key) == want
        got = SM.philox4x32_np(np.array([ctr], dtype=np.uint32), key)
        assert tuple(int(v) for v in got[0]) == want
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 1 << 32, size=(50, 4), dtype=np.uint64).astype(np.uint32)
    got = SM.philox4x32_np(ctr, (0x12345678, 0x9ABCDEF0))
    for i in range(50):
        assert tuple(int(v) for v in got[i]) == SM.philox4x32(ctr[i], (0x12345678, 0x9ABCDEF0))
    assert SM.mulhi((1 << 64) - 1, 7) == 6 and SM.mulhi(0, 7) == 0 and SM.mulhi(1 << 63, 7) == 3
    assert SM.mulhi((1 << 64) - 1, (1 << 63) + 5) == (1 << 63) + 4
    assert SM.key_of((0xDEADBEEF << 32) | 0x01234567) == (0x01234567, 0xDEADBEEF)


def _brute(row_cols, s, n):
    ex = set(int(c) for c in row_cols) | {s}
    return [c for c in range(n) if c not in ex]


def _special_rows(n):
    """(row columns, source) cases: empty row, full row, stored self-loop, excluded runs that touch column 0 and column n - 1."""
    yield [], 0
    yield [], n - 1
    yield [], n // 2
    yield list(range(n)), 3                                  # full row (stores its source): nothing left
    yield [c for c in range(n) if c != 3], 3                 # adjacent to every other node: nothing left
    yield [2, 5, 7], 5                                       # stored self-loop
    yield [0, 1, 2], 3                                       # run from column 0, the source extends it
    yield [0, 1, 2, 9], 0
    yield list(range(n - 4, n)), n - 5                       # run up to column n - 1, the source extends it
    yield list(range(n - 4, n)), n - 1
    yield [0, n - 1], n // 2
    yield [1], 0
    yield [n - 2], n - 1


def test_mirror_select_equals_brute_force_enumeration():
    rng = np.random.default_rng(11)
    cases = []
    for n in (1, 2, 3, 17, 40):
        for _ in range(60):
            d = int(rng.integers(0, n + 1))
            cases.append((n, sorted(rng.choice(n, size=d, replace=False).tolist()), int(rng.integers(0, n))))
    cases += [(40, cols, s) for cols, s in _special_rows(40)] + [(12, cols, s) for cols, s in _special_rows(12)]
    empties = 0
    for n, cols, s in cases:
        xs = SM.excluded(cols, s)
        want = _brute(cols, s, n)
        assert n - len(xs) == len(want)
        assert [SM.select(xs, r) for r in range(len(want))] == want, (n, cols, s)
        empties += not want
    assert empties >= 4
    # through the sampler: a CSR of these rows, every sample a member of its row's complement, -1 where there is none
    n = 40
    rows40 = [(cols, s) for nn, cols, s in cases if nn == n]
    by_source = {}
    for cols, s in rows40:
        by_source.setdefault(s, cols)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    for s in range(n):
        rowptr[s + 1] = rowptr[s] + len(by_source.get(s, []))
    col = np.array([c for s in range(n) for c in by_source.get(s, [])], dtype=np.int32)
    src = sorted(by_source)
    out = SM.negative_targets(rowptr, col, n, src, 9, seed=3)
    for q, s in enumerate(src):
        comp = _brute(by_source[s], s, n)
        assert all(int(v) in comp for v in out[q]) if comp else (out[q] == -1).all()
    cptr = SM.complement_ptr(rowptr, col, n)
    pairs = SM.negative_edges(rowptr, col, n, 300, seed=4, cptr=cptr)
    for s, c in pairs.T.tolist():
        assert c in _brute(by_source.get(s, []), s, n)


def test_mirror_draws_are_uniform_over_the_complement():
    """One row whose complement has m = 7 members, S = 70 000 draws, a fixed seed: every member's count within 5 sqrt(S / m)
    of S / m — five standard deviations (of the Poisson approximation, which exceeds the binomial's) on a deterministic
    sequence."""
    n, s = 12, 4
    cols = [0, 3, 8, 11]                                     # excluded: {0, 3, 4, 8, 11}; complement {1, 2, 5, 6, 7, 9, 10}
    comp = _brute(cols, s, n)
    m, S = len(comp), 70_000
    assert m == 7
    ctr = np.zeros((S, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(S)
    ctr[:, 3] = 2                                            # query 0 of the per-source stream
    w = SM.philox4x32_np(ctr, SM.key_of(20240607))
    xs = SM.excluded(cols, s)
    counts = dict.fromkeys(comp, 0)
    for a, b in zip(w[:, 0].tolist(), w[:, 1].tolist()):
        counts[SM.select(xs, SM.mulhi(a | (b << 32), m))] += 1
    assert sum(counts.values()) == S
    bound = 5 * math.sqrt(S / m)
    for c, k in counts.items():
        assert abs(k - S / m) <= bound, (c, k)
    # the vectorised path above is the sampler's: spot-check it against the per-sample mirror
    got = SM.negative_targets(np.array([0] * (s + 1) + [len(cols)] * (n - s), dtype=np.int64), np.array(cols, dtype=np.int32), n,
                              [s], 40, seed=20240607)
    assert got[0].tolist() == [SM.select(xs, SM.mulhi(int(w[j, 0]) | (int(w[j, 1]) << 32), m)) for j in range(40)]


def _tiny():
    from ocn_amd.sparse import SparseTensor
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(4, 4))
    wide = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(4, 5))
    return adj, wide


def test_samplers_refuse_a_non_square_known(hiplib):
    from ocn_amd import sampling as S
    _, wide = _tiny()
    src = torch.tensor([0, 2])
    for call in (lambda: S.negative_targets(wide, src, 3, 1), lambda: S.negative_edges(wide, 3, 1), lambda: S.complement_ptr(wide)):
        with pytest.raises(ValueError, match="square known matrix"):
            call()


def test_negative_targets_refuses_sources_that_are_not_int64(hiplib):
    from ocn_amd import sampling as S
    adj, _ = _tiny()
    for bad in (torch.tensor([0, 2], dtype=torch.int32), torch.tensor([[0, 2]]), [0, 2]):
        with pytest.raises(ValueError, match="sources must be a 1-d int64"):
            S.negative_targets(adj, bad, 3, 1)


def test_negative_targets_refuses_per_below_one(hiplib):
    from ocn_amd import sampling as S
    adj, _ = _tiny()
    for per in (0, -3):
        with pytest.raises(ValueError, match="per must be at least 1"):
            S.negative_targets(adj, torch.tensor([0, 2]), per, 1)


def test_negative_edges_refuses_a_negative_num(hiplib):
    from ocn_amd import sampling as S
    adj, _ = _tiny()
    with pytest.raises(ValueError, match="num must not be negative"):
        S.negative_edges(adj, -1, 1)


def test_samplers_have_no_cpu_path(hiplib):
    from ocn_amd import ops, sampling as S
    adj, _ = _tiny()
    src = torch.tensor([0, 2])
    for call in (lambda: S.negative_targets(adj, src, 3, 1),
                 lambda: S.negative_edges(adj, 3, 1),
                 lambda: S.complement_ptr(adj),
                 lambda: ops.complement_count(adj._rowptr, adj._col),
                 lambda: ops.sample_complement_rows(adj._rowptr, adj._col, src, 3, 1),
                 lambda: ops.sample_complement_pairs(adj._rowptr, adj._col, torch.tensor([0, 2, 3, 5, 8]), 3, 1),
                 lambda: ops.philox4x32(torch.zeros(2, 4, dtype=torch.int32), 0, 0)):
        with pytest.raises(_lib.OcnHipError, match="no CPU path"):
            call()


def test_sampling_op_wrappers_check_their_arguments_before_the_library(hiplib, monkeypatch):
    from ocn_amd import ops
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    monkeypatch.setattr(ops, "validate_indices", False)
    rp, col, rows = torch.tensor([0, 1, 2, 2]), torch.tensor([1, 0], dtype=torch.int32), torch.tensor([0, 1])
    for per in (0, 1 << 31):
        with pytest.raises(ValueError, match="per must be in 1"):
            ops.sample_complement_rows(rp, col, rows, per, 1)
    with pytest.raises(ValueError, match="first must not be negative"):
        ops.sample_complement_rows(rp, col, rows, 3, 1, first=-1)
    for seed in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed must be in 0"):
            ops.sample_complement_rows(rp, col, rows, 3, seed)
        with pytest.raises(ValueError, match="seed must be in 0"):
            ops.sample_complement_pairs(rp, col, torch.tensor([0, 2, 4, 6]), 3, seed)
    with pytest.raises(ValueError, match="cptr: one entry per row and the total"):
        ops.sample_complement_pairs(rp, col, torch.tensor([0, 2, 4]), 3, 1)
    with pytest.raises(ValueError, match="known has 0 rows"):
        ops.complement_count(torch.tensor([0]), col)
    with pytest.raises(ValueError, match=r"ctr: expected \[n, 4\]"):
        ops.philox4x32(torch.zeros(2, 3, dtype=torch.int32), 0, 0)
    with pytest.raises(ValueError, match="key words must be in 0"):
        ops.philox4x32(torch.zeros(2, 4, dtype=torch.int32), 1 << 32, 0)
