"""CPU mirror of the 2-hop hard-negative sampler (include/ocn_hip.h: ocn_sample_two_hop; ocn_amd/sampling.py:
two_hop_negative_targets, two_hop_negative_edges) in plain Python: the candidate set as a Python set, the selection as
``sorted(H)[r]``, the generator of tests/sampling_mirror.py with the two new counter streams — written from the contract, not
from the kernel, and slow on purpose."""
import numpy as np

from tests.sampling_mirror import MASK32, key_of, mulhi, philox4x32
from tests import sampling_mirror as SM

STREAM_SLOT, STREAM_ID = 3, 4


def csr_of(n: int, rows):
    """``rows``: {row id: ascending columns} -> (rowptr int64 [n + 1], col int32)."""
    rowptr = np.zeros(n + 1, dtype=np.int64)
    for s in range(n):
        rowptr[s + 1] = rowptr[s] + len(rows.get(s, ()))
    return rowptr, np.array([c for s in range(n) for c in rows.get(s, ())], dtype=np.int32)


def undirected(n: int, pairs):
    """The symmetric adjacency rows of an undirected edge list."""
    rows = {}
    for a, b in pairs:
        rows.setdefault(a, set()).add(b)
        rows.setdefault(b, set()).add(a)
    return {s: sorted(v) for s, v in rows.items()}


def hand_cases():
    """(name, n, rows, {source: its candidate list}) of graphs whose 2-hop sets are known by inspection."""
    path = undirected(5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    star = undirected(6, [(0, leaf) for leaf in range(1, 6)])
    k34 = undirected(7, [(a, b) for a in range(3) for b in range(3, 7)])
    return (("path", 5, path, {0: [2], 1: [3], 2: [0, 4], 3: [1], 4: [2]}),
            ("star", 6, star, {0: [], 1: [2, 3, 4, 5], 3: [1, 2, 4, 5], 5: [1, 2, 3, 4]}),
            ("k34", 7, k34, {0: [1, 2], 1: [0, 2], 2: [0, 1], 3: [4, 5, 6], 6: [3, 4, 5]}))


def row(rowptr, col, s: int):
    return [int(c) for c in col[rowptr[s]:rowptr[s + 1]]]


def candidates(a_rowptr, a_col, s: int, m_rowptr=None, m_col=None, drop_self: bool = True):
    """H(s) = (U_{m in A[s,:]} A[m,:]) \\ M[s,:], without s under drop_self, ascending.  M defaults to A."""
    m_rowptr, m_col = (a_rowptr, a_col) if m_rowptr is None else (m_rowptr, m_col)
    h = set()
    for m in row(a_rowptr, a_col, s):
        h.update(row(a_rowptr, a_col, m))
    h -= set(row(m_rowptr, m_col, s))
    if drop_self:
        h.discard(int(s))
    return sorted(h)


def rank_slot(seed: int, q: int, j: int, c: int) -> int:
    """Slot j of query q (absolute: q0 + q), without sample ids."""
    w = philox4x32((j & MASK32, q & MASK32, q >> 32, STREAM_SLOT), key_of(seed))
    return mulhi(w[0] | (w[1] << 32), c)


def rank_id(seed: int, sid: int, c: int) -> int:
    """A slot that carries the sample id sid."""
    w = philox4x32((sid & MASK32, sid >> 32, 0, STREAM_ID), key_of(seed))
    return mulhi(w[0] | (w[1] << 32), c)


def sample_two_hop(a_rowptr, a_col, rows, sptr, seed: int, sid=None, q0: int = 0, m_rowptr=None, m_col=None,
                   drop_self: bool = True):
    """Mirror of the entry: (out int64 [sptr[-1]], count int64 [Q])."""
    out = np.full(int(sptr[-1]), -1, dtype=np.int64)
    count = np.zeros(len(rows), dtype=np.int64)
    memo = {}
    for q, s in enumerate(int(v) for v in rows):
        if s not in memo:
            memo[s] = candidates(a_rowptr, a_col, s, m_rowptr, m_col, drop_self)
        h = memo[s]
        count[q] = len(h)
        if not h:
            continue
        for i in range(int(sptr[q]), int(sptr[q + 1])):
            r = rank_slot(seed, q0 + q, i - int(sptr[q]), len(h)) if sid is None else rank_id(seed, int(sid[i]), len(h))
            out[i] = h[r]
    return out, count


def two_hop_negative_targets(a_rowptr, a_col, n: int, sources, per: int, seed: int, m_rowptr=None, m_col=None, first: int = 0,
                             fallback="uniform") -> np.ndarray:
    """Mirror of ocn_amd.sampling.two_hop_negative_targets on CSRs given as numpy arrays: int64 [Q, per]."""
    sptr = np.arange(len(sources) + 1, dtype=np.int64) * per
    out, count = sample_two_hop(a_rowptr, a_col, sources, sptr, seed, q0=first, m_rowptr=m_rowptr, m_col=m_col)
    out = out.reshape(len(sources), per)
    if fallback == "uniform":
        k_rowptr, k_col = (a_rowptr, a_col) if m_rowptr is None else (m_rowptr, m_col)
        for q in np.flatnonzero(count == 0):
            out[q] = SM.negative_targets(k_rowptr, k_col, n, [sources[q]], per, seed, first + int(q))[0]
    return out


def two_hop_negative_edges(a_rowptr, a_col, n: int, pos_edges, seed: int, m_rowptr=None, m_col=None, first: int = 0,
                           fallback="uniform") -> np.ndarray:
    """Mirror of ocn_amd.sampling.two_hop_negative_edges, positive by positive: int64 [2, E]."""
    src = [int(v) for v in pos_edges[0]]
    k_rowptr, k_col = (a_rowptr, a_col) if m_rowptr is None else (m_rowptr, m_col)
    out = np.full((2, len(src)), -1, dtype=np.int64)
    memo = {}
    for t, s in enumerate(src):
        if s not in memo:
            memo[s] = candidates(a_rowptr, a_col, s, m_rowptr, m_col)
        h = memo[s]
        out[0, t] = s
        if h:
            out[1, t] = h[rank_id(seed, first + t, len(h))]
        elif fallback == "uniform":
            out[1, t] = SM.negative_targets(k_rowptr, k_col, n, [s], 1, seed, first + t)[0, 0]
    return out
