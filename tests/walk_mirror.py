"""Exact reference of the walk-count route (ocn_hip.h: ocn_cn_walk_flags, ocn_walk_prep, ocn_cn_walk_group), in numpy int64,
written from the definition:

    for a candidate e = (i, j) and the p-th neighbour k of i:
        flag bit 1  iff k in N(j)                     (cn1)
        wc          =   |N(k) ∩ N(j)|                  (the 2-walks j -> m -> k)
        flag bit 2  iff wc > 0                        (cn2)

No Bloom bitmap, no hash table, no work items: a sorted-row membership test per swept element.  ``bloom_only`` turns the
membership test into "shares a Bloom bit with a member" through the LIBRARY's hash (``ocn_walk_hash``) — what a sweep that took
the bitmap's "maybe" for "member" would report.  It exists to prove that a constructed case can tell the two apart, nothing else.
"""
from collections import namedtuple

import numpy as np

Walk = namedtuple("Walk", "off flags wc cnt1 cnt2 hist")

N_BIG = 512          # ocn_hip.h, ocn_walk_prep: a target with more neighbours keeps its own sweep
N_GROUP = 64         # ... runs of equal sources are cut into pieces of 64
N_KEYS = 4096        # ... whose small targets' rows sum to at most 4096 entries


class Graph:
    """A symmetric simple graph put together edge by edge; ``csr()`` = (rowptr int64 [n + 1], col int32, rows sorted)."""

    def __init__(self, n):
        self.n = int(n)
        self.u, self.v = [], []

    def add(self, u, vs):
        vs = np.atleast_1d(np.asarray(vs, dtype=np.int64))
        assert 0 <= u < self.n and (vs >= 0).all() and (vs < self.n).all() and (vs != u).all()
        self.u.append(np.full(vs.size, u, dtype=np.int64))
        self.v.append(vs)

    def csr(self):
        u = np.concatenate(self.u + self.v) if self.u else np.zeros(0, np.int64)
        v = np.concatenate(self.v + self.u) if self.u else np.zeros(0, np.int64)
        key = np.unique(u * self.n + v)
        row, col = key // self.n, key % self.n
        rowptr = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(np.bincount(row, minlength=self.n), out=rowptr[1:])
        return rowptr, col.astype(np.int32)


def row(rowptr, col, v):
    return col[rowptr[v]:rowptr[v + 1]].astype(np.int64)


def degrees(rowptr):
    return np.diff(rowptr)


def neighbor_degree_sum(rowptr, col):
    """nds[v] = Σ_{u in N(v)} deg(u)."""
    deg = degrees(rowptr)
    out = np.zeros(rowptr.size - 1, dtype=np.int64)
    np.add.at(out, np.repeat(np.arange(rowptr.size - 1), deg), deg[col])
    return out


def hash_table(lib, which, n):
    """ocn_walk_hash(which, v) for v in 0 .. n - 1."""
    return np.fromiter((lib.ocn_walk_hash(which, v) for v in range(n)), dtype=np.int64, count=n)


def _member(sorted_row, elems):
    if sorted_row.size == 0:
        return np.zeros(elems.size, dtype=bool)
    pos = np.minimum(np.searchsorted(sorted_row, elems), sorted_row.size - 1)
    return sorted_row[pos] == elems


def _maybe(bits, sorted_row, elems):
    """elems share a Bloom bit with a member of the row"""
    return np.isin(bits[elems], bits[sorted_row])


def mirror(rowptr, col, src, dst, bloom_only=None, side="fwd", bits=None):
    """``Walk`` of the batch.  ``bloom_only`` = 0 / 1 with ``bits`` = ``hash_table(lib, bloom_only, n)``: membership in the probed
    row is replaced by a shared Bloom bit with one of its members, in the cn1 test and in the sweep.  ``side`` = "fwd": the
    elements of the rows N(k), k in N(i), are probed against N(j); "rev": the elements k' of the rows N(m), m in N(j), are
    probed against N(i), and a "maybe" that is no member is credited to the position a search without its final equality
    test would return."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    n, B = rowptr.size - 1, src.size
    deg = degrees(rowptr)
    off = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(deg[src], out=off[1:])
    flags = np.zeros(off[B], dtype=np.uint8)
    wc = np.zeros(off[B], dtype=np.int32)
    cnt1, cnt2 = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    swept = {}                                 # node -> (elements of the rows of its neighbours, the neighbour's position)
    for e in range(B):
        i, j = int(src[e]), int(dst[e])
        ni, nj = row(rowptr, col, i), row(rowptr, col, j)
        test = _member if bloom_only is None else (lambda r, x: _maybe(bits, r, x))
        f1 = test(nj, ni)
        sweeper = i if side == "fwd" or bloom_only is None else j
        if sweeper not in swept:
            ns = row(rowptr, col, sweeper)
            swept[sweeper] = (np.concatenate([row(rowptr, col, k) for k in ns]) if ns.size else np.zeros(0, np.int64),
                              np.repeat(np.arange(ns.size), deg[ns]))
        elems, pos = swept[sweeper]
        if sweeper == i:
            w = np.bincount(pos[test(nj, elems)], minlength=ni.size)
        else:
            hit = test(ni, elems)
            where = np.minimum(np.searchsorted(ni, elems[hit]), max(ni.size - 1, 0))
            w = np.bincount(where, minlength=ni.size) if ni.size else np.zeros(0, np.int64)
        f2 = w > 0
        flags[off[e]:off[e + 1]] = f1.astype(np.uint8) | (f2.astype(np.uint8) << 1)
        wc[off[e]:off[e + 1]] = w
        cnt1[e], cnt2[e] = f1.sum(), f2.sum()
    return Walk(off, flags, wc, cnt1, cnt2, hist_of(rowptr, col, src, flags, wc))


def hist_of(rowptr, col, src, flags, wc):
    """The four columns ``ops.hist_counts`` returns — n1, n2, n_union, Σ walks per node — of a batch's flags and walk counts."""
    n = rowptr.size - 1
    src = np.asarray(src, dtype=np.int64)
    deg = degrees(rowptr)[src]
    start = np.repeat(rowptr[src] - np.concatenate([[0], np.cumsum(deg)[:-1]]), deg)
    k = col[start + np.arange(deg.sum())].astype(np.int64) if deg.sum() else np.zeros(0, np.int64)
    f = flags[:k.size].astype(np.int64)
    return np.stack([np.bincount(k, weights=x, minlength=n).astype(np.int64)
                     for x in (f & 1, (f >> 1) & 1, (f != 0).astype(np.int64), wc[:k.size].astype(np.int64))], axis=1)


def prefix(w, rowptr, col, src, B):
    """The ``Walk`` of the batch's first ``B`` candidates."""
    t = int(w.off[B])
    return Walk(w.off[:B + 1], w.flags[:t], w.wc[:t], w.cnt1[:B], w.cnt2[:B],
                hist_of(rowptr, col, np.asarray(src)[:B], w.flags[:t], w.wc[:t]))


def groups_of(order, src):
    """g_head of a processing order in which equal sources are contiguous: every run cut into pieces of 64."""
    s = np.asarray(src)[np.asarray(order)]
    head, run = [], 0
    for p in range(s.size):
        run = 0 if p == 0 or s[p] != s[p - 1] else run + 1
        if run % N_GROUP == 0:
            head.append(p)
    return np.asarray(head + [s.size], dtype=np.int64)


def shared_rule(rowptr, src, dst, order, min_share):
    """The documented rule of ocn_walk_prep without ``nds``: (g_head, g_active).  A slot goes to the shared sweep iff its
    target has at most 512 neighbours and its group — a run of equal sources cut into pieces of 64 — has at least ``min_share``
    such members whose target degrees sum to at most 4096."""
    order = np.asarray(order)
    dj = degrees(rowptr)[np.asarray(dst)[order]]
    head = groups_of(order, src)
    active = np.zeros(order.size, dtype=np.int32)
    for g in range(head.size - 1):
        sl = slice(head[g], head[g + 1])
        small = dj[sl] <= N_BIG
        if small.sum() >= min_share and dj[sl][small].sum() <= N_KEYS:
            active[sl] = small
    return head, active
