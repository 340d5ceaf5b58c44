"""The constructed graphs and batches of the walk route's edge tests (tests/test_walk_edges_host.py asserts their premises,
tests/test_walk_edges_gpu.py runs them).  Every builder returns a ``Case``: the CSR of a symmetric graph, a candidate batch and
``info`` — what the case was built to contain, for the premise checks.  Node ids that must collide are found with the library's
own hashes (``ocn_walk_hash`` through ``walk_mirror.hash_table``), never with a copy of their constants."""
import functools
from collections import namedtuple

import numpy as np

from tests import walk_mirror as WM

Case = namedtuple("Case", "rowptr col src dst info")

SLOTS = 8192                     # slots of the shared sweep's key table and of the prep's source table (ocn_hip.h: ocn_walk_hash)
ROUND = 8 * 512                  # elements a per-candidate work item sweeps between two looks at its hit queue
QUEUE = 1024                     # entries of that queue; it is resolved when more than half full


def _case(g, cands, **info):
    rowptr, col = g.csr()
    c = np.asarray(cands, dtype=np.int64).reshape(-1, 2)
    return Case(rowptr, col, c[:, 0].copy(), c[:, 1].copy(), info)


_tables = {}


def table(lib, which, n):
    if (which, n) not in _tables:
        _tables[which, n] = WM.hash_table(lib, which, n)
    return _tables[which, n]


def colliding_pairs(h, lo=1000):
    """[(a, b)] with lo <= a < b and h[a] == h[b]."""
    ids = np.arange(lo, h.size)
    o = ids[np.argsort(h[ids], kind="stable")]
    same = h[o[1:]] == h[o[:-1]]
    return np.stack([o[:-1][same], o[1:][same]], axis=1)


def occupied(keys, h2):
    """Slots that linear probing with wrap-around fills when the distinct ``keys`` are inserted (the set does not depend on the
    insertion order) and the slot every key ends up in, for insertion in ascending order."""
    slot_of, used = {}, set()
    for k in sorted(set(int(k) for k in keys)):
        s = int(h2[k])
        while s in used:
            s = (s + 1) % SLOTS
        used.add(s)
        slot_of[k] = s
    return used, slot_of


def probes(key, used, h2):
    """Slots a lookup of ``key`` (not stored) reads before it meets an empty one."""
    s, n = int(h2[key]), 0
    while s in used:
        s, n = (s + 1) % SLOTS, n + 1
    return n


# ---------------------------------------------------------------------------------------------------------------------------
# common.h's rules, restated for the item counts
# ---------------------------------------------------------------------------------------------------------------------------
def walk_group_rule(nds, i, di):
    chunks = (di + 63) // 64
    if nds is None or chunks <= 1:
        return 1
    cg = min(16384 // (int(nds[i]) // chunks + 1), 8)
    return 1 if cg < 1 else min(cg, chunks)


def walk_reverse_rule(nds, i, j, di, dj):
    if nds is None or di == 0 or dj == 0:
        return False
    return 2 * int(nds[j]) + di * ((dj + 15) // 16) + 2 * di < int(nds[i])


def item_counts(c, nds):
    """(forward items, reverse items) of a batch swept candidate by candidate."""
    deg = WM.degrees(c.rowptr)
    fwd = rev = 0
    for i, j in zip(c.src, c.dst):
        di, dj = int(deg[i]), int(deg[j])
        cg = walk_group_rule(nds, i, di)
        fwd += -(-((di + 63) // 64) // cg)
        rev += (dj + 15) // 16 if walk_reverse_rule(nds, i, j, di, dj) else 0
    return fwd, rev


def forced_reverse(c):
    """The doctored cost vector of test_walk_route_swept_from_either_endpoint: sources look expensive, targets free."""
    nds = np.zeros(c.rowptr.size - 1, dtype=np.int64)
    nds[c.src] = 1 << 50
    nds[c.dst] = 0
    nds[c.src[c.src == c.dst]] = 0
    return nds


# ---------------------------------------------------------------------------------------------------------------------------
# a fan: hubs over a pool of leaves that are chained among themselves (so that walk counts are not all zero)
# ---------------------------------------------------------------------------------------------------------------------------
class Fan:
    def __init__(self, n, pool0, pool_n, hub0=2):
        self.g = WM.Graph(n)
        self.pool = np.arange(pool0, pool0 + pool_n, dtype=np.int64)
        self.hub = hub0
        for step in (1, 3):                                             # leaf p - p + 1, p - p + 3
            self.g.u.append(self.pool[:-step])
            self.g.v.append(self.pool[:-step] + step)

    def node(self, neigh, at=None):
        if at is None:
            at, self.hub = self.hub, self.hub + 1
        assert at < self.pool[0] or at > self.pool[-1]
        if len(neigh):
            self.g.add(at, neigh)
        return at

    def source(self, d, shift=0, at=None):
        """every second leaf from ``shift`` on"""
        assert shift + 2 * d <= self.pool.size + 1
        return self.node(self.pool[shift:shift + 2 * d:2], at)

    def target(self, d, shift=0, at=None):
        """``d`` consecutive leaves from ``shift`` on"""
        assert shift + d <= self.pool.size
        return self.node(self.pool[shift:shift + d], at)


# ---------------------------------------------------------------------------------------------------------------------------
# per-candidate sweeps
# ---------------------------------------------------------------------------------------------------------------------------
KINDS = ("fwd", "rev", "f1")
WHERE = ("before", "between", "after")


@functools.lru_cache(maxsize=None)
def _bloom_case(lib, big):
    n, L = 100_000, (4097 if big else 3)
    h = table(lib, 0, n)
    pairs = colliding_pairs(h)
    room = L + 2000
    picked, reserved, pi = [], set(), 0
    for kind in KINDS:
        for where in WHERE:
            while True:
                a, b = (int(v) for v in pairs[pi])
                pi += 1
                if a in reserved or b in reserved:
                    continue
                if (where == "before" and b < n - room) or (where == "after" and a > 1000 + room) or \
                        (where == "between" and 1000 + room < a < n - room):
                    break
            reserved |= {a, b}
            picked.append((kind, where, a, b))

    def fresh(count, lo, hi):
        out = [v for v in range(lo, min(hi, lo + count + len(reserved))) if v not in reserved][:count]
        assert len(out) == count
        return out

    g, cands, gadgets = WM.Graph(n), [], []
    hubs = iter(range(2, 1000))
    for kind, where, a, b in picked:
        elem, member = (b, a) if where == "after" else (a, b)
        if where == "before":
            fill = fresh(L - 1, b + 1, n)
        elif where == "after":
            fill = fresh(L - 1, 1000, a)
        else:
            fill = fresh((L - 1) // 2, 1000, a) + fresh(L - 1 - (L - 1) // 2, a + 1, n)
        row = [member] + fill
        if kind == "fwd":          # i - k, k - {elem, member}; N(j) = row: the element swept from i's side is probed against N(j)
            i, k, j = next(hubs), next(hubs), next(hubs)
            g.add(i, [k]); g.add(k, [elem, member]); g.add(j, row)
            probed = j
        elif kind == "rev":        # j - m, m - {elem, member}; N(i) = row: the element swept from j's side is probed against N(i)
            i, j, m = next(hubs), next(hubs), next(hubs)
            g.add(j, [m]); g.add(m, [elem, member]); g.add(i, row)
            probed = i
        else:                      # the element is a neighbour k of i: the cn1 test of the finalise step against N(j)
            i, j = next(hubs), next(hubs)
            g.add(i, [elem, member]); g.add(j, row)
            probed = j
        gadgets.append(dict(kind=kind, where=where, e=len(cands), elem=elem, member=member, probed=probed))
        cands.append((i, j))
    return _case(g, cands, gadgets=gadgets, which=0, row_len=L)


def bloom_case(lib, big):
    """Nine candidates, one per (kind of false positive, place of the colliding key in the probed row); the probed rows have 3
    entries (searched in the LDS copy) or, ``big``, 4097 (searched in memory)."""
    return _bloom_case(lib, bool(big))


SRC_DEGS = (0, 1, 63, 64, 65, 511, 512, 513, 1025)
TGT_DEGS = (0, 1, 15, 16, 17, 33, 4095, 4096, 4097)


@functools.lru_cache(maxsize=None)
def sizes_case():
    """Every source row length against every probed row length, and the degenerate candidates: self-candidates, repeated
    candidates, isolated endpoints, candidates that are stored edges."""
    f = Fan(9000, 100, 8200)
    s = {d: f.source(d) for d in SRC_DEGS}
    t = {d: f.target(d, shift=5) for d in TGT_DEGS}
    cands = [(s[a], t[b]) for a in SRC_DEGS for b in TGT_DEGS]
    p = f.pool
    own = [f.source(65, shift=1), f.target(17, shift=9), f.source(0)]      # (nodes that are nobody else's source or target)
    cands += [(v, v) for v in own] + [(s[64], t[33]), (s[64], t[33]), (s[0], t[0]), (s[65], int(p[0])), (int(p[8]), t[17]),
                                      (int(p[4]), int(p[5])), (int(p[7]), int(p[7]))]
    # swept from the target's side the probed row is the source's: 4095, 4096 (its LDS copy) and 4097 entries (in memory)
    cands += [(f.source(d, shift=d % 2), t[b]) for d, b in ((4095, 17), (4096, 33), (4097, 16))]
    return _case(f.g, cands, s=s, t=t)


@functools.lru_cache(maxsize=None)
def block_case():
    """i - X, X - Y complete, the target one of X: every element the sweep from i's side meets (Y and i itself, |Y| + 1 per
    row) is a neighbour of the target, so all 64 x 128 swept elements pass the bitmap and are hits: wc = |Y| + 1 everywhere, no
    cn1 entry.  Two rounds of 4096 passes each: the queue overflows and the rest resolves in place."""
    a, b = 64, 127
    g = WM.Graph(2000)
    X, Y = np.arange(100, 100 + a), np.arange(1000, 1000 + b)
    g.add(1, X)
    for x in X:
        g.add(int(x), Y)
    return _case(g, [(1, int(X[5])), (1, int(X[0])), (int(X[5]), 1)], walks=b + 1, rows=a)


@functools.lru_cache(maxsize=None)
def _flush_case(lib, n_pass):
    n = 4000
    h = table(lib, 0, n)
    i, j = 1, 2
    M = np.arange(10, 23)
    taken = set(h[M].tolist())
    assert int(h[i]) not in taken
    P = np.asarray([v for v in range(1000, n) if int(h[v]) not in taken][:79])
    ks = np.arange(100, 164)
    g = WM.Graph(n)
    g.add(i, ks)
    g.add(j, M)
    c = n_pass - 51 * 10
    assert 0 <= c <= 10
    for t, k in enumerate(ks):
        g.add(int(k), np.concatenate([M[:c], P[:79 - c]]) if t == 51 else np.concatenate([M[:10], P[:69]]))
    return _case(g, [(i, j)], n_pass=n_pass, which=0)


def flush_case(lib, n_pass):
    """One work item of 64 rows of 80 elements, 5120 > 4096 elements: its first round is not its last.  Of the first 4096
    elements exactly ``n_pass`` pass the bitmap (all of them members of N(j): the other elements share no bit with it)."""
    return _flush_case(lib, int(n_pass))


def first_round_passes(c, bits):
    """(Bloom passes among the first ROUND elements of the first candidate's sweep from its source's side, elements in all)"""
    i, j = int(c.src[0]), int(c.dst[0])
    ni = WM.row(c.rowptr, c.col, i)[:512]
    elems = np.concatenate([WM.row(c.rowptr, c.col, k) for k in ni])
    maybe = np.isin(bits[elems], bits[WM.row(c.rowptr, c.col, j)])
    return int(maybe[:ROUND].sum()), int(elems.size)


# ---------------------------------------------------------------------------------------------------------------------------
# prep and shared sweep
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_sizes_case():
    """4097 candidates over 40 sources and 60 small targets; the tests run its prefixes."""
    f = Fan(3000, 500, 400)
    s = [f.source(1 + (7 * q) % 70, shift=3 * q) for q in range(40)]
    t = [f.target((11 * q) % 41, shift=5 * q) for q in range(60)]
    r = np.random.RandomState(3)
    return _case(f.g, [(s[a], t[b]) for a, b in zip(r.randint(0, 40, 4097), r.randint(0, 60, 4097))])


@functools.lru_cache(maxsize=None)
def groups_case():
    """One batch with every group size and every sharing decision of the documented rule; ``info['groups']``: source ->
    (what the group is about, its candidates' targets in no particular order)."""
    f = Fan(8000, 1000, 4300)
    light = [f.target(q % 40, shift=13 * q) for q in range(80)]
    t512 = [f.target(512, shift=100 * q) for q in range(7)]
    t513 = [f.target(513, shift=77 * q) for q in range(2)]
    t511, t1, t2, t5, t7 = (f.target(d, shift=d) for d in (511, 1, 2, 5, 7))
    groups = {}
    for cnt, d in ((63, 63), (64, 64), (65, 65), (128, 20), (129, 30)):
        groups[f.source(d, shift=cnt)] = ("%d candidates, source row %d" % (cnt, d), [light[(3 * q) % 80] for q in range(cnt)])
    for q in range(50):
        groups[f.source(3 + q % 10, shift=2 * q)] = ("pair", [light[q], light[79 - q]])
    groups[f.source(9)] = ("one small", [t5, t513[0], t513[1]])
    groups[f.source(10)] = ("two small", [t5, t7, t513[0]])
    groups[f.source(11)] = ("three small", [t5, t7, t1])
    groups[f.source(12)] = ("keys 4096", t512 + [t511, t1])
    groups[f.source(13)] = ("keys 4097", t512 + [t511, t2])
    groups[f.source(14)] = ("mixed", [t512[0], t513[0], t5, t7])
    cands = [(s, j) for s, (_, ts) in groups.items() for j in ts]
    r = np.random.RandomState(5)
    cands = [cands[q] for q in r.permutation(len(cands))]
    return _case(f.g, cands, groups=groups)


@functools.lru_cache(maxsize=None)
def _group_bloom_case(lib, cluster):
    n = 140_000
    h1, h2 = table(lib, 1, n), table(lib, 2, n)
    by_slot = {}
    for v in range(1000, n):
        by_slot.setdefault(int(h2[v]), []).append(v)
    for m, x in colliding_pairs(h1):
        m, x = int(m), int(x)
        s = int(h2[m])
        if not 10 < s < SLOTS - 10 or abs(int(h2[x]) - s) < 8:
            continue
        near = [[v for v in by_slot.get(s + d, []) if v not in (m, x)] for d in range(3)]
        if all(near):
            break
    i, k, j1, j2 = 2, 3, 4, 5
    fill = [v for v in range(1000, n) if abs(int(h2[v]) - s) > 8 and h1[v] != h1[m]][:2]
    g = WM.Graph(n)
    g.add(i, [k])
    g.add(k, [m, x])
    g.add(j1, [x, fill[0]])
    g.add(j2, [v[0] for v in near] if cluster else [fill[1]])
    return _case(g, [(i, j1), (i, j2)], elem=m, member=x, which=1)


def group_bloom_case(lib, cluster):
    """Two candidates of one source, swept together.  The swept element ``elem`` shares its bit of the shared sweep's bitmap with
    the key ``member`` and is no key itself; its home slot is empty, or (``cluster``) holds the first of three other keys in a
    row, which the lookup has to walk past."""
    return _group_bloom_case(lib, bool(cluster))


def group_keys(c):
    """the keys of the shared sweep's table when all candidates of the case share one group: the members of the targets' rows"""
    return sorted(set(int(v) for j in c.dst for v in WM.row(c.rowptr, c.col, j)))


@functools.lru_cache(maxsize=None)
def wrap_sweep_case(lib):
    """The targets' rows hold three ids of slot 8191 and one each of slots 8189 and 8190: the cluster runs 8189, 8190, 8191, 0,
    1, and two of the three are displaced across the wrap.  All three are swept (true keys that must be found), and so is
    ``elem``: no key, home slot inside the cluster, past the bitmap by a shared bit with the key ``member``."""
    n = 140_000
    h1, h2 = table(lib, 1, n), table(lib, 2, n)
    last = [int(v) for v in np.flatnonzero(h2 == SLOTS - 1) if v >= 1000][:3]
    d, e = (int(next(v for v in np.flatnonzero(h2 == s) if v >= 1000)) for s in (SLOTS - 2, SLOTS - 3))
    core = set(last + [d, e])
    z = y = None
    for v in np.flatnonzero(h2 >= SLOTS - 3):          # an id of the cluster's slots with a partner under the bitmap's hash
        partners = [int(w) for w in np.flatnonzero(h1 == h1[v]) if w != v and w >= 1000 and 8 < h2[w] < SLOTS - 8]
        if v >= 1000 and int(v) not in core and partners:
            z, y = int(v), partners[0]
            break
    a, b, c = last
    i, k1, k2, j1, j2 = 2, 3, 4, 5, 6
    g = WM.Graph(n)
    g.add(i, [k1, k2])
    g.add(k1, [a, b, c, z])
    g.add(k2, [c, d, e])
    g.add(j1, [a, b, e])
    g.add(j2, [c, d, y, b])
    return _case(g, [(i, j1), (i, j2), (i, j1)], elem=z, member=y, which=1, displaced=last)


@functools.lru_cache(maxsize=None)
def wrap_prep_case(lib):
    """Seven distinct sources with two candidates each: three of slot 8191 of the prep's source table, one of slot 8190, two of
    slot 0 and one of slot 1, so the table's cluster runs across 8191 -> 0 whatever order the atomics insert them in."""
    n = 60_000
    h2 = table(lib, 2, n)
    ids = []
    for slot, count in ((SLOTS - 1, 3), (SLOTS - 2, 1), (0, 2), (1, 1)):
        ids += [int(v) for v in np.flatnonzero(h2 == slot) if v >= 1000][:count]
    f = Fan(n, 100, 400)
    t = [f.target(3 + q, shift=9 * q) for q in range(6)]
    for q, v in enumerate(ids):
        f.source(5 + 9 * q, shift=q, at=v)
    cands = [(v, t[(q + r) % 6]) for r in (0, 3) for q, v in enumerate(ids)]
    return _case(f.g, cands, sources=ids)


@functools.lru_cache(maxsize=None)
def cpi_case(n_hubs):
    """``n_hubs`` sources of 4096 leaves of their own, two candidates each, and one source of 778 neighbours (13 chunks of 64: no
    multiple of any chunks-per-item above 1) — n_hubs * 64 + 13 chunks in the shared sweep."""
    leaves0, per = 1000, 4096
    nl = n_hubs * per + 778
    n = leaves0 + nl + 2 * n_hubs + 10
    g = WM.Graph(n)
    leaf = np.arange(leaves0, leaves0 + nl, dtype=np.int64)
    g.u.append(leaf[:-1]); g.v.append(leaf[1:])                     # the leaves in one chain
    tid = leaves0 + nl
    cands = []
    for q in range(n_hubs + 1):
        hub = 2 + q
        mine = leaf[q * per:(q + 1) * per] if q < n_hubs else leaf[n_hubs * per:]
        g.add(hub, mine)
        for r in range(2):
            g.add(tid, [int(mine[(37 * q + 101 * r) % mine.size]), int(mine[-1 - r]), int(leaf[(q * 53 + r) % nl])])
            cands.append((hub, tid))
            tid += 1
    return _case(g, cands, chunks=n_hubs * 64 + 13)


@functools.lru_cache(maxsize=None)
def cost_case():
    """A source of 256 neighbours with 401 neighbours each (a sweep from its side reads ~100 000 elements) and light targets (5
    leaves: a sweep from their side reads ~1 300).  ``info['many']`` = 192 candidates, ``info['two']`` = 2."""
    g = WM.Graph(3000)
    h, mids, leaves = 2, np.arange(100, 356), np.arange(1000, 1400)
    g.add(h, mids)
    for m in mids:
        g.add(int(m), leaves)
    for q in range(192):
        g.add(2000 + q, leaves[(np.arange(5) * 7 + q) % 400])
    return _case(g, [(h, 2000 + q) for q in range(192)], many=192, two=2)
