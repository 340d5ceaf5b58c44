"""CPU mirror of the random-walk retrieval (include/ocn_hip.h: ocn_rw_visits_count / _fill; ocn_amd/recommend.py:
random_walk_candidates, random_walk_short_list) in plain Python and numpy: the walks one by one, the visits as dicts, the order
by ``sorted()`` — written from the contract, not from the kernel.  Only the Philox blocks are vectorised
(``sampling_mirror.philox4x32_np``), so that a case of a few hundred thousand steps takes about a second."""
import numpy as np

from tests.sampling_mirror import MASK32, key_of, mulhi, philox4x32, philox4x32_np

STREAM_RW_A, STREAM_RW_B = 5, 6          # counter word 3: the block of u1 | u2, the block of u3


def words_one(seed: int, s: int, w: int, length: int):
    """(u1, u2[, u3]) of walk w of source s from the scalar generator — the reference of ``words`` below."""
    a = philox4x32((w, s & MASK32, s >> 32, STREAM_RW_A), key_of(seed))
    u = [a[0] | (a[1] << 32), a[2] | (a[3] << 32)]
    if length == 3:
        b = philox4x32((w, s & MASK32, s >> 32, STREAM_RW_B), key_of(seed))
        u.append(b[0] | (b[1] << 32))
    return tuple(u)


def words(seed: int, s: int, walks: int, length: int):
    """The random words of the walks 0 .. walks - 1 of source s: a list of tuples of Python integers."""
    ctr = np.empty((walks, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(walks, dtype=np.uint32)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = s & MASK32, s >> 32, STREAM_RW_A
    a = philox4x32_np(ctr, key_of(seed)).astype(np.uint64).tolist()
    out = [[r[0] | (r[1] << 32), r[2] | (r[3] << 32)] for r in a]
    if length == 3:
        ctr[:, 3] = STREAM_RW_B
        b = philox4x32_np(ctr, key_of(seed)).astype(np.uint64).tolist()
        for o, r in zip(out, b):
            o.append(r[0] | (r[1] << 32))
    return out


def raw_counts(rowptr, col, s: int, walks: int, length: int, seed: int):
    """(c2, c3): {node: walks whose second / third step ends there}, before any exclusion."""
    assert length in (2, 3)
    rowptr = [int(v) for v in rowptr]
    col = [int(v) for v in col]
    c2, c3 = {}, {}
    for u in words(seed, int(s), walks, length):
        p = int(s)
        for t in range(1, length + 1):
            deg = rowptr[p + 1] - rowptr[p]
            if deg == 0:
                break
            p = col[rowptr[p] + mulhi(u[t - 1], deg)]
            if t == 2:
                c2[p] = c2.get(p, 0) + 1
            elif t == 3:
                c3[p] = c3.get(p, 0) + 1
    return c2, c3


def value(c2: int, c3: int, decay, length: int) -> np.float32:
    """float32(c2) + float32(decay) * float32(c3): one rounded product, one rounded add."""
    if length == 2:
        return np.float32(c2)
    return np.float32(np.float32(c2) + np.float32(np.float32(decay) * np.float32(c3)))


def source_segment(rowptr, col, s: int, walks: int, length: int, seed: int, decay=None, m_rowptr=None, m_col=None):
    """[(v, c2, c3, val)] of one source, ascending v: every visited node that is neither s nor in row s of M (A by default)."""
    m_rowptr, m_col = (rowptr, col) if m_rowptr is None else (m_rowptr, m_col)
    c2, c3 = raw_counts(rowptr, col, s, walks, length, seed)
    drop = set(int(c) for c in m_col[int(m_rowptr[s]):int(m_rowptr[s + 1])]) | {int(s)}
    return [(v, c2.get(v, 0), c3.get(v, 0), value(c2.get(v, 0), c3.get(v, 0), decay, length))
            for v in sorted((set(c2) | set(c3)) - drop)]


def visits(rowptr, col, sources, walks: int, length: int, seed: int, decay=None, m_rowptr=None, m_col=None):
    """Mirror of the entry pair: (ptr int64 [Q + 1], edges int64 [T, 2], val float32 [T], visits int32 [T, 2])."""
    ptr, edges, val, vis, memo = [0], [], [], [], {}
    for s in (int(v) for v in sources):
        if s not in memo:
            memo[s] = source_segment(rowptr, col, s, walks, length, seed, decay, m_rowptr, m_col)
        for v, a, b, x in memo[s]:
            edges.append((s, v)); val.append(x); vis.append((a, b))
        ptr.append(len(edges))
    return (np.array(ptr, dtype=np.int64), np.array(edges, dtype=np.int64).reshape(-1, 2), np.array(val, dtype=np.float32),
            np.array(vis, dtype=np.int32).reshape(-1, 2))


def short_list(ptr, edges, val, m: int):
    """The m best of every segment — higher val first, ties to the lower node id — returned in ascending id:
    (ptr_m int64 [Q + 1], edges_m int64 [T_m, 2])."""
    ptr_m, keep = [0], []
    for q in range(len(ptr) - 1):
        seg = list(range(int(ptr[q]), int(ptr[q + 1])))
        best = sorted(seg, key=lambda i: (-float(val[i]), int(edges[i, 1])))[:m]
        keep.extend(sorted(best))
        ptr_m.append(len(keep))
    return np.array(ptr_m, dtype=np.int64), np.asarray(edges)[keep].reshape(-1, 2)


def ranks(ptr, edges, val, q: int, targets):
    """1-based place of every target among the candidates of segment q in the order of ``short_list``; 0 = not visited."""
    seg = list(range(int(ptr[q]), int(ptr[q + 1])))
    order = sorted(seg, key=lambda i: (-float(val[i]), int(edges[i, 1])))
    place = {int(edges[i, 1]): r + 1 for r, i in enumerate(order)}
    return [place.get(int(t), 0) for t in targets]
