"""Reference of the order-exact column sums (ocn_hip.h: ocn_cn_colsum_exact) in numpy float32, written from the documented
arithmetic and from nothing else: no sort network, no buckets, no staging — the union entries of a column in ascending flag
position, added one by one.

    statistic   no union entry: scale = 1;  union entries but no column with n1 >= 2: nip = ip;
                else scale = 1f / float(min{n1 >= 2}), nip = ip / scale                      (common.h: cn5_column_stats, cn5_nip)
    column      inv1 = 1f / n1 if n1 >= 2 else 0,  t = fl(nip * inv1)
    ordered     t != 0, or the integer sum (walks if valued, else n2) >= 2^24, or cn6
    unordered   a touched column: S2 = float(n2) (float(walks) if valued)
    entry       v2 = fl(c - tt): c = wc (or 1) where the entry has CN2 else 0, tt = t where it has CN1 else 0;
                an entry whose flagsA byte is 0 (cn6's wider union) adds +0
    S2          s2_init[c] (or 0) + v2 + v2 + ..., sequentially
    cn6         inv2 = 1 / (S2 or 1);  v3 = fl(fl(a3 - tt) - fl(nip * (in2 ? fl(v2 * inv2) : 0)));  S3 = 0 + v3 + v3 + ...

Every operation is one numpy float32 operation (rounded once, never fused).  Columns of equal length are summed side by side:
an elementwise float32 add rounds each column exactly as the scalar add would.
"""
from collections import namedtuple

import numpy as np

CS_WAVE_MAX = 64        # colsum.hip: columns of at most this many entries take one wave (rank sort in registers)
CS_MED_MAX = 512        # ... up to this many one wave with the keys in LDS (2, 4 or 8 registers of keys per lane)
CS_LDS = 4096           # ... up to this many one workgroup, sorted in LDS; beyond: sorted in place in memory
CS_CHUNK = 2048         # values staged per accumulation round of such a column
CS_BINS = 256           # the LDS sort: one bucket pass by position range ...
CS_BIN_MAX = 48         # ... unless a bucket holds more than this: then the bitonic network

HIST_FIELD_BITS = 21    # ops.HIST_FIELD_BITS: hist word 0 = n1 | n2 << 21 | n_union << 42, word 1 = walks
F_CN1, F_CN2 = 1, 2     # ocn_hip.h: OCN_F_CN1, OCN_F_CN2
EXACT_INT = 1 << 24     # integer sums below this are exact in fp32 in any order

f32 = np.float32

Sums = namedtuple("Sums", "s2 s3 written length ordered nip")


def hist_pack(n1, n2, nu, walks):
    """int64 [N, 2] in the packing of ``ops.hist_counts``."""
    b = HIST_FIELD_BITS
    w0 = np.asarray(n1, np.int64) | (np.asarray(n2, np.int64) << b) | (np.asarray(nu, np.int64) << (2 * b))
    return np.stack([w0, np.asarray(walks, np.int64)], axis=1)


def hist_counts(hist):
    m = (1 << HIST_FIELD_BITS) - 1
    p = hist[:, 0]
    return p & m, (p >> HIST_FIELD_BITS) & m, (p >> (2 * HIST_FIELD_BITS)) & m, hist[:, 1]


def hist_of_flags(col_of_pos, flagsA, wc, n_cols):
    """The histogram the intersection pass leaves for these flags: ``col_of_pos[q]`` = the column of flag position q."""
    fa = flagsA[:col_of_pos.size]
    cnt = lambda m: np.bincount(col_of_pos[m], minlength=n_cols).astype(np.int64)
    walks = np.zeros(n_cols, np.int64)
    if wc is not None:
        m = (fa & F_CN2) != 0
        np.add.at(walks, col_of_pos[m], wc[:col_of_pos.size][m].astype(np.int64))
    return hist_pack(cnt((fa & F_CN1) != 0), cnt((fa & F_CN2) != 0), cnt(fa != 0), walks)


def nip_of(hist, innerprod):
    n1 = hist_counts(hist)[0]
    ip = f32(innerprod)
    if not (hist[:, 0] != 0).any():
        return f32(ip / f32(1))
    big = n1[n1 >= 2]
    if big.size == 0:
        return ip
    scale = f32(1) / f32(int(big.min()))
    return f32(ip / scale)


def union_entries(rowptr, col, src, off, flagsA, flagsB):
    """(column, flag position) of every union entry of the batch, sorted by column, then by position."""
    B = src.size
    a0 = rowptr[src]
    da = rowptr[src + 1] - a0
    base = off[:B]
    keep = base + da <= flagsA.size                      # a row beyond the flag capacity has no flags
    a0, da, base = a0[keep], da[keep], base[keep]
    rep = np.repeat(np.arange(da.size), da)
    within = np.arange(int(da.sum())) - np.repeat(np.cumsum(da) - da, da)
    pos = base[rep] + within
    k = col[a0[rep] + within].astype(np.int64)
    f = flagsA[pos] != 0
    if flagsB is not None:
        f |= (flagsB[pos] & F_CN1) != 0
    pos, k = pos[f], k[f]
    o = np.lexsort((pos, k))
    return k[o], pos[o]


def _chain(acc, v):
    """acc + v[:, 0] + v[:, 1] + ... per row, one float32 add at a time."""
    assert acc.dtype == np.float32 and v.dtype == np.float32
    for i in range(v.shape[1]):
        acc = acc + v[:, i]
    return acc


def colsum(rowptr, col, src, off, flagsA, flagsB, wc, hist, innerprod, s2_init=None, order=None):
    """S2 (and S3 with ``flagsB``) as float32 [N].  The arguments are those of ``ops.cn_colsum_exact`` as numpy arrays.
    ``written``: the columns the entry writes at all (the others are 0 here); ``length``: entries per column in this call.
    ``order`` (L -> a permutation of range(L)): add every column's values in that order instead of the ascending one — what
    a wrong rank would give; S3 still takes inv2 from the ascending S2.  For the tests of the cases, never the reference."""
    N = hist.shape[0]
    n1, n2, _, walks = hist_counts(hist)
    cn6, valued = flagsB is not None, wc is not None
    assert not (cn6 and (valued or s2_init is not None))
    nip = nip_of(hist, innerprod)
    inv1 = np.where(n1 >= 2, f32(1) / np.maximum(n1, 1).astype(np.float32), f32(0)).astype(np.float32)
    t = nip * inv1
    isum = walks if valued else n2
    ordered = (t != 0) | (isum >= EXACT_INT) | cn6
    s2 = np.zeros(N, np.float32) if s2_init is None else s2_init.astype(np.float32).copy()
    s3 = np.zeros(N, np.float32) if cn6 else None
    written = np.full(N, s2_init is not None)
    closed = (hist[:, 0] != 0) & ~ordered
    s2[closed] = isum[closed].astype(np.float32)
    written[closed] = True
    k, pos = union_entries(rowptr, col, src, off, flagsA, flagsB)
    length = np.bincount(k, minlength=N).astype(np.int64)
    start = np.cumsum(length) - length
    chained = ordered & (length > 0)
    for L in np.unique(length[chained]):
        L = int(L)
        cols = np.flatnonzero(chained & (length == L))
        P = pos[start[cols][:, None] + np.arange(L)[None, :]]
        perm = np.arange(L) if order is None else np.asarray(order(L))
        fa = flagsA[P]
        c = np.where((fa & F_CN2) != 0, wc[P].astype(np.float32) if valued else f32(1), f32(0)).astype(np.float32)
        tt = np.where((fa & F_CN1) != 0, t[cols][:, None], f32(0)).astype(np.float32)
        v2 = c - tt
        in2 = fa != 0
        val = np.where(in2, v2, f32(0))
        asc = _chain(s2[cols], val)
        s2[cols] = asc if order is None else _chain(s2[cols], val[:, perm])
        written[cols] = True
        if cn6:
            inv2 = f32(1) / np.where(asc == 0, f32(1), asc)
            a3 = np.where((flagsB[P] & F_CN1) != 0, f32(1), f32(0)).astype(np.float32)
            a2n = np.where(in2, v2 * inv2[:, None], f32(0))
            v3 = (a3 - tt) - nip * a2n
            s3[cols] = _chain(np.zeros(cols.size, np.float32), v3[:, perm])
    assert s2.dtype == np.float32 and t.dtype == np.float32 and (s3 is None or s3.dtype == np.float32)
    return Sums(s2, s3, written, length, ordered, nip)


def bits(x):
    """float32 array -> its bit patterns (so that -0.0 != +0.0 and NaN == NaN in a comparison)."""
    return np.ascontiguousarray(x, np.float32).view(np.uint32)
