"""CPU mirror of the structured negative samplers (include/ocn_hip.h: ocn_philox4x32, ocn_sample_complement_rows,
ocn_sample_complement_pairs) in plain numpy and Python integers: the generator, the multiply-high, the selection in the
complement of a row and the pair selection — written from the contract, not from the kernels, and slow on purpose."""
import bisect

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

# Known answers of Philox4x32-10 (the Random123 test vectors): (counter, key, output)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox4x32(ctr, key):
    """Philox4x32-10 of one counter (four uint32 words) under one key (two words), as Python integers."""
    c0, c1, c2, c3 = (int(v) & MASK32 for v in ctr)
    k0, k1 = (int(v) & MASK32 for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def philox4x32_np(ctr: np.ndarray, key) -> np.ndarray:
    """The same for an [n, 4] uint32 array of counters, vectorised (uint64 products)."""
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(int(key[0]) & MASK32), np.uint64(int(key[1]) & MASK32)
    m32, sh = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ k0, p1 & m32, (p0 >> sh) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return np.stack(c, axis=1).astype(np.uint32)


def mulhi(u: int, m: int) -> int:
    """floor(u * m / 2^64) for 0 <= u < 2^64."""
    return (int(u) * int(m)) >> 64


def key_of(seed: int):
    return int(seed) & MASK32, int(seed) >> 32


def rank_rows(seed: int, q: int, j: int, m: int) -> int:
    w = philox4x32((j, q & MASK32, q >> 32, 2), key_of(seed))
    return mulhi(w[0] | (w[1] << 32), m)


def rank_pairs(seed: int, t: int, m: int) -> int:
    w = philox4x32((t & MASK32, t >> 32, 0, 1), key_of(seed))
    return mulhi(w[0] | (w[1] << 32), m)


def excluded(row_cols, s: int):
    """X(s): the ascending columns of the row with s spliced in, counted once."""
    return sorted(set(int(c) for c in row_cols) | {int(s)})


def select(xs, r: int) -> int:
    """The r-th smallest (0-based) non-negative integer outside the ascending list xs: r + i, i the smallest index with
    xs[i] - i > r, len(xs) if there is none (binary search: xs[i] - i never decreases)."""
    lo, hi = 0, len(xs)
    while lo < hi:
        mid = (lo + hi) // 2
        if xs[mid] - mid > r:
            hi = mid
        else:
            lo = mid + 1
    return r + lo


def negative_targets(rowptr, col, n: int, sources, per: int, seed: int, first: int = 0) -> np.ndarray:
    """Mirror of ocn_amd.sampling.negative_targets on a CSR given as numpy arrays: int64 [Q, per]."""
    out = np.full((len(sources), per), -1, dtype=np.int64)
    for q, s in enumerate(int(v) for v in sources):
        xs = excluded(col[rowptr[s]:rowptr[s + 1]], s)
        m = n - len(xs)
        if m <= 0:
            continue
        for j in range(per):
            out[q, j] = select(xs, rank_rows(seed, first + q, j, m))
    return out


def complement_ptr(rowptr, col, n: int):
    """Prefix of the complement sizes as a list of Python integers, [n + 1]."""
    cptr = [0]
    for s in range(n):
        cptr.append(cptr[-1] + n - len(excluded(col[rowptr[s]:rowptr[s + 1]], s)))
    return cptr


def negative_edges(rowptr, col, n: int, num: int, seed: int, first: int = 0, cptr=None) -> np.ndarray:
    """Mirror of ocn_amd.sampling.negative_edges: int64 [2, num].  ``cptr``: the prefix, where the caller has it already (any
    indexable of integers; computing it here walks every row)."""
    cptr = complement_ptr(rowptr, col, n) if cptr is None else cptr
    total = int(cptr[n])
    assert total > 0
    out = np.empty((2, num), dtype=np.int64)
    for t in range(num):
        r = rank_pairs(seed, first + t, total)
        s = bisect.bisect_right(cptr, r, 0, n) - 1          # the last row with cptr[s] <= r
        out[0, t] = s
        out[1, t] = select(excluded(col[rowptr[s]:rowptr[s + 1]], s), r - int(cptr[s]))
    return out
