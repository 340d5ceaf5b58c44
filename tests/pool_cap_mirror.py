"""The capped pooling (include/ocn_hip.h: ocn_cn_gather_cap) restated in numpy and Python integers, from the contract and
not from the kernel: the strata, the picks (Philox4x32-10 through ``sampling_mirror``), the multipliers and the three pooled
rows in fp32 with every multiply and add rounded separately, in ascending position."""
import numpy as np

from tests.sampling_mirror import key_of, mulhi, philox4x32

STREAM_CN_CAP = 7
F32 = np.float32


def strata(u: int, d: int):
    """The bounds [lo_t, lo_{t+1}) of the d strata of u > d ranks: lo_t = ceil(t u / d)."""
    return [(-(-t * u // d), -(-(t + 1) * u // d)) for t in range(d)]


def stratum_of(r: int, u: int, d: int) -> int:
    return r * d // u


def pick(seed: int, i: int, j: int, t: int, lo: int, size: int) -> int:
    """The selected rank of stratum t of candidate (i, j)."""
    w = philox4x32((i, j, t, STREAM_CN_CAP), key_of(seed))
    return lo + mulhi(w[0] | (w[1] << 32), size)


def multipliers(member, i: int, j: int, cap: int, seed: int):
    """One integer per position of the source row: the multiplier of a selected member, 0 for any other position.
    ``member``: truth value per position, ascending."""
    member = [bool(v) for v in member]
    pos = [p for p, m in enumerate(member) if m]
    u, out = len(pos), [0] * len(member)
    if u <= cap:
        for p in pos:
            out[p] = 1
        return out
    for t, (lo, hi) in enumerate(strata(u, cap)):
        out[pos[pick(seed, i, j, t, lo, hi - lo)]] = hi - lo
    return out


def entry_weights(f: int, w, c):
    """(wa, wb) of an entry with flag byte f, column weights w = {w1, t, inv2, .} and cn2 value c (fp32 throughout)."""
    wa = F32(w[0]) if f & 1 else F32(0)
    v = F32((F32(c) if f & 2 else F32(0)) - (F32(w[1]) if f & 1 else F32(0)))
    return wa, F32(v * F32(w[2]))


def pool(rowptr, col, src, dst, off, flags, wc, weights, h, cap: int, seed: int):
    """mult (int64, one per flag position up to off[B]; positions of no batch row stay -1) and xcn1, xcn2, xij (fp32 [B, H],
    batch order)."""
    B, H = len(src), h.shape[1]
    h = np.ascontiguousarray(h, dtype=F32)
    mult = np.full(int(max((int(off[e]) + int(rowptr[src[e] + 1] - rowptr[src[e]]) for e in range(B)), default=0)), -1, np.int64)
    x1, x2, xij = np.zeros((B, H), F32), np.zeros((B, H), F32), np.zeros((B, H), F32)
    with np.errstate(all="ignore"):
        for e in range(B):
            i, j = int(src[e]), int(dst[e])
            a0, da, base = int(rowptr[i]), int(rowptr[i + 1] - rowptr[i]), int(off[e])
            s = multipliers(flags[base:base + da] != 0, i, j, cap, seed)
            mult[base:base + da] = s
            a1, a2 = np.zeros(H, F32), np.zeros(H, F32)
            for p in range(da):
                f = int(flags[base + p])
                if not f:
                    continue
                k = int(col[a0 + p])
                wa, wb = entry_weights(f, weights[k], F32(wc[base + p]) if wc is not None else F32(1))
                wa, wb = F32(wa * F32(s[p])), F32(wb * F32(s[p]))
                if wa != 0 or wb != 0:
                    a1 = a1 + wa * h[k]               # float32 arrays: one rounded multiply, one rounded add per feature
                    a2 = a2 + wb * h[k]
            x1[e], x2[e], xij[e] = a1, a2, h[i] * h[j]
    return mult, x1, x2, xij
