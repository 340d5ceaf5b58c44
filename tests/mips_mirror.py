"""The contract of ``ocn_mips_topm_i8`` (include/ocn_hip.h) in plain CPU torch, for the embedding-retrieval tests: an int64
matmul (exact), ``float32(dot) * kscale`` (the one rounding), eligibility from Python sets, a stable sort by (-val with -0.0
folded onto +0.0, node id), cut and pad — and the place of given nodes in that order."""
import torch


def values(query_q, keys_q, kscale):
    """val [Q, N] float32: the exact integer dot products, converted (exact below 2^24) and scaled by one fp32 multiply."""
    dot = query_q.cpu().to(torch.int64) @ keys_q.cpu().to(torch.int64).t()
    assert int(dot.abs().max()) < (1 << 24) if dot.numel() else True
    return dot.to(torch.float32) * kscale.cpu().to(torch.float32)[None, :]


def excluded(q, rows, excl, drop_self):
    """The set of node ids query ``q`` may not be offered."""
    out = set()
    if rows is None:
        return out
    s = int(rows[q])
    if drop_self:
        out.add(s)
    if excl is not None:
        rp, col = excl
        out.update(col[int(rp[s]):int(rp[s + 1])].tolist())
    return out


def ordered(val, rows=None, excl=None, drop_self=True):
    """Per query the eligible node ids in the contract's order (a list of int64 tensors)."""
    Q, N = val.shape
    rows = None if rows is None else rows.cpu()
    excl = None if excl is None else (excl[0].cpu(), excl[1].cpu())
    neg = -(val + 0.0)                                       # -0.0 + 0.0 = +0.0: the two zeros get one image
    order = torch.sort(neg, dim=1, stable=True).indices      # ascending -val = descending val, ties in ascending node id
    out = []
    for q in range(Q):
        keep = torch.ones(N, dtype=torch.bool)
        ex = sorted(x for x in excluded(q, rows, excl, drop_self) if 0 <= x < N)
        if ex:
            keep[torch.tensor(ex)] = False
        o = order[q]
        out.append(o[keep[o]])
    return out


def cut(val, lists, m):
    """(top_val [Q, m], top_node [Q, m]) of ordered lists: the first ``m``, padded with -inf / -1."""
    Q = val.shape[0]
    tv = torch.full((Q, m), float("-inf"), dtype=torch.float32)
    tn = torch.full((Q, m), -1, dtype=torch.int64)
    for q, o in enumerate(lists):
        k = min(m, o.numel())
        tn[q, :k] = o[:k]
        tv[q, :k] = val[q, o[:k]]
    return tv, tn


def topm(query_q, keys_q, kscale, m, rows=None, excl=None, drop_self=True):
    val = values(query_q, keys_q, kscale)
    return cut(val, ordered(val, rows, excl, drop_self), m)


def ranks(query_q, keys_q, kscale, rows, excl, drop_self, tptr, tnode):
    """rank int64 [P]: for target j of query q, 1 + the eligible nodes that precede it in the order, 0 where it is not
    eligible (or no node id)."""
    val = values(query_q, keys_q, kscale)
    lists = ordered(val, rows, excl, drop_self)
    tptr, tnode = tptr.cpu().tolist(), tnode.cpu().tolist()
    out = torch.zeros(len(tnode), dtype=torch.int64)
    for q, o in enumerate(lists):
        place = {int(n): i + 1 for i, n in enumerate(o.tolist())}
        for j in range(tptr[q], tptr[q + 1]):
            out[j] = place.get(int(tnode[j]), 0)
    return out
