"""The edges of the lane-group walk (ocn_amd/csrc/lane_group.h) on a graph built by hand: source rows that end on, one before and
one past a round of positions, members at the first and the last position of a row, candidates without a member, member counts
of every residue mod 8 (the tails of the four- and eight-wide take), a part-full last wave, lane groups that do not start at
lane 0.  Embeddings, gradients and weights are small integers and powers of two, so every product and sum is exact in fp32
whatever its order, and the expected values are plain torch on the CPU.  Every kernel that walks this way, at every width:
``ops.cn8_pool``, ``ops.cn_pool_frozen``, the chain ``cn_flags`` -> ``cn_gather`` on the packed form, ``cn_gather3``,
``cn_attribution``."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WIDTHS = (16, 32, 64, 128, 256, 512)
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 128, 129)      # |N(s_L)|: a round is 32 positions at H = 16 and 64 at every other width
LEAVES = 129
KINDS = ("all", "none", "third", "last")
N = 200                                                 # leaves 0 .. 128, sources 129 .. 138, targets 139 .. 178, the rest isolated


def target_rows(kind, L):
    """The leaves in row t of T1 (= A: the target's neighbours), of T2 and of T3 for a target of this kind."""
    last = [L - 1] if L > 0 else []
    return {"all": (range(LEAVES), range(5, LEAVES), range(3)),
            "none": ((), (), ()),
            "third": (range(0, LEAVES, 3), range(1, LEAVES, 3), range(2, LEAVES, 3)),
            "last": (last, sorted(set([0] + last)) if L > 0 else [], last)}[kind]


def matrix(rows):
    """SparseTensor [N, N] on the device with row r = rows[r] (a dict of column lists)."""
    from ocn_amd.sparse import SparseTensor
    ei = torch.tensor([[r, c] for r, cols in rows.items() for c in cols], dtype=torch.long).t().contiguous()
    return SparseTensor.from_edge_index(ei.to(DEV), sparse_sizes=(N, N))


@pytest.fixture(scope="module")
def star(hiplib):
    """Source s_L is adjacent to the leaves 0 .. L-1 and to nothing else, so position p of its row is leaf p.  One target per
    (L, kind).  The 40 candidates (s_L, t_{L, kind}) in a shuffled order; f1 / f2 / f3 [40, 129]: leaf p is a member of the
    candidate's cn1 / cn2 / cn3 set (p < L and p in row t of T1 / T2 / T3) — from the construction."""
    from ocn_amd.utils import CNState
    a_rows, t2_rows, t3_rows, cand = {}, {}, {}, []
    for q, L in enumerate(LENGTHS):
        s = LEAVES + q
        a_rows[s] = list(range(L))
        for kq, kind in enumerate(KINDS):
            t = LEAVES + len(LENGTHS) + 4 * q + kq
            r1, r2, r3 = (list(r) for r in target_rows(kind, L))
            a_rows[t], t2_rows[t], t3_rows[t] = r1, r2, r3
            cand.append((s, t, L, r1, r2, r3))
    for r, cols in list(a_rows.items()):                # A is symmetric; the leaves' rows play no part (no leaf is an endpoint)
        for c in cols:
            a_rows.setdefault(c, []).append(r)
    perm = torch.randperm(len(cand), generator=torch.Generator().manual_seed(5)).tolist()
    cand = [cand[p] for p in perm]
    B = len(cand)
    f = torch.zeros(3, B, LEAVES, dtype=torch.bool)
    for e, (_, _, L, r1, r2, r3) in enumerate(cand):
        for q, r in enumerate((r1, r2, r3)):
            f[q, e, [p for p in r if p < L]] = True
    length = torch.tensor([c[2] for c in cand])
    # what the walks take: the entries with any flag.  Every residue mod 8, so a trip of four and of eight ends on every tail;
    # rows that end exactly on, before and past a round; and the widths below 512 put more than one candidate into a wave
    members = (f[0] | f[1]).sum(1)
    assert {int(m) % 8 for m in members} == set(range(8)), sorted(members.tolist())
    assert {int(m) % 8 for m in f[0].sum(1)} >= {0, 1, 3, 5, 6, 7} and int(members.max()) == 129 and int((members == 0).sum()) >= 10
    assert B == 40 and B % 16 != 0                      # H = 16: sixteen candidates per wave, the last wave part full
    e = torch.tensor([[c[0] for c in cand], [c[1] for c in cand]])
    adj, t2, t3 = matrix(a_rows), matrix(t2_rows), matrix(t3_rows)
    ed = e.to(DEV)
    st = CNState(adj, adj, t2, ed)                      # the (A, A, T2) pass and the (A, T3) pass share the offsets
    st3 = CNState(adj, t3, None, ed)
    st.check_status(); st3.check_status()
    off = torch.cat([torch.zeros(1, dtype=torch.long), length.cumsum(0)])
    assert torch.equal(st.off.cpu(), off) and torch.equal(st3.off.cpu(), off)
    flags = torch.zeros(int(off[-1]), dtype=torch.uint8)
    flags3 = torch.zeros_like(flags)
    for b in range(B):
        L = int(length[b])
        flags[off[b]:off[b + 1]] = (f[0, b, :L].to(torch.uint8) | (f[1, b, :L].to(torch.uint8) << 1))
        flags3[off[b]:off[b + 1]] = f[2, b, :L].to(torch.uint8)
    assert torch.equal(st.flags[:flags.numel()].cpu(), flags) and torch.equal(st3.flags[:flags.numel()].cpu() & 1, flags3)
    return SimpleNamespace(B=B, e=e, ed=ed, src=ed[0].contiguous(), dst=ed[1].contiguous(), adj=adj, t2=t2, t3=t3, f=f.double(),
                           length=length, off=off, flags=flags, st=st, st3=st3)


def embeddings(H, seed=0):
    return torch.randint(-4, 5, (N, H), generator=torch.Generator().manual_seed(1000 * seed + H)).double()


def table(seed):
    """{w1, t, inv2, 0} per column from small integers and powers of two, zeros among them: entries with wa = wb = 0 are not
    fetched, others add to one accumulator only."""
    g = torch.Generator().manual_seed(seed)
    pick = lambda vals: torch.tensor(vals, dtype=torch.double)[torch.randint(0, len(vals), (N,), generator=g)]
    return torch.stack([pick([0.0, 1.0, 2.0, -1.0, 0.5]), pick([0.0, 1.0, 2.0, 0.5]), pick([0.0, 1.0, 0.5, 2.0]),
                        torch.zeros(N, dtype=torch.double)], dim=1)


def entry_weights(c, w):
    """(wa, wb) [B, 129] of the pattern route: wa = [cn1] w1, wb = ([cn2] - [cn1] t) inv2, per candidate and leaf."""
    w = w[:LEAVES]
    return c.f[0] * w[:, 0], (c.f[1] - c.f[0] * w[:, 1]) * w[:, 2]


def same(got, want):
    return torch.equal(got.cpu(), want.float())


def pooled(c, x, wa, wb):
    return wa @ x[:LEAVES], wb @ x[:LEAVES], x[c.e[0]] * x[c.e[1]]


@pytest.mark.parametrize("H", WIDTHS)
def test_cn8_pool(star, H):
    """T1 as CSR rows, T2 as bit rows: both probes in one launch."""
    from ocn_amd import ops
    c = star
    x = embeddings(H)
    adj, t2 = c.adj, c.t2
    bm2 = ops.bitrows_from_csr(t2._rowptr, t2._col, N)
    x1, x2, xij, n1, n2 = ops.cn8_pool(adj._rowptr, adj._col, (adj._rowptr, adj._col), None, c.src, c.dst, x.float().to(DEV),
                                       t2_bitmap=bm2)
    w1, w2, wij = pooled(c, x, c.f[0], c.f[1])
    assert same(x1, w1) and same(x2, w2) and same(xij, wij)
    assert torch.equal(n1.cpu().long(), c.f[0].sum(1).long()) and torch.equal(n2.cpu().long(), c.f[1].sum(1).long())
    assert bool(w1.any()) and bool(w2.any())


@pytest.mark.parametrize("H", WIDTHS)
def test_cn_pool_frozen(star, H):
    """T1 as bit rows, T2 as CSR rows; the counts are the member counts whatever the weights."""
    from ocn_amd import ops
    c = star
    x, w = embeddings(H, 1), table(3)
    adj, t2 = c.adj, c.t2
    bm1 = ops.bitrows_from_csr(adj._rowptr, adj._col, N)
    x1, x2, xij, n1, n2 = ops.cn_pool_frozen(adj._rowptr, adj._col, None, (t2._rowptr, t2._col), c.src, c.dst,
                                             x.float().to(DEV), w.float().to(DEV), t1_bitmap=bm1)
    wa, wb = entry_weights(c, w)
    w1, w2, wij = pooled(c, x, wa, wb)
    assert same(x1, w1) and same(x2, w2) and same(xij, wij)
    assert torch.equal(n1.cpu().long(), c.f[0].sum(1).long()) and torch.equal(n2.cpu().long(), c.f[1].sum(1).long())
    assert bool(w1.any()) and bool(w2.any()) and int(((wa == 0) & (wb == 0) & (c.f[0] + c.f[1] > 0)).sum()) > 0


@pytest.mark.parametrize("H", WIDTHS)
def test_flags_then_gather_on_the_packed_form(star, H):
    """Below H = 128 a batch of fewer than 262 144 / LPE candidates is pooled by the wave form, which walks otherwise: there the
    40 candidates are repeated until the launch takes the packed form (the expected rows repeat with them)."""
    from ocn_amd.utils import CNState
    c = star
    lpe = min(H // 4, 64)
    reps = 1 if lpe >= 32 else -(-262144 // (lpe * c.B))
    x, w = embeddings(H, 2), table(4)
    st = c.st if reps == 1 else CNState(c.adj, c.adj, c.t2, c.ed.repeat(1, reps))
    x1, x2, xij = st.gather(w.float().to(DEV), x.float().to(DEV))
    st.check_status()
    wa, wb = entry_weights(c, w)
    w1, w2, wij = (t.repeat(reps, 1) for t in pooled(c, x, wa, wb))
    assert x1.shape[0] == c.B * reps and (lpe >= 32 or x1.shape[0] * lpe >= 262144)
    assert same(x1, w1) and same(x2, w2) and same(xij, wij)


@pytest.mark.parametrize("H", WIDTHS)
def test_cn_gather3(star, H):
    """w1 = [cn1] inv1, w2 = ([cn2] - t [cn1]) inv2, w3 = (([cn3] - t [cn1]) - nip w2) inv3 per entry."""
    from ocn_amd import ops
    c = star
    x, wA, wB = embeddings(H, 3), table(5), table(6)
    nip = 2.0
    adj = c.adj
    out = ops.cn_gather3(adj._rowptr, adj._col, c.src, c.dst, c.st.off, c.st.flags, c.st3.flags, wA.float().to(DEV),
                         wB.float().to(DEV), torch.tensor([nip], device=DEV), x.float().to(DEV))
    a, inv3 = wA[:LEAVES], wB[:LEAVES, 0]
    tt = c.f[0] * a[:, 1]
    w1 = c.f[0] * a[:, 0]
    w2 = (c.f[1] - tt) * a[:, 2]
    w3 = ((c.f[2] - tt) - nip * w2) * inv3
    for got, want in zip(out, (w1 @ x[:LEAVES], w2 @ x[:LEAVES], w3 @ x[:LEAVES], x[c.e[0]] * x[c.e[1]])):
        assert same(got, want) and bool(want.any())


@pytest.mark.parametrize("H", WIDTHS)
def test_cn_attribution(star, H):
    """Per flag position {wa <h[k], g1[e]>, wb <h[k], g2[e]>}, their sum as the rank, -inf where the position is no member."""
    from ocn_amd import ops
    c = star
    x, w = embeddings(H, 4), table(7)
    gen = torch.Generator().manual_seed(H)
    g1, g2 = (torch.randint(-3, 4, (c.B, H), generator=gen).double() for _ in range(2))
    adj, st = c.adj, c.st
    attr, rank = ops.cn_attribution(adj._rowptr, adj._col, c.src, st.off, st.flags, None, w.float().to(DEV), x.float().to(DEV),
                                    g1.float().to(DEV), g2.float().to(DEV))
    wa, wb = entry_weights(c, w)
    r1, r2 = wa * (g1 @ x[:LEAVES].t()), wb * (g2 @ x[:LEAVES].t())        # [B, 129]
    total = int(c.off[-1])
    want_attr, want_rank = torch.zeros(total, 2, dtype=torch.double), torch.full((total,), float("-inf"), dtype=torch.double)
    for b in range(c.B):
        L = int(c.length[b])
        want_attr[c.off[b]:c.off[b + 1]] = torch.stack([r1[b, :L], r2[b, :L]], dim=1)
        member = c.flags[c.off[b]:c.off[b + 1]] != 0
        want_rank[c.off[b]:c.off[b + 1]][member] = (r1[b, :L] + r2[b, :L])[member]
    assert same(attr[:total], want_attr) and same(rank[:total], want_rank)
    assert bool(want_attr.any()) and int(torch.isinf(want_rank).sum()) > 100 and int(torch.isfinite(want_rank).sum()) > 100
