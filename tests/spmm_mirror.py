"""CPU mirror of the encoder SpMM (include/ocn_hip.h: ocn_spmm_csr, ocn_spmm_csr_rows, ocn_deg_rsqrt) in plain torch on the CPU:
float32, every product and every sum a tensor operation of its own (one IEEE rounding each), no library call — written from the
documented order contract, not from the kernel.  A row's terms are laid out first (which entry or the self term stands at which
position), then added position by position over all rows at once.

The order contract: a row's entries are taken in ascending column order; the product and the sum are rounded separately; the self
term stands at the sorted position of the diagonal (``self_mode=2``: before the first column >= r, at the end where there is none)
or after the neighbours (``self_mode=1``); under ``self_mode=2`` an explicit self loop is replaced, not doubled; mean divides by the
number of terms it added (1 where there were none); ``post`` comes last.

Also here: the fixed graph and the forms the SpMM tests share, and a float64 dense restatement that checks the mirror itself."""
import itertools

import torch

LENGTHS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
N_FIXED = 261
WIDTHS = [16, 32, 64, 128, 256, 512]
MODES = ["sum", "mean", "max"]


def _f32(t):
    return torch.as_tensor(t).to(torch.float32)


def term_layout(rowptr, col, self_mode):
    """(src [n, T] int64, count [n] int64): position t of row r holds entry src[r, t] (an index into col / val), -1 for the
    self term, -2 past the row's last term."""
    rp, cl = rowptr.tolist(), col.tolist()
    n = len(rp) - 1
    rows = []
    for r in range(n):
        ent = list(range(rp[r], rp[r + 1]))
        assert all(cl[a] < cl[b] for a, b in zip(ent, ent[1:])), "columns must ascend in a row"
        if self_mode == 1:
            ent = ent + [-1]
        elif self_mode == 2:
            below = [p for p in ent if cl[p] < r]
            above = [p for p in ent if cl[p] > r]             # the entry with column r itself, if any, is dropped: replaced
            ent = below + [-1] + above
        rows.append(ent)
    T = max([len(e) for e in rows] + [1])
    src = torch.full((n, T), -2, dtype=torch.int64)
    for r, ent in enumerate(rows):
        if ent:
            src[r, :len(ent)] = torch.tensor(ent, dtype=torch.int64)
    return src, torch.tensor([len(e) for e in rows], dtype=torch.int64)


def spmm(rowptr, col, x, pre=None, post=None, mode="sum", edge_scale=False, self_mode=0, val=None):
    """What ocn_spmm_csr documents, term by term: float32 [n, F] for the operator (rowptr, col[, val]) with n rows."""
    rowptr, col = rowptr.to(torch.int64), col.to(torch.int64)
    n = rowptr.numel() - 1
    x = _f32(x)
    F = x.shape[1]
    weighted = pre is not None or val is not None
    rowid = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    # the weight of every entry and of every row's self term, each product rounded to float32 on its own
    wk = torch.ones(col.numel(), dtype=torch.float32)
    wself = torch.ones(n, dtype=torch.float32)
    if pre is not None:
        pre = _f32(pre)
        wk = pre[rowid] * pre[col] if edge_scale else pre[col].clone()
        if self_mode:
            wself = pre[:n] * pre[:n] if edge_scale else pre[:n].clone()
    if val is not None:
        wk = _f32(val) * wk
    src, count = term_layout(rowptr, col, self_mode)
    # rows by falling term count: the rows that still have a term at position t are a prefix
    order = torch.argsort(count, descending=True, stable=True)
    src_o, count_o = src[order], count[order]
    is_self = src_o == -1
    safe = src_o.clamp(min=0)
    w_o = torch.where(is_self, wself[order][:, None], wk[safe] if col.numel() else torch.ones_like(safe, dtype=torch.float32))
    k_o = torch.where(is_self, order[:, None], col[safe] if col.numel() else torch.zeros_like(safe))
    acc = torch.full((n, F), float("-inf") if mode == "max" else 0.0, dtype=torch.float32)
    for t in range(int(count_o.max()) if n else 0):
        m = int((count_o > t).sum())
        term = x[k_o[:m, t]]
        if weighted:
            term = w_o[:m, t, None] * term                    # fl(w * x) ...
        if mode == "max":
            acc[:m] = torch.maximum(acc[:m], term)
        else:
            acc[:m] = acc[:m] + term                          # ... then fl(acc + that)
    if mode == "max":
        acc[count_o == 0] = 0.0
    if mode == "mean":
        acc = acc / count_o.clamp(min=1).to(torch.float32)[:, None]
    out = torch.empty_like(acc)
    out[order] = acc
    if post is not None:
        out = _f32(post)[:, None] * out
    return out


def deg_rsqrt(rowptr, add, val=None):
    """What ocn_deg_rsqrt documents: the row length, or the sequential float32 row sum of ``val``, then 1 / sqrt(add + deg) with
    both operations IEEE-rounded; 0 where add + deg <= 0."""
    rowptr = rowptr.to(torch.int64)
    n = rowptr.numel() - 1
    length = rowptr[1:] - rowptr[:-1]
    if val is None:
        deg = length.to(torch.float32)
    else:
        val = _f32(val)
        deg = torch.zeros(n, dtype=torch.float32)
        for t in range(int(length.max()) if n else 0):
            live = length > t
            deg[live] = deg[live] + val[rowptr[:-1][live] + t]
    d = torch.tensor(add, dtype=torch.float32) + deg
    live = d > 0
    root = sqrt32(torch.where(live, d, torch.ones((), dtype=torch.float32)))
    return torch.where(live, recip32(root), torch.zeros((), dtype=torch.float32))


def _step(v, up):
    return torch.nextafter(v, torch.full_like(v, float("inf") if up else float("-inf")))


def sqrt32(d):
    """The correctly rounded float32 square root of a positive float32 tensor.  Not ``torch.sqrt``: on some hosts torch's CPU build
    takes it from a vector maths library that is an ulp off for one argument in eight (seen against the kernel, whose root IS
    correctly rounded).  A candidate from float64, then moved while it fails the definition: s is the rounded root iff
    (s - ulp/2)² < d < (s + ulp/2)², and those squares (25-bit numbers) are exact in float64."""
    d64 = d.to(torch.float64)
    s = torch.sqrt(d64).to(torch.float32)
    for _ in range(2):
        dn, up = _step(s, False), _step(s, True)
        lo = (s.to(torch.float64) + dn.to(torch.float64)) / 2
        hi = (s.to(torch.float64) + up.to(torch.float64)) / 2
        s = torch.where(lo * lo > d64, dn, torch.where(hi * hi < d64, up, s))
    return s


def recip32(s):
    """The correctly rounded float32 1 / s of a positive float32 tensor: of a float64 candidate and its two neighbours the one
    with the smallest |1 - q s| — a product of two float32 and its difference from 1 are exact in float64."""
    s64 = s.to(torch.float64)
    q = (1.0 / s64).to(torch.float32)
    cands = torch.stack([_step(q, False), q, _step(q, True)])
    err = (1.0 - cands.to(torch.float64) * s64).abs()
    return cands.gather(0, err.argmin(0, keepdim=True))[0]


# ---- what the SpMM tests share ----------------------------------------------------------------------------------------------------
def csr_from_rows(rows):
    """(rowptr int64, col int32) of a list of ascending column lists."""
    rowptr = torch.zeros(len(rows) + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([len(c) for c in rows], dtype=torch.int64), 0)
    return rowptr, torch.tensor([k for c in rows for k in c], dtype=torch.int32)


def random_rows(n_rows, n_cols, lengths, seed, loops_every=0):
    """Row r: ``lengths[r]`` distinct random columns below n_cols, ascending; with ``loops_every`` = m every m-th non-empty row has
    its own id among them (it takes the place of one of the drawn columns)."""
    g = torch.Generator().manual_seed(seed)
    rows, filled = [], 0
    for r in range(n_rows):
        cols = torch.randperm(n_cols, generator=g)[:lengths[r]].tolist()
        if cols:
            filled += 1
            if loops_every and filled % loops_every == 0 and r not in cols:
                cols[0] = r
        rows.append(sorted(cols))
    return rows


_fixed = {}


def fixed_graph():
    """The 261-node graph of the SpMM tests: row r has LENGTHS[r % 23] entries — for every lane-group size LPE in {4, 8, 16, 32, 64}
    a row of LPE - 1, LPE, LPE + 1, 2 LPE and 2 LPE + 1 entries, every remainder modulo the inner unroll of 4, a row of several
    trips — distinct random columns, ascending; every third non-empty row holds its own id.  261 is no multiple of 4 … 64, the rows
    of a workgroup at the six widths.  dict: rows, rowptr, col, val, pre, post (CPU tensors; treat them as read-only)."""
    if not _fixed:
        rows = random_rows(N_FIXED, N_FIXED, [LENGTHS[r % len(LENGTHS)] for r in range(N_FIXED)], seed=2610, loops_every=3)
        rowptr, col = csr_from_rows(rows)
        g = torch.Generator().manual_seed(2611)
        _fixed.update(rows=rows, rowptr=rowptr, col=col, n=N_FIXED,
                      pre=torch.rand(N_FIXED, generator=g) + 0.1, post=torch.rand(N_FIXED, generator=g) + 0.1,
                      val=torch.rand(col.numel(), generator=g) + 0.5)
    return _fixed


def fixed_x(F, n=N_FIXED):
    return torch.randn(n, F, generator=torch.Generator().manual_seed(1000 + F))


def forms(self_modes=(0, 1, 2)):
    """The 36 forms of one mode: self_mode x scaling (none, pre, pre with edge_scale) x post x val, as dicts of flags."""
    out = []
    for sm, scale, post, val in itertools.product(self_modes, ("none", "pre", "edge"), (False, True), (False, True)):
        out.append(dict(self_mode=sm, scale=scale, post=post, val=val))
    return out


def form_kwargs(form, pre, post, val):
    """The keyword arguments of ``spmm`` / ``ops.spmm_csr`` for one form over the given vectors."""
    kw = dict(self_mode=form["self_mode"])
    if form["scale"] != "none":
        kw.update(pre=pre, edge_scale=form["scale"] == "edge")
    if form["post"]:
        kw["post"] = post
    if form["val"]:
        kw["val"] = val
    return kw


def transpose(rowptr, col, val, n_cols):
    """The CSR of the transpose (columns ascending), values carried along."""
    rowptr, col = rowptr.to(torch.int64), col.to(torch.int64)
    n = rowptr.numel() - 1
    rowid = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    perm = torch.argsort(col * max(n, 1) + rowid)
    rp = torch.zeros(n_cols + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(torch.bincount(col, minlength=n_cols), 0)
    return rp, rowid[perm].to(torch.int32), None if val is None else val[perm]


# ---- float64 dense restatement: the check of the mirror itself ------------------------------------------------------------------
def dense64(rowptr, col, x, n_cols, pre=None, post=None, mode="sum", edge_scale=False, self_mode=0, val=None):
    """(ref, bound): the same operator as dense float64 algebra — the weights are float64 products of the float32 factors — and
    the elementwise first-order bound on |mirror - ref|: (T + 6) 2^-24 |post| Σ_t |w_t| |x_t| for sum and mean (T terms: T - 1
    additions, at most three roundings per weight and product, one for the mean, one for post), 3 · 2^-24 |post| |w x| of the
    winner for max."""
    rowptr, col = rowptr.to(torch.int64), col.to(torch.int64)
    n = rowptr.numel() - 1
    x = x.to(torch.float64)
    rowid = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    w = torch.ones(col.numel(), dtype=torch.float64)
    wself = torch.ones(n, dtype=torch.float64)
    if pre is not None:
        p64 = pre.to(torch.float64)
        w = p64[rowid] * p64[col] if edge_scale else p64[col].clone()
        wself = p64[:n] * p64[:n] if edge_scale else p64[:n].clone()
    if val is not None:
        w = w * val.to(torch.float64)
    mask = torch.zeros(n, n_cols, dtype=torch.bool)
    mask[rowid, col] = True
    W = torch.zeros(n, n_cols, dtype=torch.float64)
    W[rowid, col] = w
    if self_mode == 2:                                         # the loop, where there is one, is replaced by the self term
        d = torch.arange(n)
        mask[d, d] = False
        W[d, d] = 0.0
    T = mask.sum(1) + (1 if self_mode else 0)
    po = torch.ones(n, dtype=torch.float64) if post is None else post.to(torch.float64)
    u = 2.0 ** -24
    if mode == "max":
        c = torch.where(mask[:, :, None], W[:, :, None] * x[None], torch.full((), float("-inf"), dtype=torch.float64))
        best = c.amax(1) if n_cols else torch.full((n, x.shape[1]), float("-inf"), dtype=torch.float64)
        if self_mode:
            best = torch.maximum(best, wself[:, None] * x[:n])
        best = torch.where((T > 0)[:, None], best, torch.zeros((), dtype=torch.float64))
        return po[:, None] * best, 3 * u * po.abs()[:, None] * best.abs()
    s = W @ x
    mag = W.abs() @ x.abs()
    if self_mode:
        s = s + wself[:, None] * x[:n]
        mag = mag + wself.abs()[:, None] * x[:n].abs()
    if mode == "mean":
        s = s / T.clamp(min=1).to(torch.float64)[:, None]
    return po[:, None] * s, (T + 6).to(torch.float64)[:, None] * u * po.abs()[:, None] * mag
