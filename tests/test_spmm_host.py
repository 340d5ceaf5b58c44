"""The CPU mirror of the encoder SpMM (tests/spmm_mirror.py) checked without a GPU: hand-derived sums whose float32 value depends
on where the self term stands, the mean's denominators, every form against a float64 dense restatement within a first-order
bound, the fixed graph's stated properties, and the wrappers' refusal of a ``pre`` that ``edge_scale`` would read past."""
import pytest
import torch

from tests import spmm_mirror as M

BIG = float(2 ** 24)


def _one_row(n, r, cols):
    return M.csr_from_rows([sorted(cols) if i == r else [] for i in range(n)])


def _order_x(r):
    x = torch.full((8, 16), 0.5)
    x[r] = BIG
    return x


# ---- hand-derived order cases: x = 0.5 everywhere, x[r] = 2^24 (float32 spacing 2 above it, ties to even) ----------------------------
def test_self_term_position_decides_the_sum():
    """Row 3 = {0,1,2,4,5,6,7}.  At the diagonal's sorted place: 1.5 + 2^24 -> 16777218, four more halves change nothing.  After
    the neighbours: 3.5 + 2^24 = 16777219.5 -> 16777220.  Self first would give 16777216."""
    rowptr, col = _one_row(8, 3, [0, 1, 2, 4, 5, 6, 7])
    x = _order_x(3)
    assert torch.equal(M.spmm(rowptr, col, x, self_mode=2)[3], torch.full((16,), 16777218.0))
    assert torch.equal(M.spmm(rowptr, col, x, self_mode=1)[3], torch.full((16,), 16777220.0))
    assert torch.equal(M.spmm(rowptr, col, x, self_mode=0)[3], torch.full((16,), 3.5))


def test_self_term_one_entry_late_would_show():
    """Row 2 = {0,1,3,4,5,6,7}: 1.0 + 2^24 = 16777217 is a tie and goes to the even 16777216, where every further half is lost.  With
    the self term one entry late the prefix is 1.5 and the sum 16777218.  Row 0 = {1,2,3}: the self term comes first, 16777216;
    row 7 = {1,2,3}: no column >= 7, the self term comes last, 1.5 + 2^24 -> 16777218."""
    rowptr, col = _one_row(8, 2, [0, 1, 3, 4, 5, 6, 7])
    assert torch.equal(M.spmm(rowptr, col, _order_x(2), self_mode=2)[2], torch.full((16,), 16777216.0))
    rowptr, col = _one_row(8, 0, [1, 2, 3])
    assert torch.equal(M.spmm(rowptr, col, _order_x(0), self_mode=2)[0], torch.full((16,), 16777216.0))
    rowptr, col = _one_row(8, 7, [1, 2, 3])
    assert torch.equal(M.spmm(rowptr, col, _order_x(7), self_mode=2)[7], torch.full((16,), 16777218.0))


def test_explicit_loop_is_replaced_in_place_and_doubled_after():
    """Row 3 = {0,...,7}, its own id included.  self_mode=2 still gives 16777218: the loop is replaced.  self_mode=1 adds x[3] twice:
    1.5 + 2^24 -> 16777218, four halves lost, + 2^24 = 33554434, a tie at spacing 4 -> 33554432.  self_mode=0 takes the loop as an
    entry: 16777218."""
    rowptr, col = _one_row(8, 3, range(8))
    x = _order_x(3)
    assert torch.equal(M.spmm(rowptr, col, x, self_mode=2)[3], torch.full((16,), 16777218.0))
    assert torch.equal(M.spmm(rowptr, col, x, self_mode=1)[3], torch.full((16,), 33554432.0))
    assert torch.equal(M.spmm(rowptr, col, x, self_mode=0)[3], torch.full((16,), 16777218.0))
    # weighted: the replaced loop takes the SELF weight, not the entry's value
    val = torch.full((8,), 2.0)
    xs = torch.ones(8, 16)
    assert torch.equal(M.spmm(rowptr, col, xs, self_mode=2, val=val)[3], torch.full((16,), 15.0))      # 7 * 2 + 1
    assert torch.equal(M.spmm(rowptr, col, xs, self_mode=1, val=val)[3], torch.full((16,), 17.0))      # 8 * 2 + 1


# ---- mean counts -------------------------------------------------------------------------------------------------------------------
def test_mean_divides_by_the_terms_it_added():
    """x[k] = k + 1 in every feature.  Rows: 1 = {0,4,6} (no loop), 3 = {1,3,5,7} (a loop), 5 = {} (empty)."""
    rows = [[], [0, 4, 6], [], [1, 3, 5, 7], [], [], [], []]
    rowptr, col = M.csr_from_rows(rows)
    x = (torch.arange(8, dtype=torch.float32) + 1)[:, None].repeat(1, 16)

    def mean(sm):
        return M.spmm(rowptr, col, x, mode="mean", self_mode=sm)[:, 0].tolist()

    f = lambda a, b: (torch.tensor(float(a)) / torch.tensor(float(b))).item()       # noqa: E731 (one float32 division)
    m0, m1, m2 = mean(0), mean(1), mean(2)
    assert m0[1] == f(1 + 5 + 7, 3) and m1[1] == f(1 + 5 + 7 + 2, 4) and m2[1] == f(1 + 2 + 5 + 7, 4)      # entries + 1
    assert m0[3] == f(2 + 4 + 6 + 8, 4) and m1[3] == f(2 + 4 + 6 + 8 + 4, 5)
    assert m2[3] == f(2 + 4 + 6 + 8, 4)                                            # the loop replaced: the entries, no more
    assert m0[5] == 0.0                                                            # no term: divided by 1
    assert m1[5] == 6.0 and m2[5] == 6.0                                           # the self term alone, divided by 1
    assert M.spmm(rowptr, col, x, mode="max")[5, 0].item() == 0.0                  # max of an empty row
    assert M.spmm(rowptr, col, x, mode="max", self_mode=1)[5, 0].item() == 6.0
    _, count = M.term_layout(rowptr, col, 2)
    assert count.tolist() == [1, 4, 1, 4, 1, 1, 1, 1]


# ---- the fixed graph is what its description says ---------------------------------------------------------------------------------
def test_fixed_graph_has_the_stated_rows():
    g = M.fixed_graph()
    rows = g["rows"]
    assert len(rows) == 261 and all(261 % k for k in (4, 8, 16, 32, 64))
    assert [len(c) for c in rows] == [M.LENGTHS[r % 23] for r in range(261)]
    for lpe in (4, 8, 16, 32, 64):
        assert {lpe - 1, lpe, lpe + 1, 2 * lpe, 2 * lpe + 1} <= set(M.LENGTHS)
    assert {k % 4 for k in M.LENGTHS} == {0, 1, 2, 3} and max(M.LENGTHS) > 3 * 64
    assert all(c == sorted(set(c)) and (not c or (0 <= c[0] and c[-1] < 261)) for c in rows)
    filled = [r for r in range(261) if rows[r]]
    assert all(filled[i] in rows[filled[i]] for i in range(2, len(filled), 3))     # every third non-empty row holds its own id
    kinds = set()
    for r, c in enumerate(rows):
        if c:
            kinds.add("equal" if c == [r] else "below" if c[-1] < r else "above" if c[0] > r else "straddle")
            kinds.add("loop" if r in c else "no loop")
    assert kinds == {"equal", "below", "above", "straddle", "loop", "no loop"}
    assert 9000 < g["col"].numel() < 12000 and g["val"].numel() == g["col"].numel()
    assert float(g["pre"].min()) >= 0.1 and float(g["post"].min()) >= 0.1 and not torch.equal(g["pre"], g["post"])
    assert len(M.forms()) == 36


# ---- every form against float64 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", M.MODES)
def test_mirror_within_first_order_bound_of_float64(mode):
    g = M.fixed_graph()
    x = M.fixed_x(16)
    worst = 0.0
    for form in M.forms():
        kw = M.form_kwargs(form, g["pre"], g["post"], g["val"])
        got = M.spmm(g["rowptr"], g["col"], x, mode=mode, **kw)
        ref, bound = M.dense64(g["rowptr"], g["col"], x, 261, mode=mode, **kw)
        err = (got.to(torch.float64) - ref).abs()
        live = bound > 0
        if live.any():
            worst = max(worst, float((err[live] / bound[live]).max()))
        assert bool((err <= bound).all()), (mode, form, float((err - bound).max()))
    print(f"{mode}: worst |mirror - ref64| / bound over 36 forms = {worst:.3f}")
    assert worst > 0.0                                                             # (the comparison saw roundings at all)


def test_deg_rsqrt_mirror():
    rowptr = torch.tensor([0, 0, 3, 11, 14])
    assert M.deg_rsqrt(rowptr, 1.0).tolist() == [1.0, 0.5, (torch.tensor(1.0) / torch.tensor(3.0)).item(), 0.5]
    assert M.deg_rsqrt(rowptr, 0.0)[0].item() == 0.0                               # d <= 0 -> 0
    val = torch.ones(14)
    val[11] = BIG                                          # sequential float32: 2^24 + 1 + 1 stays 2^24; 1 + 1 + 2^24 would not
    assert M.deg_rsqrt(rowptr, 0.0, val=val)[3].item() == 2.0 ** -12
    g = M.fixed_graph()
    for add in (1.0, 0.0):
        got = M.deg_rsqrt(g["rowptr"], add, val=g["val"]).to(torch.float64)
        deg = torch.zeros(261, dtype=torch.float64).index_add_(
            0, torch.repeat_interleave(torch.arange(261), g["rowptr"][1:] - g["rowptr"][:-1]), g["val"].to(torch.float64))
        d = add + deg
        ref = torch.where(d > 0, 1.0 / torch.sqrt(d.clamp(min=1e-30)), torch.zeros((), dtype=torch.float64))
        # <= 200 additions, the sqrt (halves the relative error), the division
        assert bool(((got - ref).abs() <= (0.5 * 201 + 2) * 2.0 ** -24 * ref).all())
        assert (got == 0).sum().item() == (12 if add == 0.0 else 0)                # the empty rows: r % 23 == 0


def test_root_and_reciprocal_are_correctly_rounded():
    """sqrt32 / recip32 against the definition in exact integer arithmetic: float32 values are integers times a power of two, so
    (2s ∓ ulp)² <> 4d and |2^k - q s| compare as Python integers."""
    from fractions import Fraction
    g = torch.Generator().manual_seed(5)
    d = torch.cat([torch.arange(1, 300, dtype=torch.float32), torch.rand(700, generator=g) * 250 + 0.01,
                   torch.tensor([2.0 ** -20, 3e-30, 2.0 ** 40, 16777215.0])])
    s = M.sqrt32(d)
    q = M.recip32(s)
    inf = torch.tensor(float("inf"))
    for dv, sv, qv in zip(d.tolist(), s.tolist(), q.tolist()):
        D, S, Q = Fraction(dv), Fraction(sv), Fraction(qv)
        s_dn, s_up = Fraction(torch.nextafter(torch.tensor(sv), -inf).item()), Fraction(torch.nextafter(torch.tensor(sv), inf).item())
        assert ((S + s_dn) / 2) ** 2 < D < ((S + s_up) / 2) ** 2, dv
        q_dn, q_up = Fraction(torch.nextafter(torch.tensor(qv), -inf).item()), Fraction(torch.nextafter(torch.tensor(qv), inf).item())
        assert abs(1 - Q * S) < min(abs(1 - q_dn * S), abs(1 - q_up * S)), sv
    assert M.sqrt32(torch.tensor([4.0, 9.0, 34.0])).tolist() == [2.0, 3.0, float.fromhex("0x1.752e50p+2")]


def test_transpose_mirror():
    g = M.fixed_graph()
    rp, cl, vl = M.transpose(g["rowptr"], g["col"], g["val"], 261)
    dense = torch.zeros(261, 261)
    rowid = torch.repeat_interleave(torch.arange(261), g["rowptr"][1:] - g["rowptr"][:-1])
    dense[rowid, g["col"].long()] = g["val"]
    back = torch.zeros(261, 261)
    back[torch.repeat_interleave(torch.arange(261), rp[1:] - rp[:-1]), cl.long()] = vl
    assert torch.equal(back, dense.t())
    assert all(cl[rp[r]:rp[r + 1]].tolist() == sorted(cl[rp[r]:rp[r + 1]].tolist()) for r in range(261))


# ---- the wrappers refuse a pre that edge_scale would read past ----------------------------------------------------------------------
def test_wrappers_refuse_edge_scale_on_an_operator_taller_than_pre(monkeypatch):
    """``pre`` lives in the operator's COLUMN space (one entry per row of x); ``edge_scale`` also reads pre[r] for every output
    row r, so the operator may not have more rows than x."""
    from ocn_amd import ops
    monkeypatch.setattr(ops, "_req", lambda t, dtype, name, ndim=None: t)
    rowptr = torch.tensor([0, 1, 2, 2, 3])                                       # 4 rows over 3 columns
    col = torch.tensor([1, 0, 2], dtype=torch.int32)
    x, pre = torch.zeros(3, 16), torch.ones(3)
    with pytest.raises(ValueError, match="edge_scale"):
        ops.spmm_csr(rowptr, col, x, pre=pre, edge_scale=True)
    with pytest.raises(ValueError, match="edge_scale"):
        ops.spmm_csr_rows(rowptr, col, x, torch.tensor([0, 3]), pre=pre, edge_scale=True)
    with pytest.raises(ValueError, match="square operator"):
        ops.spmm_csr(rowptr, col, x, pre=pre, self_mode=1)
    with pytest.raises(ValueError, match="pre must have one entry per row of x"):
        ops.spmm_csr(rowptr, col, x, pre=torch.ones(4))                            # the row count is the wrong length for pre
