"""The slot-pair form of the intersection pass (cn_flags.hip, NS = 2: a wave owns two consecutive processing slots;
``ocn_cn_flags_pair_min_batch``) against the one-slot form on the same inputs — every output is an integer, so every
comparison is ``torch.equal`` — and against the torch restatement of tests/test_flags_rec_gpu.py.

The graph has about 9 000 nodes (above ``ocn_cn_flags_small_graph_cols()``: the histogram goes to memory, the form that takes
pairs), sparse, with planted rows of 0, 1, 63, 64, 65, 130, 500, 600 and 1 100 entries that serve as source rows and, T1 being
A itself, as target rows: registers (<= 64), the wave's LDS slice whole (<= 1 024 beside a partner in registers), its half
(<= 512 beside a partner that needs LDS too), and the search in memory (> 512 beside such a partner, > 1 024 always).  T2 is
the pattern of A·A, as bit rows and — one scenario — as a CSR only (the sampled search and its shared slice).  Each scenario
is a batch of its own; with the prep pass's order and records (record-fed kernel) and in batch order (the kernel walks the
arrays), so that the pairs are the ones written down here."""
import pytest
import torch

from tests.test_flags_rec_gpu import _bit_rows, _expect

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N = 9000
DEG = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 130, 6: 500, 7: 600, 8: 1100}      # node -> planted row length
D0, D1, D63, D64, D65, D130, D500, D600, D1100 = range(9)
_G = {}


def _graph():
    """(A, T2) as (rowptr, col, rows): A random rows of 0 .. 19 entries and the planted ones, T2 = the pattern of A·A."""
    if not _G:
        g = torch.Generator().manual_seed(11)
        rows = []
        for r in range(N):
            d = DEG.get(r, int(torch.randint(0, 20, (1,), generator=g)))
            rows.append(torch.sort(torch.randperm(N, generator=g)[:d])[0].to(torch.int32))
        rowptr = torch.zeros(N + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(torch.tensor([r.numel() for r in rows]), 0)
        col = torch.cat(rows)
        ri = torch.repeat_interleave(torch.arange(N), rowptr[1:] - rowptr[:-1])
        a = torch.sparse_coo_tensor(torch.stack([ri, col.long()]), torch.ones(col.numel()), (N, N)).coalesce()
        a2 = torch.sparse.mm(a, a).coalesce().indices()                 # sorted by (row, col)
        cnt = torch.bincount(a2[0], minlength=N)
        rp2 = torch.zeros(N + 1, dtype=torch.int64)
        rp2[1:] = torch.cumsum(cnt, 0)
        col2 = a2[1].to(torch.int32)
        rows2 = list(torch.split(col2, cnt.tolist()))
        _G["A"] = (rowptr, col, rows)
        _G["T2"] = (rp2, col2, rows2)
        _G["bits2"] = _bit_rows(rows2, N)
        lens2 = cnt[torch.tensor(sorted(DEG))]
        assert int(lens2[D0]) == 0 and int(lens2.max()) > 64            # an empty A² row and sampled ones
    return _G["A"], _G["T2"], _G["bits2"]


def _random(B, seed):
    g = torch.Generator().manual_seed(seed)
    src, dst = torch.randint(0, N, (B,), generator=g), torch.randint(0, N, (B,), generator=g)
    k = min(B, 9)
    src[:k] = torch.randperm(9, generator=g)[:k]                        # planted rows among the sources ...
    dst[B - k:] = torch.randperm(9, generator=g)[:k]                    # ... and among the targets
    return src, dst


def _pairs(*p):
    return torch.tensor([s for s, _ in p]), torch.tensor([d for _, d in p])


# name -> (src, dst); in batch order slots 2g and 2g + 1 are rows 2g and 2g + 1
SCENARIOS = {
    "B1": _random(1, 1), "B2": _random(2, 2), "B7": _random(7, 7), "B8": _random(8, 8), "B9": _random(9, 9),
    "B41": _random(41, 41),
    "same_source": _pairs((D130, D64), (D130, D130), (D65, D500), (D65, 4000), (D1, D1), (D1, D63), (D600, D0), (D600, D600)),
    "unequal_sources": _pairs((D0, D130), (D130, D65), (D1, D500), (D1100, D130), (D63, D65), (D65, D63), (20, D600), (D500, 21)),
    "both_in_registers": _pairs((D130, D63), (D65, D64), (D500, D1), (D500, D0), (30, 31), (D64, 32)),
    "lds_beside_registers": _pairs((D130, D130), (D65, D64), (D64, D0), (D500, D600), (D63, D500), (D63, 40)),
    "both_in_lds": _pairs((D130, D130), (D130, D500), (D65, D500), (D500, D65), (D600, D65), (D1100, D130)),
    "above_half_beside_lds": _pairs((D130, D600), (D130, D130), (D500, D500), (D65, D600), (D600, D600), (D1100, D600)),
    "above_the_slice": _pairs((D130, D1100), (D130, D64), (D65, D130), (D500, D1100), (D1100, D1100), (D600, D1100), (D64, D1100)),
}


def _launch(lib, src, dst, mode, t2, pairs, cap=None):
    """One prep and one launch: pairs = the slot-pair form (bound 0) or the one-slot form (bound past any batch)."""
    from ocn_amd import ops
    P, S = ops.ptr, ops.stream_ptr
    A, T2, bits2 = _graph()
    B = src.numel()
    rowptrA, colA, src_d, dst_d = A[0].to(DEV), A[1].to(DEV), src.to(DEV), dst.to(DEV)
    rp2, c2 = (T2[0].to(DEV), T2[1].to(DEV)) if t2 == "csr" else (None, None)
    bm2 = bits2.to(DEV) if t2 == "bits" else None
    off = torch.empty(B + 1, dtype=torch.int64, device=DEV)
    sws = torch.zeros(int(lib.ocn_scan_workspace_bytes(B)) // 8 + 1, dtype=torch.int64, device=DEV)
    ows = torch.zeros(int(lib.ocn_order_workspace_bytes(N)) // 8 + 1, dtype=torch.int64, device=DEV)
    order = torch.empty(B, dtype=torch.int64, device=DEV) if mode == "rec" else None
    rec = torch.full((B, 4), -7, dtype=torch.int64, device=DEV)
    gcost = torch.full(((B + 3) // 4,), -7, dtype=torch.int32, device=DEV)
    if mode == "rec":
        ops.check(lib.ocn_batch_prep(P(rowptrA), P(src_d), B, P(off), P(sws), N, P(ows), None, None, 0, S()), "prep")
        ops.check(lib.ocn_order_by_node_finish_rec(P(src_d), P(dst_d), P(rowptrA), P(off), B, N, P(order), P(rec), P(ows), S()), "finish_rec")
    else:
        ops.check(lib.ocn_edge_offsets(P(rowptrA), P(src_d), B, P(off), P(sws), S()), "offsets")
    total = int(off[B])
    cap = total if cap is None else cap
    flags = torch.zeros(max(total, 1), dtype=torch.uint8, device=DEV)
    hist = torch.zeros(N, 2, dtype=torch.int64, device=DEV)
    cnt1 = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    cnt2 = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    fn = lib.ocn_cn_flags_rec if mode == "rec" else lib.ocn_cn_flags
    prev = ops.flags_pair_min_batch(0 if pairs else 1 << 40)
    try:
        ops.check(fn(P(rowptrA), P(colA), P(rowptrA), P(colA), P(rp2), P(c2), None, 0, P(bm2), bm2.shape[1] if bm2 is not None else 0,
                     P(src_d), P(dst_d), P(order), B, N, P(off), P(flags), cap, P(hist), P(cnt1), P(cnt2), P(status), P(rec),
                     P(gcost), S()), "flags")
        torch.cuda.synchronize()
    finally:
        ops.flags_pair_min_batch(prev)
    return dict(off=off.cpu(), order=order.cpu() if order is not None else torch.arange(B), flags=flags.cpu()[:total],
                hist=hist.cpu(), cnt1=cnt1.cpu(), cnt2=cnt2.cpu(), rec=rec.cpu(), gcost=gcost.cpu(), status=status.cpu())


def _both(lib, src, dst, mode, t2, cap=None):
    """The pair form and the one-slot form; the prep pass may order the slots of one source differently from run to run, so
    `rec` and `gcost` are compared where the two runs got the same order (always in batch order)."""
    for _ in range(4):
        two, one = _launch(lib, src, dst, mode, t2, True, cap), _launch(lib, src, dst, mode, t2, False, cap)
        if torch.equal(two["order"], one["order"]):
            break
    assert torch.equal(two["order"], one["order"])
    for k in ("off", "flags", "hist", "cnt1", "cnt2", "rec", "gcost", "status"):
        assert torch.equal(two[k], one[k]), k
    return two


def _against_the_restatement(out, src, dst, t2):
    A, T2, _ = _graph()
    flags, hist, cnt1, cnt2, rec, gcost = _expect(A, A, T2, src, dst, out["off"], out["order"], N, False)
    assert torch.equal(out["flags"], flags)
    assert torch.equal(out["hist"][:, 0], hist) and int(out["hist"][:, 1].abs().sum()) == 0
    assert torch.equal(out["cnt1"], cnt1) and torch.equal(out["cnt2"], cnt2)
    assert torch.equal(out["rec"], rec) and torch.equal(out["gcost"], gcost)
    assert int(out["status"].abs().sum()) == 0


@pytest.mark.parametrize("mode", ["rec", "none"])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_pairs_write_what_single_slots_write(hiplib, name, mode):
    assert N > hiplib.ocn_cn_flags_small_graph_cols() and hiplib.ocn_cn_flags_pair_min_batch(-1) == 32768
    src, dst = SCENARIOS[name]
    _against_the_restatement(_both(hiplib, src, dst, mode, "bits"), src, dst, "bits")


@pytest.mark.parametrize("name", ["B41", "lds_beside_registers", "both_in_lds"])
def test_pairs_with_t2_as_csr_only(hiplib, name):
    """No bit rows: the pair shares the wave's 64-entry T2 slice — whole (a 64-point sample of a long row, or a short row)
    beside an empty A² row (dst = the node without neighbours), a half for a row of <= 32 entries, the search in memory
    otherwise."""
    src, dst = SCENARIOS[name]
    for mode in ("rec", "none"):
        _against_the_restatement(_both(hiplib, src, dst, mode, "csr"), src, dst, "csr")


def test_flag_capacity_that_only_the_first_slot_fits(hiplib):
    """flags_cap between the two slots' ends: the first slot's flags are written, the second's are not, the counts are whole
    and the status words say OCN_ST_CAP — as the one-slot form does it."""
    A, T2, _ = _graph()
    src, dst = _pairs((D65, D64), (D130, D65), (D500, D130))
    for mode in ("rec", "none"):
        out = _both(hiplib, src, dst, mode, "bits", cap=100)
        assert torch.equal(out["order"], torch.arange(3))                  # (sources ascending: the order is the batch's)
        flags, hist, cnt1, cnt2, _, _ = _expect(A, A, T2, src, dst, out["off"], out["order"], N, False)
        assert int(flags[65:].sum()) > 0                                   # (there was something to leave out)
        assert torch.equal(out["flags"][:65], flags[:65]) and int(out["flags"][65:].abs().sum()) == 0
        assert torch.equal(out["hist"][:, 0], hist) and torch.equal(out["cnt1"], cnt1) and torch.equal(out["cnt2"], cnt2)
        assert int(out["status"][0]) == 1 and int(out["status"][3]) == 1
