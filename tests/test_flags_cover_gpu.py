"""The intersection pass with a certified T2 (``ocn_cn_flags_cover``, t2_cover = 1: T2 is the full pattern of A·A and A is
symmetric, so a candidate that is a stored entry of A reads no T2) against the same call with the certificate off — every
output is an integer, so every comparison is ``torch.equal`` — and against the torch restatement of tests/test_flags_rec_gpu.py.

The graph is symmetric, about 9 000 nodes (above ``ocn_cn_flags_small_graph_cols()``: the histogram goes to memory), with planted
source rows of 0, 1, 63, 64, 65, 130, 500, 600, 1 100 and 4 200 entries: one chunk (the ballot over the chunk), several chunks
(the two-level search: da / 64 not whole, a segment of 2 .. 18 entries) and a row past 4 096 entries, which ignores the
certificate.  The planted nodes neighbour ordinary nodes only, so their row lengths are exact.  T2 is the pattern of A·A built
on the CPU (an OR of A's bit rows), as bit rows and as a CSR only.  A second graph of 1 500 columns takes the LDS-histogram
form.  Each batch is prepared ONCE (offsets, order, records) and the kernel run on copies of that state with the certificate
on and off, in the record-fed and in the array order, with one and with two slots per wave."""
import numpy as np
import pytest
import torch

from tests.test_flags_rec_gpu import _bit_rows, _expect

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BIG = dict(n=9000, deg=[0, 1, 63, 64, 65, 130, 500, 600, 1100, 4200], seed=11)
SMALL = dict(n=1500, deg=[0, 1, 63, 64, 65, 130, 500], seed=12)          # <= 8 192 columns: the LH form
_G = {}


def _graph(spec):
    """dict(A=(rowptr, col, rows), T2=(rowptr, col, rows), bits2, n, deg): node q < len(deg) has exactly deg[q] neighbours."""
    key = spec["n"]
    if key not in _G:
        n, deg = spec["n"], spec["deg"]
        P = len(deg)
        rng = np.random.default_rng(spec["seed"])
        u = [np.full(d, q, dtype=np.int64) for q, d in enumerate(deg)]
        v = [rng.choice(np.arange(P, n), d, replace=False).astype(np.int64) for d in deg]
        ru, rv = rng.integers(P, n, 3 * n), rng.integers(P, n, 3 * n)      # ordinary nodes: about six neighbours of their own
        u, v = np.concatenate(u + [ru[ru != rv]]), np.concatenate(v + [rv[ru != rv]])
        keys = np.unique(np.concatenate([u * n + v, v * n + u]))          # both directions, duplicate-free, sorted by (row, col)
        row, col = keys // n, (keys % n).astype(np.int32)
        cnt = np.bincount(row, minlength=n)
        assert cnt[:P].tolist() == list(deg)
        rowptr = torch.zeros(n + 1, dtype=torch.int64)
        rowptr[1:] = torch.from_numpy(np.cumsum(cnt))
        rows = list(torch.split(torch.from_numpy(col), cnt.tolist()))
        bits = _bit_rows(rows, n)
        b8 = bits.numpy().view(np.uint8)                                   # [n][4 * words]
        t8 = np.zeros_like(b8)
        for j in range(n):
            if cnt[j]:
                t8[j] = np.bitwise_or.reduce(b8[rows[j].numpy()], axis=0)  # row j of A·A = the union of the rows of N(j)
        rows2 = [torch.from_numpy(np.flatnonzero(np.unpackbits(t8[j], bitorder="little")[:n]).astype(np.int32)) for j in range(n)]
        rp2 = torch.zeros(n + 1, dtype=torch.int64)
        rp2[1:] = torch.cumsum(torch.tensor([r.numel() for r in rows2]), 0)
        _G[key] = dict(A=(rowptr, torch.from_numpy(col), rows), T2=(rp2, torch.cat(rows2), rows2),
                       bits2=torch.from_numpy(t8.view("<i4").copy()), n=n, deg=list(deg), coo=(row, col.astype(np.int64)))
    return _G[key]


def _not_stored(gr, i, rng):
    """A target that is no neighbour of i: another planted node (their rows are long A² rows) or an ordinary one."""
    have = set(gr["A"][2][i].tolist())
    while True:
        j = int(rng.integers(0, gr["n"]))
        if j not in have and j != i:
            return j


def _planted(gr):
    """Per planted source row: stored targets at its first, last and a middle position, for rows of several chunks one inside
    chunk 0 and one outside it, and a target that is not stored — consecutive, so that in array order the slot pairs mix
    stored with not stored slots of one source."""
    rng = np.random.default_rng(5)
    out = []
    for i, d in enumerate(gr["deg"]):
        row = gr["A"][2][i].tolist()
        pos = [0, d - 1, d // 2] if d else []
        if d > 64:
            pos += [17, 64 + (d - 64) // 3]
        out += [(i, row[p]) for p in dict.fromkeys(pos)] + [(i, _not_stored(gr, i, rng))]
    return out


def _pair_cases(gr):
    """One source with (stored, not stored) and (not stored, stored), short and long rows; two sources; an odd tail."""
    rng = np.random.default_rng(6)
    out = []
    for i in (2, 4, 5, 6):                                                 # 63, 65, 130, 500 entries
        row = gr["A"][2][i].tolist()
        out += [(i, row[3]), (i, _not_stored(gr, i, rng)), (i, _not_stored(gr, i, rng)), (i, row[-2])]
    r5, r3, r1 = gr["A"][2][5].tolist(), gr["A"][2][3].tolist(), gr["A"][2][1].tolist()
    out += [(5, r5[70]), (3, r3[10]), (3, _not_stored(gr, 3, rng)), (6, gr["A"][2][6].tolist()[400]), (1, r1[0]), (0, 1)]
    out += [(5, r5[129])]                                                  # the odd tail
    return out


def _random(gr, B, seed):
    """B candidates, every other one a stored entry of A (drawn by entry: degree-biased), the rest random pairs."""
    rng = np.random.default_rng(seed)
    row, col = gr["coo"]
    pick = rng.integers(0, row.size, B)
    src, dst = rng.integers(0, gr["n"], B), rng.integers(0, gr["n"], B)
    src[::2], dst[::2] = row[pick[::2]], col[pick[::2]]
    return list(zip(src.tolist(), dst.tolist()))


def _scenarios(gr):
    if "scen" not in gr:
        sc = {"planted": _planted(gr), "pairs": _pair_cases(gr)}
        for B in range(1, 42):
            sc[f"B{B}"] = _random(gr, B, 100 + B)
        gr["scen"] = {k: (torch.tensor([s for s, _ in c]), torch.tensor([d for _, d in c])) for k, c in sc.items()}
        gr["expect"] = {}
    return gr["scen"]


def _prepared(lib, gr, src, dst, mode):
    """Offsets, and for the record-fed form the order and the half-written records, formed once per batch."""
    from ocn_amd import ops
    P, S = ops.ptr, ops.stream_ptr
    B, n = src.numel(), gr["n"]
    d = gr.setdefault("dev", {})
    if not d:
        d.update(rowptrA=gr["A"][0].to(DEV), colA=gr["A"][1].to(DEV), rp2=gr["T2"][0].to(DEV), c2=gr["T2"][1].to(DEV),
                 bm2=gr["bits2"].to(DEV))
    src_d, dst_d = src.to(DEV), dst.to(DEV)
    off = torch.empty(B + 1, dtype=torch.int64, device=DEV)
    sws = torch.zeros(int(lib.ocn_scan_workspace_bytes(B)) // 8 + 1, dtype=torch.int64, device=DEV)
    order, rec = None, torch.full((B, 4), -7, dtype=torch.int64, device=DEV)
    if mode == "rec":
        ows = torch.zeros(int(lib.ocn_order_workspace_bytes(n)) // 8 + 1, dtype=torch.int64, device=DEV)
        order = torch.empty(B, dtype=torch.int64, device=DEV)
        ops.check(lib.ocn_batch_prep(P(d["rowptrA"]), P(src_d), B, P(off), P(sws), n, P(ows), None, None, 0, S()), "prep")
        ops.check(lib.ocn_order_by_node_finish_rec(P(src_d), P(dst_d), P(d["rowptrA"]), P(off), B, n, P(order), P(rec), P(ows), S()),
                  "finish_rec")
    else:
        ops.check(lib.ocn_edge_offsets(P(d["rowptrA"]), P(src_d), B, P(off), P(sws), S()), "offsets")
    return dict(src=src_d, dst=dst_d, off=off, order=order, rec=rec, B=B, total=int(off[B]))


def _launch(lib, gr, prep, mode, t2, pairs, cover, bm2=None):
    """One launch on a copy of the prepared state.  t2: "bits" (bit rows; beside the CSR on the small graph, whose form reads
    the row lengths), "csr" (no bit rows)."""
    from ocn_amd import ops
    P, S = ops.ptr, ops.stream_ptr
    d, B, n = gr["dev"], prep["B"], gr["n"]
    small = n <= lib.ocn_cn_flags_small_graph_cols()
    rp2, c2 = (d["rp2"], d["c2"]) if (t2 == "csr" or small) else (None, None)
    bm2 = (d["bm2"] if bm2 is None else bm2) if t2 == "bits" else None
    flags = torch.zeros(max(prep["total"], 1), dtype=torch.uint8, device=DEV)
    hist = torch.zeros(n, 2, dtype=torch.int64, device=DEV)
    cnt1 = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    cnt2 = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    rec = prep["rec"].clone()
    gcost = torch.full(((B + 3) // 4,), -7, dtype=torch.int32, device=DEV)
    prev = ops.flags_pair_min_batch(0 if pairs else 1 << 40)
    try:
        ops.check(lib.ocn_cn_flags_cover(
            P(d["rowptrA"]), P(d["colA"]), P(d["rowptrA"]), P(d["colA"]), P(rp2), P(c2), None, 0, P(bm2),
            bm2.shape[1] if bm2 is not None else 0, P(prep["src"]), P(prep["dst"]), P(prep["order"]), B, n, P(prep["off"]), P(flags),
            prep["total"], P(hist), P(cnt1), P(cnt2), P(status), P(rec), P(gcost), int(mode == "rec"), int(cover), S()), "flags")
        torch.cuda.synchronize()
    finally:
        ops.flags_pair_min_batch(prev)
    return dict(flags=flags.cpu()[:prep["total"]], hist=hist.cpu(), cnt1=cnt1.cpu(), cnt2=cnt2.cpu(), rec=rec.cpu(),
                gcost=gcost.cpu(), status=status.cpu())


def _restated(gr, name, src, dst, prep):
    """The torch restatement, once per (batch, processing order)."""
    order = prep["order"].cpu() if prep["order"] is not None else torch.arange(prep["B"])
    key = (name, tuple(order.tolist()))
    if key not in gr["expect"]:
        gr["expect"][key] = _expect(gr["A"], gr["A"], gr["T2"], src, dst, prep["off"].cpu(), order, gr["n"], False)
    return gr["expect"][key]


def _on_off_and_restated(lib, gr, mode, t2, pairs):
    for name, (src, dst) in _scenarios(gr).items():
        prep = _prepared(lib, gr, src, dst, mode)
        on, off = _launch(lib, gr, prep, mode, t2, pairs, True), _launch(lib, gr, prep, mode, t2, pairs, False)
        for k in ("flags", "hist", "cnt1", "cnt2", "rec", "gcost", "status"):
            assert torch.equal(on[k], off[k]), (name, k)
        flags, hist, cnt1, cnt2, rec, gcost = _restated(gr, name, src, dst, prep)
        assert torch.equal(on["flags"], flags), name
        assert torch.equal(on["hist"][:, 0], hist) and int(on["hist"][:, 1].abs().sum()) == 0, name
        assert torch.equal(on["cnt1"], cnt1) and torch.equal(on["cnt2"], cnt2), name
        assert torch.equal(on["rec"], rec) and torch.equal(on["gcost"], gcost), name
        assert int(on["status"].abs().sum()) == 0, name


@pytest.mark.parametrize("t2", ["bits", "csr"])
@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("mode", ["rec", "none"])
def test_certified_equals_uncertified_and_the_restatement(hiplib, mode, pairs, t2):
    gr = _graph(BIG)
    assert gr["n"] > hiplib.ocn_cn_flags_small_graph_cols()
    _on_off_and_restated(hiplib, gr, mode, t2, pairs)


@pytest.mark.parametrize("t2", ["bits", "csr"])
@pytest.mark.parametrize("mode", ["rec", "none"])
def test_small_graph_form(hiplib, mode, t2):
    gr = _graph(SMALL)
    assert gr["n"] <= hiplib.ocn_cn_flags_small_graph_cols()
    _on_off_and_restated(hiplib, gr, mode, t2, False)


def _wedge(gr, i, p_j, far=False):
    """For the stored candidate (i, j = N(i)[p_j]): a neighbour k of i (its position p_k in N(i)) and a node i2 != i that has k
    but not j as a neighbour (k's position p2 in N(i2)) — (i2, j) is a not-stored candidate that probes the same bit."""
    row = gr["A"][2][i].tolist()
    j = row[p_j]
    cand = range(len(row) - 1, -1, -1) if far else range(len(row))
    for p_k in cand:
        k = row[p_k]
        if k == j:
            continue
        for i2 in gr["A"][2][k].tolist():
            r2 = gr["A"][2][i2].tolist()
            if i2 != i and i2 != j and j not in r2:
                return j, k, p_k, i2, r2.index(k)
    raise AssertionError("no such wedge")


@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("mode", ["rec", "none"])
def test_the_shortcut_is_taken_and_by_which_slots(hiplib, mode, pairs):
    """One wedge bit (j, k) of T2 cleared for a stored candidate (i, j), the now false certificate handed over: the certified
    run reports position k of N(i) as cn2 without looking, the uncertified run reads the cleared bit — for a one-chunk row
    (63 entries: the ballot) and for rows of several chunks (130 and 1 100 entries: the search; k in the last chunk).  The row
    of 4 200 entries ignores the certificate: both runs read the bit.  A not-stored candidate with the same target, whose
    source has k too, reads it in both runs, and so does the not-stored partner slot of the stored one."""
    gr = _graph(BIG)
    _scenarios(gr)
    rng = np.random.default_rng(9)
    for i, covered in ((2, True), (5, True), (8, True), (9, False)):
        d = gr["deg"][i]
        j, k, p_k, i2, p2 = _wedge(gr, i, d // 2, far=True)
        other = _not_stored(gr, i, rng)
        src, dst = torch.tensor([i, i, i2]), torch.tensor([j, other, j])       # slots 0, 1: one source — stored, not stored
        prep = _prepared(hiplib, gr, src, dst, mode)
        bm = gr["dev"]["bm2"].clone()
        assert (int(bm[j, k >> 5]) >> (k & 31)) & 1                           # the wedge j - i - k
        bm[j, k >> 5] &= ~(1 << (k & 31)) if (k & 31) != 31 else 0x7fffffff
        on, off = (_launch(hiplib, gr, prep, mode, "bits", pairs, c, bm2=bm) for c in (True, False))
        o = prep["off"].cpu()
        at = int(o[0]) + p_k
        assert int(off["flags"][at]) & 2 == 0
        assert (int(on["flags"][at]) & 2 != 0) == covered
        assert int(on["cnt2"][0]) - int(off["cnt2"][0]) == int(covered)
        for q in (1, 2):                                                       # not stored: the same in both runs
            assert torch.equal(on["flags"][int(o[q]):int(o[q + 1])], off["flags"][int(o[q]):int(o[q + 1])])
            assert int(on["cnt2"][q]) == int(off["cnt2"][q])
        assert int(on["flags"][int(o[2]) + p2]) & 2 == 0
