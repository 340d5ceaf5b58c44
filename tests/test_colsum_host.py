"""CPU suite: the numpy mirror of the order-exact column sums (tests/colsum_mirror.py) against the oracle, its constants
against colsum.hip, and the hand-fed cases of tests/test_colsum_gpu.py against the conditions that make them worth running —
all of them conditions on the reference alone."""
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import ocn_oracle as O
from ocn_amd import ops
from ocn_amd.synth import chung_lu_graph, sample_edges
from tests import colsum_cases as C
from tests import colsum_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------
# the mirror is the oracle's arithmetic
# ---------------------------------------------------------------------------------------------
def _golden_graph():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "order_sensitive_colsum.json")))
    adj = O.to_symmetric(O.from_edge_index(torch.tensor(g["undirected_edges"]).t(), g["n"]))
    return adj, torch.tensor(g["batch"]).t().contiguous(), (g["innerprod"], 0.37)


def _random_graph():
    n = 90
    adj = O.to_symmetric(O.from_edge_index(chung_lu_graph(n, 7.0, 40, seed=3, clique_frac=0.4, window=24), n))
    return adj, sample_edges(adj.row, adj.col, n, 160, seed=4), (0.37, -3.0, 250.0)


def _mirror_inputs(adj, e, cn1, cn2, cn3=None, valued=False):
    """The arrays ops.cn_colsum_exact takes, from the oracle's matrices: flags in position order (row e of the batch, p-th
    neighbour of its source)."""
    Ei = O.row_select(adj, e[0])
    key = O.spm2elem(Ei).numpy()                                     # sorted by (row, col): index == flag position
    where = lambda m: np.searchsorted(key, O.spm2elem(m).numpy())
    flagsA = np.zeros(key.size, np.uint8)
    flagsA[where(cn1)] |= M.F_CN1
    flagsA[where(cn2)] |= M.F_CN2
    flagsB = wc = None
    if cn3 is not None:
        flagsB = np.zeros(key.size, np.uint8)
        flagsB[where(cn3)] = M.F_CN1
    if valued:
        wc = np.zeros(key.size, np.int32)
        wc[where(cn2)] = cn2.val.numpy().astype(np.int32)
    rowptr = adj.rowptr().numpy()
    off = np.zeros(e.shape[1] + 1, np.int64)
    np.cumsum(np.diff(rowptr)[e[0].numpy()], out=off[1:])
    hist = M.hist_of_flags(Ei.col.numpy(), flagsA, wc, adj.n_cols)
    return rowptr, adj.col.numpy().astype(np.int32), e[0].numpy(), off, flagsA, flagsB, wc, hist


def _or_one(s):
    """The reference's fix-up after the sum (model.py:2409, :2917); an unwritten column is 0 in the mirror."""
    return np.where(s == 0, np.float32(1), s)


@pytest.mark.parametrize("graph", [_golden_graph, _random_graph])
def test_mirror_equals_the_oracle(graph):
    """S2 of cn5, S2 / S3 of cn6 and S2 of the walk-count route, bit for bit, from flags built out of the oracle's own
    cn1 / cn2 / cn3 matrices."""
    adj, e, ips = graph()
    a2 = O.adj2_sparse(adj)
    cn1, cn2 = O.adjoverlap(adj, adj, e), O.adjoverlap(adj, a2, e)
    cn3 = O.adjoverlap(adj, O.adj3_sparse(adj, a2), e)
    w1, w2 = O.get_cn1_cn2(adj, e)
    x = torch.zeros(adj.n_rows, 1)
    assert (w2.val > 1).any() or graph is _golden_graph
    for ip in ips:
        tip = torch.tensor([ip])
        got = M.colsum(*_mirror_inputs(adj, e, cn1, cn2), ip)
        assert np.array_equal(M.bits(_or_one(got.s2)), M.bits(O.cn5_pool(x, cn1, cn2, tip)[2]["S2"].numpy()))
        got = M.colsum(*_mirror_inputs(adj, e, w1, w2, valued=True), ip)
        assert np.array_equal(M.bits(_or_one(got.s2)), M.bits(O.cn5_pool(x, w1, w2, tip)[2]["S2"].numpy()))
        got = M.colsum(*_mirror_inputs(adj, e, cn1, cn2, cn3), ip)
        aux = O.cn6_pool(x, cn1, cn2, cn3, tip)[3]
        assert np.array_equal(M.bits(_or_one(got.s2)), M.bits(aux["S2"].numpy()))
        assert np.array_equal(M.bits(_or_one(got.s3)), M.bits(aux["S3"].numpy()))
        assert got.nip == np.float32(aux["nip"].item())


def test_mirror_knows_the_golden_column():
    """tests/golden/order_sensitive_colsum.json: 2^25 in the reference's order, 2^25 + 4 with the ones first."""
    adj, e, (ip, _) = _golden_graph()
    cn1, cn2 = O.adjoverlap(adj, adj, e), O.adjoverlap(adj, O.adj2_sparse(adj), e)
    inp = _mirror_inputs(adj, e, cn1, cn2)
    assert M.colsum(*inp, ip).s2[0] == 33554432.0
    assert M.colsum(*inp, ip, order=lambda L: np.array([1, 2, 3, 0, 4])).s2[0] == 33554436.0


def test_mirror_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "ocn_amd", "csrc", "colsum.hip")).read()
    for name in ("CS_WAVE_MAX", "CS_MED_MAX", "CS_LDS", "CS_CHUNK", "CS_BINS", "CS_BIN_MAX"):
        m = re.findall(r"(?:#define\s+%s\s+|constexpr\s+int\s+%s\s*=\s*)(\d+)" % (name, name), src)
        assert len(m) == 1 and int(m[0]) == getattr(M, name), name
    hdr = open(os.path.join(ROOT, "include", "ocn_hip.h")).read()
    assert int(re.search(r"#define\s+OCN_F_CN1\s+(\d+)u", hdr).group(1)) == M.F_CN1
    assert int(re.search(r"#define\s+OCN_F_CN2\s+(\d+)u", hdr).group(1)) == M.F_CN2
    assert ops.HIST_FIELD_BITS == M.HIST_FIELD_BITS
    rng = np.random.default_rng(0)
    cnt = rng.integers(0, 1 << 21, (50, 4))
    hist = M.hist_pack(*cnt.T)
    assert np.array_equal(ops.hist_counts(torch.from_numpy(hist)).numpy(), cnt)


# ---------------------------------------------------------------------------------------------
# the cases are what they claim to be
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", C.VARIANTS)
def test_ladder_has_every_length(variant):
    case = C.ladder(variant)
    ref = M.colsum(*C.args(case), C.INNERPRODS[0])
    n1, n2, nu, _ = M.hist_counts(case.hist)
    assert tuple(ref.length[:len(C.LADDER)]) == C.LADDER and case.B == C.LADDER_B and case.flagsA.size == case.off[-1]
    assert n1[n1 >= 2].min() == 3 and ref.nip == np.float32(C.INNERPRODS[0]) / (np.float32(1) / np.float32(3))
    x = C.LADDER_EXTRA
    assert case.hist[x["untouched"], 0] == 0 and ref.length[x["untouched"]] == 0 and not ref.written[x["untouched"]]
    assert n1[x["closed"]] == 0 and n2[x["closed"]] > 0
    assert ref.length[x["early"]] == 70
    k, pos = M.union_entries(*C.args(case)[:6])
    assert pos[k == x["early"]].max() < case.off[min(cut[1] for cut in C.SHARD_CUTS)]
    if variant == "cn6":
        assert ref.ordered[:case.K][ref.length[:case.K] > 0].all() and ref.length[x["b_only"]] == 30 and nu[x["b_only"]] == 0
        assert ref.s2[x["b_only"]] == 0 and ref.s3[x["b_only"]] == 30
        outside = np.bincount(k[case.flagsA[pos] == 0], minlength=case.N)       # entries of the wider union alone
        assert (outside[:len(C.LADDER)][np.array(C.LADDER) >= 63] > 0).all()
        assert (nu[:len(C.LADDER)] < np.array(C.LADDER))[np.array(C.LADDER) >= 63].all()
    else:
        assert not ref.ordered[x["closed"]] and ref.written[x["closed"]]
        assert ref.s2[x["closed"]] == (M.hist_counts(case.hist)[3] if variant == "valued" else n2)[x["closed"]]
        assert case.hist[x["b_only"], 0] == 0 and not ref.written[x["b_only"]]
        assert ref.ordered[:len(C.LADDER)][np.array(C.LADDER) >= 3].all() and not ref.ordered[:2].any()
        assert np.array_equal(nu[:len(C.LADDER)], C.LADDER)


def _same_as_ascending(case, ip, order, ref):
    """The ordered case columns of 63 or more entries whose sums do NOT change when added in ``order``."""
    cols = np.flatnonzero(ref.ordered & (ref.length >= 63))
    assert cols.size
    alt = M.colsum(*C.args(case), ip, order=order)
    same = M.bits(alt.s2)[cols] == M.bits(ref.s2)[cols]
    if case.variant == "cn6":
        same |= M.bits(alt.s3)[cols] == M.bits(ref.s3)[cols]
    return ref.length[cols[same]].tolist()


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_ladder_and_layout_columns_discriminate(layout, variant):
    """Every ordered column of 63 or more entries, at every innerprod the GPU test uses: the sum (S2, and S3 in cn6) in
    descending order, with the halves swapped and with every aligned run of 64 reversed differs in bits from the ascending
    one — a kernel that ranked such a column wrongly in one of these ways could not pass."""
    case = C.layout_case(variant, layout)
    for ip in C.INNERPRODS:
        ref = M.colsum(*C.args(case), ip)
        for order in C.WRONG_ORDERS:
            assert _same_as_ascending(case, ip, order, ref) == [], (ip, order.__name__)


@pytest.mark.parametrize("variant", ("plain", "cn6"))
def test_many_columns_discriminate(variant):
    case = C.many(variant)
    ref = M.colsum(*C.args(case), C.MANY_IP)
    lengths = ref.length[:case.K - 1]
    assert ((lengths >= 513) & (lengths <= 600)).sum() == 1000 and ((lengths >= 65) & (lengths <= 70)).sum() == 5000
    assert ref.ordered[:case.K].all() and len(set(M.bits(ref.s2)[:case.K - 1].tolist())) > 300       # (448 streams of values)
    for order in C.WRONG_ORDERS:
        assert _same_as_ascending(case, C.MANY_IP, order, ref) == [], order.__name__


def test_layouts_reach_both_lds_sorts():
    """The test's own bin rule (position * CS_BINS // capacity) on the columns of 513 .. 4096 entries: "even" and "full" stay
    within CS_BIN_MAX per bin (the bucket sort — "full" with bins of exactly CS_BIN_MAX), "tail", "rows" and "over" exceed it
    (the bitonic network — "over" by one)."""
    want = {"even": lambda m: m <= M.CS_BIN_MAX // 2, "full": lambda m: m == M.CS_BIN_MAX, "over": lambda m: m == M.CS_BIN_MAX + 1,
            "rows": lambda m: m > M.CS_BIN_MAX, "tail": lambda m: m > M.CS_BIN_MAX}
    for variant in C.VARIANTS:
        for layout in C.LAYOUTS:
            case = C.layout_case(variant, layout)
            ref = M.colsum(*C.args(case), C.INNERPRODS[0])
            cols = C.lds_sorted_columns(case, ref)
            assert sorted(ref.length[cols]) == sorted(C.LDS_SORTED if layout in ("even", "tail", "rows") else C.FULL_BINS)
            assert all(want[layout](C.bin_occupancy(case, c)) for c in cols), layout
            if layout == "tail":
                assert case.flagsA.size == 64 * case.off[-1] and not case.flagsA[case.off[-1]:].any()


@pytest.mark.parametrize("variant", ("plain", "valued"))
def test_mirror_chains_through_edge_shards(variant):
    """The mirror's own s2_init: the ladder split into 2 and into 3 contiguous row ranges, chained from zeros, ends with the
    single call's bits; the "early" column is complete after the first shard and has no entry in the later ones."""
    case = C.ladder(variant)
    for ip in C.INNERPRODS:
        ref = M.colsum(*C.args(case), ip)
        for cuts in C.SHARD_CUTS:
            run = np.zeros(case.N, np.float32)
            for i, rows in enumerate(zip(cuts[:-1], cuts[1:])):
                part = M.colsum(*C.args(case, rows), ip, s2_init=run)
                run = part.s2
                early = C.LADDER_EXTRA["early"]
                assert part.length[early] == (70 if i == 0 else 0) and M.bits(run)[early] == M.bits(ref.s2)[early]
            touched = case.hist[:, 0] != 0
            assert np.array_equal(M.bits(run)[touched], M.bits(ref.s2)[touched]) and not run[~touched].any()


def test_two24_case():
    case = C.two24()
    n1, _, _, walks = M.hist_counts(case.hist)
    assert n1.max() == 1 and walks[0] == (1 << 24) - 1 and walks[1] >= 1 << 24
    ref = M.colsum(*C.args(case), 0.37)
    assert ref.nip == np.float32(0.37) and not ref.ordered[0] and ref.ordered[1] and ref.length[1] == 20
    assert ref.s2[0] == float((1 << 24) - 1)
    k, pos = M.union_entries(*C.args(case)[:6])
    acc = np.float32(0)
    for w in case.wc[pos[k == 1]]:
        acc = acc + np.float32(w)
    assert ref.s2[1] == acc and acc != np.float32(walks[1])              # the sequential sum, not the rounded integer
    for order in C.WRONG_ORDERS[:2]:
        assert M.colsum(*C.args(case), 0.37, order=order).s2[1] != acc


@pytest.mark.parametrize("variant", ("plain", "valued"))
def test_singletons_case(variant):
    case = C.singletons(variant)
    n1, n2, nu, walks = M.hist_counts(case.hist)
    assert n1.max() == 1 and nu.max() > M.CS_MED_MAX
    ref = M.colsum(*C.args(case), 0.37)
    assert ref.nip == np.float32(0.37) and not ref.ordered.any()
    assert np.array_equal(ref.s2, (walks if variant == "valued" else n2).astype(np.float32))
    assert np.array_equal(ref.written, case.hist[:, 0] != 0)
