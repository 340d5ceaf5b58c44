"""Random-walk retrieval without a GPU: the CPU mirror against the answers pinned in the contract, its structure, the two
expectation identities on a small irregular graph, the header and the binding, and every refusal — of the C entries (before any
HIP call) and of the Python layer (before any device work)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import rw_mirror as RM
from tests import two_hop_sampling_mirror as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RW_ENTRIES = ("ocn_rw_max_walks", "ocn_rw_visits_count", "ocn_rw_visits_fill")


def k34():
    _, n, rows, _ = TM.hand_cases()[2]
    return (n, *TM.csr_of(n, rows))


def irregular():
    n = 8
    rows = TM.undirected(n, [(0, 1), (0, 2), (0, 3), (1, 4), (2, 4), (2, 5), (3, 5), (3, 6), (5, 6), (4, 7), (6, 7), (1, 2)])
    return n, rows, TM.csr_of(n, rows)


# ---- the mirror ----------------------------------------------------------------------------------------------------------
def test_pinned_answers_on_k34():
    n, rowptr, col = k34()
    assert RM.raw_counts(rowptr, col, 0, 2048, 3, 0) == ({0: 694, 1: 696, 2: 658}, {3: 526, 4: 507, 5: 506, 6: 509})
    assert RM.raw_counts(rowptr, col, 0, 2048, 3, 7) == ({0: 697, 1: 656, 2: 695}, {3: 519, 4: 550, 5: 491, 6: 488})
    ptr, edges, val, vis = RM.visits(rowptr, col, [0], 2048, 3, 0, decay=0.5)
    assert ptr.tolist() == [0, 2] and edges.tolist() == [[0, 1], [0, 2]] and vis.tolist() == [[696, 0], [658, 0]]
    assert val.dtype == np.float32 and val.tolist() == [696.0, 658.0]
    c2, c3 = RM.raw_counts(rowptr, col, 0, 2048, 2, 0)       # two steps: the same second steps, no third
    assert c2 == {0: 694, 1: 696, 2: 658} and c3 == {}


def test_the_vectorised_words_are_the_scalar_words():
    for seed, s in ((0, 0), ((1 << 64) - 1, 5), ((0x5EED << 32) | 0x4321, (1 << 31) - 1)):
        for length in (2, 3):
            got = RM.words(seed, s, 70, length)
            assert all(tuple(got[w]) == RM.words_one(seed, s, w, length) for w in (0, 1, 63, 64, 69))


def test_fewer_walks_are_a_prefix():
    """The counts of W' < W walks are the partial sums over w < W': a walk does not know how many there are."""
    n, rows, (rowptr, col) = irregular()
    seed, s = 3, 2
    want2, want3 = {}, {}
    marks = {}
    for w in range(300):
        u = RM.words_one(seed, s, w, 3)
        p = s
        for t in (1, 2, 3):
            p = rows[p][RM.mulhi(u[t - 1], len(rows[p]))]
            if t == 2:
                want2[p] = want2.get(p, 0) + 1
            if t == 3:
                want3[p] = want3.get(p, 0) + 1
        if w + 1 in (1, 100, 300):
            marks[w + 1] = (dict(want2), dict(want3))
    for W, want in marks.items():
        assert RM.raw_counts(rowptr, col, s, W, 3, seed) == want, W


def test_a_source_stands_alone():
    n, rows, (rowptr, col) = irregular()
    seg = {s: RM.source_segment(rowptr, col, s, 200, 3, 9, 0.25) for s in range(n)}
    for order in ([0, 1, 2], [2, 0], [5, 5, 0, 7, 5]):
        ptr, edges, val, vis = RM.visits(rowptr, col, order, 200, 3, 9, 0.25)
        for q, s in enumerate(order):
            got = [(int(e[1]), int(v[0]), int(v[1]), x) for e, v, x in zip(edges[ptr[q]:ptr[q + 1]], vis[ptr[q]:ptr[q + 1]], val[ptr[q]:ptr[q + 1]])]
            assert got == seg[s] and all(int(e[0]) == s for e in edges[ptr[q]:ptr[q + 1]])
    ids = [v for v, *_ in seg[0]]
    assert ids == sorted(ids) and 0 not in ids and not set(ids) & set(rows[0])


def test_value_is_two_roundings():
    d, c2, c3 = 0.3, 1001, 777
    want = np.float32(c2) + np.float32(np.float32(d) * np.float32(c3))
    assert RM.value(c2, c3, d, 3) == np.float32(want) and RM.value(c2, c3, None, 2) == np.float32(c2)
    assert float(RM.value(c2, c3, d, 3)) != c2 + d * c3      # (the roundings are visible)


def test_short_list_order():
    ptr = np.array([0, 5, 5, 7])
    edges = np.array([[0, 2], [0, 4], [0, 6], [0, 8], [0, 9], [3, 1], [3, 2]])
    val = np.array([1, 3, 3, 1, 2], dtype=np.float32).tolist() + [5.0, 5.0]
    p, e = RM.short_list(ptr, edges, np.array(val, dtype=np.float32), 3)
    assert p.tolist() == [0, 3, 3, 5] and e[:, 1].tolist() == [4, 6, 9, 1, 2]            # ties to the lower id, ascending id out
    p, e = RM.short_list(ptr, edges, np.array(val, dtype=np.float32), 4)
    assert e[:4, 1].tolist() == [2, 4, 6, 9]
    assert RM.ranks(ptr, edges, np.array(val, dtype=np.float32), 0, [4, 6, 9, 2, 8, 7]) == [1, 2, 3, 4, 5, 0]


# ---- the expectation -------------------------------------------------------------------------------------------------------
def test_visit_counts_estimate_the_ra_path_index():
    """E[c2(v)] / W = RA(s, v) / deg s and E[c3(v)] / W = P3(s, v) / deg s, P3 the sum of 1 / (deg m · deg c) over the 3-walks
    s - m - c - v: every estimate within 5 standard deviations of a binomial share.  Fixed inputs: nothing here can flake.  On
    this input the largest deviation is 0.003 against bounds of at least 0.004."""
    n, rows, (rowptr, col) = irregular()
    s, W = 0, 65535
    deg = {v: len(rows[v]) for v in range(n)}
    ra, p3 = {}, {}
    for m_ in rows[s]:
        for c in rows[m_]:
            ra[c] = ra.get(c, 0.0) + 1.0 / deg[m_]
            for v in rows[c]:
                p3[v] = p3.get(v, 0.0) + 1.0 / (deg[m_] * deg[c])
    assert abs(sum(ra.values()) / deg[s] - 1.0) < 1e-12 and abs(sum(p3.values()) / deg[s] - 1.0) < 1e-12
    c2, c3 = RM.raw_counts(rowptr, col, s, W, 3, 0)
    assert sum(c2.values()) == W and sum(c3.values()) == W and set(c2) <= set(ra) and set(c3) <= set(p3)
    worst = 0.0
    for counts, exact in ((c2, ra), (c3, p3)):
        for v, x in exact.items():
            p = x / deg[s]
            dev = abs(counts.get(v, 0) / W - p)
            worst = max(worst, dev)
            assert dev <= 5.0 * math.sqrt(p * (1.0 - p) / W), (v, dev, p)
    assert worst < 0.004


# ---- header and binding -------------------------------------------------------------------------------------------------------
def test_header_and_binding(hiplib):
    from ocn_amd import _lib, ops
    with open(os.path.join(ROOT, "include", "ocn_hip.h")) as fh:
        header = fh.read()
    assert "#define OCN_ABI_VERSION 9" in header and _lib.ABI_VERSION == 9 and hiplib.ocn_abi_version() == 9
    for name in RW_ENTRIES:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES and hasattr(hiplib, name)
    assert len(_lib.SIGNATURES["ocn_rw_visits_count"][1]) == 12 and len(_lib.SIGNATURES["ocn_rw_visits_fill"][1]) == 16
    assert 1024 <= hiplib.ocn_rw_max_walks() <= 65535 and ops.rw_max_walks() == hiplib.ocn_rw_max_walks()
    with open(os.path.join(ROOT, "ocn_amd", "csrc", "philox.h")) as fh:
        streams = fh.read()
    assert re.search(r"SAMPLE_STREAM_RW_A = 5u, SAMPLE_STREAM_RW_B = 6u", streams) and "SAMPLE_STREAM_TWO_HOP_ID = 4u" in streams
    assert (RM.STREAM_RW_A, RM.STREAM_RW_B) == (5, 6)


def test_entries_refuse_before_any_hip_call(hiplib):
    """NULL pointers, negative sizes, walks outside 1 .. max, another length, a bad decay, misaligned outputs: OCN_EINVAL, on a
    machine without a GPU as well — and Q == 0 returns 0 after the checks."""
    lib = hiplib
    W = lib.ocn_rw_max_walks()
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    n = 4

    def count(**kw):
        a = dict(rpa=p, ca=p, rpm=p, cm=p, n=n, src=p, Q=0, walks=64, length=2, seed=0, count=p)
        a.update(kw)
        return lib.ocn_rw_visits_count(a["rpa"], a["ca"], a["rpm"], a["cm"], a["n"], a["src"], a["Q"], a["walks"], a["length"], a["seed"],
                                       a["count"], None)

    def fill(**kw):
        a = dict(rpa=p, ca=p, rpm=p, cm=p, n=n, src=p, Q=0, walks=64, length=3, seed=0, ptr=p, decay=0.5, edges=p, val=p, visits=p)
        a.update(kw)
        return lib.ocn_rw_visits_fill(a["rpa"], a["ca"], a["rpm"], a["cm"], a["n"], a["src"], a["Q"], a["walks"], a["length"], a["seed"],
                                      a["ptr"], a["decay"], a["edges"], a["val"], a["visits"], None)

    assert count() == 0 and fill() == 0 and count(walks=W, length=3) == 0 and fill(walks=1, length=2, decay=0.0) == 0
    for name in ("rpa", "ca", "rpm", "cm", "src", "count"):
        assert count(**{name: None}) == -1, name
    for name in ("rpa", "ca", "rpm", "cm", "src", "ptr", "edges", "val", "visits"):
        assert fill(**{name: None}) == -1, name
    for call in (count, fill):
        for bad in (dict(Q=-1), dict(n=0), dict(n=-3), dict(n=1 << 31), dict(walks=0), dict(walks=-5), dict(walks=W + 1),
                    dict(walks=65536), dict(length=1), dict(length=4), dict(length=0)):
            assert call(**bad) == -1, (call.__name__, bad)
    for decay in (-0.5, float("nan"), float("inf")):
        assert fill(decay=decay) == -1, decay
    assert fill(edges=odd) == -1 and fill(visits=odd) == -1


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def cpu_adj(n=8):
    from ocn_amd.sparse import SparseTensor
    n, rows, (rowptr, col) = irregular()
    return SparseTensor(rowptr=torch.from_numpy(rowptr), col=torch.from_numpy(col), sparse_sizes=(n, n))


@pytest.fixture
def unreachable(hiplib, monkeypatch):
    from ocn_amd import ops
    for name in ("rw_visits_count", "rw_visits_fill", "scan_i32", "segment_topk", "segment_rank", "check_edges"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: pytest.fail(f"ops.{_n} was reached"))


def test_random_walks_is_checked_when_it_is_made(hiplib):
    from ocn_amd import ops
    from ocn_amd.recommend import RandomWalks
    rw = RandomWalks(128, ops.rw_max_walks(), 3, 0.5, (1 << 64) - 1)
    assert (rw.m, rw.walks, rw.length, rw.decay, rw.seed) == (128, ops.rw_max_walks(), 3, 0.5, (1 << 64) - 1)
    assert RandomWalks(1, 1, 2) == RandomWalks(m=1, walks=1, length=2, decay=None, seed=0)
    with pytest.raises(Exception):
        rw.m = 3                                             # frozen
    for bad, match in (((0, 64, 2), "m must be in"), ((ops.segment_topk_max_k() + 1, 64, 2), "m must be in"), ((True, 64, 2), "m must"),
                       ((2.0, 64, 2), "m must"), ((8, 0, 2), "walks must"), ((8, ops.rw_max_walks() + 1, 2), "walks must"),
                       ((8, 64.0, 2), "walks must"), ((8, True, 2), "walks must"), ((8, 64, 1), "length must"), ((8, 64, 4), "length must"),
                       ((8, 64, True), "length must"), ((8, 64, 3), "decay must"), ((8, 64, 3, -1.0), "decay must"),
                       ((8, 64, 3, float("nan")), "decay must"), ((8, 64, 3, float("inf")), "decay must"), ((8, 64, 3, True), "decay must"),
                       ((8, 64, 2, 0.5), "decay belongs to length=3"), ((8, 64, 2, None, -1), "seed must"),
                       ((8, 64, 2, None, 1 << 64), "seed must"), ((8, 64, 2, None, 1.5), "seed must")):
        with pytest.raises(ValueError, match=match):
            RandomWalks(*bad)


def test_candidates_refuse_before_any_device_work(unreachable):
    from ocn_amd import ops, recommend as R
    from ocn_amd.sparse import SparseTensor
    adj = cpu_adj()
    src = torch.tensor([0, 1], dtype=torch.int64)
    for kw, match in ((dict(walks=64, length=4), "length must"), (dict(walks=0, length=2), "walks must"),
                      (dict(walks=ops.rw_max_walks() + 1, length=3, decay=0.5), "walks must"), (dict(walks=64, length=3), "decay must"),
                      (dict(walks=64, length=3, decay=-1), "decay must"), (dict(walks=64, length=2, decay=0.5), "decay belongs"),
                      (dict(walks=64, length=2, seed=-1), "seed must"), (dict(walks=64, length=2, seed=1 << 64), "seed must")):
        with pytest.raises(ValueError, match=match):
            R.random_walk_candidates(adj, src, **kw)
    with pytest.raises(ValueError, match="1-d int64"):
        R.random_walk_candidates(adj, src.int(), 64, 2)
    with pytest.raises(ValueError, match="1-d int64"):
        R.random_walk_candidates(adj, src[None], 64, 2)
    other = SparseTensor(rowptr=torch.zeros(4, dtype=torch.int64), col=torch.zeros(0, dtype=torch.int32), sparse_sizes=(3, 3))
    with pytest.raises(ValueError, match="known is"):
        R.random_walk_candidates(adj, src, 64, 2, known=other)
    with pytest.raises(ValueError, match="rw must be a RandomWalks"):
        R.random_walk_short_list(adj, src, ("ra", 8))


def test_requests_refuse_before_any_device_work(unreachable):
    from ocn_amd import recommend as R
    from ocn_amd.model import predictor_dict
    from ocn_amd.ranking import rank_links
    adj = cpu_adj()
    src = torch.tensor([0, 1], dtype=torch.int64)
    pred = predictor_dict["cn5"](16, 16, 1, 3, 0.0).eval()
    h = torch.zeros(8, 16)
    truth = (torch.tensor([0, 1, 2]), torch.tensor([4, 5]))
    rw2, rw3 = R.RandomWalks(8, 64, 2), R.RandomWalks(8, 64, 3, 0.5)
    with pytest.raises(ValueError, match="hops = 2"):
        R.recommend_links(pred, h, adj, None, src, 4, 100, prefilter=rw3)
    with pytest.raises(ValueError, match="hops = 3"):
        R.recommend_links(pred, h, adj, None, src, 4, 100, prefilter=rw2, hops=3)
    with pytest.raises(ValueError, match="fewer than k = 9"):
        R.recommend_links(pred, h, adj, None, src, 9, 100, prefilter=rw2)
    with pytest.raises(ValueError, match="hops = 2"):
        rank_links(pred, h, adj, None, src, truth, 100, prefilter=rw3)
    with pytest.raises(ValueError, match="cn6 needs adj2"):
        R.recommend_links(predictor_dict["cn6"](16, 16, 1, 3, 0.0).eval(), h, adj, None, src, 4, 100, prefilter=rw2)
    with pytest.raises(RuntimeError, match="eval"):
        R.recommend_links(pred.train(), h, adj, None, src, 4, 100, prefilter=rw2)


def test_check_prefilter_refuses_what_it_refused(hiplib):
    from ocn_amd import recommend as R
    assert R._check_prefilter(("ra", 32), 5) == ("ra", 32) and R._check_prefilter(("cn", 32, 0.5), 5, 3) == ("cn", 32, 0.5)
    rw = R.RandomWalks(32, 64, 2)
    assert R._check_prefilter(rw, 5, 2) is rw
    with pytest.raises(ValueError, match=r"prefilter must be None or \(kind, m\) with kind one of"):
        R._check_prefilter(("ra", 32, 0.5), 5, 2)
    with pytest.raises(ValueError, match=r"\(kind, m, decay\) under hops=3"):
        R._check_prefilter(("ra", 32), 5, 3)
    with pytest.raises(ValueError, match="is no path sum"):
        R._check_prefilter(("jaccard", 32), 5)
    with pytest.raises(ValueError, match="fewer than k = 40"):
        R._check_prefilter(("ra", 32), 40)
    with pytest.raises(ValueError, match="prefilter must be None"):
        R._check_prefilter("ra:32", 5)
    with pytest.raises(ValueError, match="m an int"):
        R._check_prefilter(("ra", True), 1)


def test_a_valid_request_on_cpu_tensors_reaches_the_device_layer(hiplib):
    """No CPU path: the ops layer refuses host tensors itself."""
    from ocn_amd import _lib, recommend as R
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        R.random_walk_candidates(cpu_adj(), torch.tensor([0, 1], dtype=torch.int64), 64, 2)
