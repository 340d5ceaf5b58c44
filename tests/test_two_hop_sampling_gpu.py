"""The 2-hop hard-negative sampler (``ocn_sample_two_hop``; ocn_amd/sampling.py: ``two_hop_negative_targets``,
``two_hop_negative_edges``) on the GPU against the CPU mirror of tests/two_hop_sampling_mirror.py.  A sample is an integer
fixed by (seed, its own index, adj, known), so every comparison is ``torch.equal``."""
import importlib.util
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import sampling_mirror as SM
from tests import two_hop_sampling_mirror as TM

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERS = (1, 255, 256, 257, 1000)  # below, at and above one chunk of 256 slots, and several chunks
SEED = (0x5EED << 32) | 0x4321   # both key words in use


# ---- graphs ------------------------------------------------------------------------------------------------------------
def on_gpu(n, rowptr, col):
    from ocn_amd.sparse import SparseTensor
    return SparseTensor(rowptr=torch.from_numpy(rowptr).to(DEV), col=torch.from_numpy(col).to(DEV), sparse_sizes=(n, n))


def case(n, rows, sources, known_rows=None):
    """``rows``: {row id: ascending columns} of A (and of ``known`` where it differs).  The CSRs as numpy arrays (the mirror's
    operands) and as SparseTensors on the GPU."""
    for r in (rows, known_rows or {}):
        for s, cols in r.items():
            assert list(cols) == sorted(set(cols)) and (not len(cols) or (0 <= cols[0] and cols[-1] < n)), s
    rowptr, col = TM.csr_of(n, rows)
    src = np.array(sources, dtype=np.int64)
    c = SimpleNamespace(n=n, rows=rows, rowptr=rowptr, col=col, adj=on_gpu(n, rowptr, col), src=src,
                        sources=torch.from_numpy(src).to(DEV), k_rowptr=None, k_col=None, known=None)
    if known_rows is not None:
        c.k_rowptr, c.k_col = TM.csr_of(n, known_rows)
        c.known = on_gpu(n, c.k_rowptr, c.k_col)
    return c


def mirror_targets(c, per, seed=SEED, first=0, fallback="uniform", src=None):
    return torch.from_numpy(TM.two_hop_negative_targets(c.rowptr, c.col, c.n, c.src if src is None else src, per, seed,
                                                        c.k_rowptr, c.k_col, first, fallback))


def cand(c, s):
    return TM.candidates(c.rowptr, c.col, int(s), c.k_rowptr, c.k_col)


@pytest.fixture(scope="module")
def special(hiplib):
    """n = 97, directed, sparse enough that 2-hop sets stay small: an empty row, a row adjacent to every other node, a stored
    self-loop, sources whose only candidate is column 0 / column 96, a source all of whose 2-hop nodes are its neighbours, a
    repeated source; random rows of 1 .. 4 columns elsewhere.  The mirror of the longest call is computed once."""
    n = 97
    rng = np.random.default_rng(97)
    rows = {s: sorted(rng.choice(n, size=int(rng.integers(1, 5)), replace=False).tolist()) for s in range(20, n)}
    rows[1] = [c for c in range(n) if c != 1]                # adjacent to every other node: no candidate, and no non-link either
    rows[2] = [2, 40, 96]                                    # stored self-loop: its own row enters the union
    rows[3], rows[10] = [10], [0, 3]                         # H(3) = {0}
    rows[4], rows[11] = [11], [4, 96]                        # H(4) = {96}
    rows[5], rows[12] = [12, 50], [50]                       # everything within two hops of 5 is a neighbour ...
    rows[50] = [5, 12]                                       # ... or 5 itself: H(5) is empty, the uniform fallback serves it
    rows[6], rows[13] = [13, 96], [0, 1, 2, 3, 94, 95, 96]   # members at both ends of the range
    rows[7] = [20, 21, 22, 23, 24, 25]
    rows[96] = [0, 95]
    sources = [0, 1, 2, 3, 4, 5, 6, 7, 96, 20, 21, 60, 95, 6, 0, 2, 33]          # row 0 is empty; 6, 0 and 2 repeat
    c = case(n, rows, sources)
    assert 0 not in rows and cand(c, 3) == [0] and cand(c, 4) == [96] and cand(c, 5) == [] and cand(c, 1) == [] and cand(c, 0) == []
    assert 0 in cand(c, 6) and 95 in cand(c, 6) and 96 not in cand(c, 6)
    c.want = mirror_targets(c, max(PERS))
    c.want_hard = mirror_targets(c, 65, fallback=None)
    return c


@pytest.fixture(scope="module")
def sweep(hiplib):
    """n = 333 (no multiple of 64): sources whose candidates straddle the edge of a 64- and of a 128-column window, sit exactly
    at a window's first column (64, 128, 192, 320) or at its last (63, 127, 191, 332), or only in the ragged last window."""
    n = 333
    rng = np.random.default_rng(333)
    rows = {s: sorted(rng.choice(n, size=int(rng.integers(1, 6)), replace=False).tolist()) for s in range(40, n)}
    targets = {0: list(range(58, 71)), 1: list(range(120, 137)), 2: [64], 3: [128], 4: [192], 5: [320], 6: [63], 7: [127],
               8: [191], 9: [332], 10: list(range(321, 333)), 11: [63, 64], 12: [127, 128, 255, 256], 13: [0, 332]}
    for s, t in targets.items():
        rows[s], rows[20 + s] = [20 + s], t                  # one neighbour, whose row is the wanted candidate set
    c = case(n, rows, list(targets) + [40, 100, 200, 332, 0, 12])
    for s, t in targets.items():
        assert cand(c, s) == t, s
    return c


@pytest.fixture(scope="module")
def medium(hiplib):
    """n = 500, symmetric, about four neighbours per node and one hub with 120: candidate sets of a few to a few hundred."""
    n = 500
    rng = np.random.default_rng(500)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, n - 5, size=(1000, 2)) if a != b]
    pairs += [(7, int(b)) for b in rng.choice(np.arange(8, n - 5), size=120, replace=False)]
    rows = TM.undirected(n, pairs)                           # the last five nodes stay isolated
    return case(n, rows, list(range(0, n, 7)) + [7, 499, 7])


# ---- 1. hand cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2], ids=["path", "star", "k34"])
def test_hand_cases_draw_from_the_sets_known_by_inspection(which, hiplib):
    from ocn_amd import ops
    from ocn_amd.sampling import two_hop_negative_targets
    name, n, rows, want = TM.hand_cases()[which]
    c = case(n, rows, list(range(n)) + [0])
    got = two_hop_negative_targets(c.adj, c.sources, 40, SEED, fallback=None)
    assert got.dtype == torch.int64 and got.shape == (n + 1, 40) and got.is_contiguous()
    assert torch.equal(got.cpu(), mirror_targets(c, 40, fallback=None))
    for s, h in want.items():
        assert sorted(set(got[s].tolist())) == (h if h else [-1]), (name, s)
    a = (c.adj._rowptr, c.adj._col)
    sptr = torch.arange(n + 2, device=DEV) * 3
    out, count = ops.sample_two_hop(*a, *a, c.sources, sptr, SEED, want_count=True)
    assert count.dtype == torch.int32 and torch.equal(count, ops.two_hop_diff_count(*a, *a, c.sources))
    assert count.tolist() == [len(cand(c, s)) for s in c.src] and torch.equal(out.view(n + 1, 3), got[:, :3])
    # a count-only call (no slot at all) is served too
    out0, count0 = ops.sample_two_hop(*a, *a, c.sources, torch.zeros(n + 2, dtype=torch.int64, device=DEV), SEED, want_count=True)
    assert out0.shape == (0,) and torch.equal(count0, count)


# ---- 2. special graph, varying per --------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", PERS)
def test_targets_equal_the_mirror_bit_for_bit(special, per):
    from ocn_amd.sampling import two_hop_negative_targets
    c = special
    got = two_hop_negative_targets(c.adj, c.sources, per, SEED)
    assert got.dtype == torch.int64 and got.shape == (len(c.src), per) and got.is_contiguous()
    assert torch.equal(got.cpu(), c.want[:, :per])
    assert bool((got[3] == 0).all()) and bool((got[4] == 96).all()) and bool((got[1] == -1).all())
    if per >= 255:                                            # the same source at another position draws other samples
        assert not torch.equal(got[6], got[13]) and not torch.equal(got[2], got[15])
        assert {0, 95} <= set(got[6].tolist())


# ---- 3. window sweep ----------------------------------------------------------------------------------------------------
def test_window_width_does_not_enter_the_result(sweep):
    """The same samples and counts at 64-column windows (six, the last one ragged), 128-column windows and the default
    (one window, the one-sweep path), all equal to the mirror.  The two-sweep path of a graph wider than the default window
    (more than a million columns) cannot be reached at test size: it is the same code that ``window_cols = 64`` runs here."""
    from ocn_amd import ops
    c = sweep
    a = (c.adj._rowptr, c.adj._col)
    lens = np.array([300, 257, 1, 5, 0, 256] + [7] * (len(c.src) - 6), dtype=np.int64)        # ragged slots, an empty range
    sptr = np.concatenate([[0], np.cumsum(lens)])
    want, want_count = TM.sample_two_hop(c.rowptr, c.col, c.src, sptr, SEED, q0=11)
    dsptr = torch.from_numpy(sptr).to(DEV)
    assert ops.sample_two_hop_window_cols() >= c.n
    for window in (64, 128, 0):
        out, count = ops.sample_two_hop(*a, *a, c.sources, dsptr, SEED, first=11, want_count=True, window_cols=window)
        assert torch.equal(out.cpu(), torch.from_numpy(want)), window
        assert torch.equal(count.cpu().long(), torch.from_numpy(want_count)), window
        assert torch.equal(count, ops.two_hop_diff_count(*a, *a, c.sources, window_cols=window))
        assert torch.equal(out, ops.sample_two_hop(*a, *a, c.sources, dsptr, SEED, first=11, window_cols=window))
    # with sample ids: fixed by the id, not by the slot's place or the window
    sid = torch.from_numpy(np.random.default_rng(1).permutation(int(sptr[-1])).astype(np.int64) + (1 << 33)).to(DEV)
    want_id, _ = TM.sample_two_hop(c.rowptr, c.col, c.src, sptr, SEED, sid=sid.cpu().numpy())
    for window in (64, 0):
        got = ops.sample_two_hop(*a, *a, c.sources, dsptr, SEED, sid=sid, first=5, window_cols=window)
        assert torch.equal(got.cpu(), torch.from_numpy(want_id)), window
    # every member of a set that straddles a window edge is drawn: 13 members, 300 draws
    assert sorted(set(out[:300].tolist())) == list(range(58, 71))


# ---- 4. more than one bitmap word per thread ----------------------------------------------------------------------------
def test_wide_graph_with_several_words_per_thread(hiplib):
    """n = 70 000: the window's 2 188 words are nine per thread.  Sparse random rows, and a hub whose 3 000 neighbours span the
    whole range: a source next to the hub has candidates in the words of every thread."""
    from ocn_amd.sampling import two_hop_negative_targets
    n, hub = 70_000, 31_000
    rng = np.random.default_rng(70)
    keys = rng.integers(0, n, size=3 * n, dtype=np.int64) * n + rng.integers(0, n, size=3 * n, dtype=np.int64)
    hub_cols = np.unique(np.concatenate([rng.choice(n, size=3000, replace=False), [0, 31, 32, n - 1]]))
    src = np.array([5, 40_000, n - 1, hub, 123, 5], dtype=np.int64)
    keys = np.unique(np.concatenate([keys, hub * n + hub_cols, src[:3] * n + hub]))
    row, col = keys // n, (keys % n).astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.int64)
    c = SimpleNamespace(n=n, rowptr=rowptr, col=col, adj=on_gpu(n, rowptr, col), src=src, k_rowptr=None, k_col=None)
    h5 = cand(c, 5)
    assert len(h5) > 2900 and h5[0] == 0 and h5[-1] == n - 1
    got = two_hop_negative_targets(c.adj, torch.from_numpy(src).to(DEV), 300, SEED)
    assert torch.equal(got.cpu(), mirror_targets(c, 300))
    assert got[0].unique().numel() > 250 and int(got[0].max()) > n * 9 // 10 and int(got[0].min()) < n // 10


# ---- 5. known != adj ----------------------------------------------------------------------------------------------------
def test_known_superset_excludes_its_links(medium):
    from ocn_amd.sampling import two_hop_negative_targets
    m = medium
    known_rows = {s: list(v) for s, v in m.rows.items()}
    extra = {}
    for s in (0, 7, 14, 21, 70):                             # every other candidate of these sources becomes a known link
        extra[s] = cand(m, s)[::2]
        assert extra[s]
        known_rows[s] = sorted(set(known_rows.get(s, [])) | set(extra[s]))
    known_rows[28] = sorted(set(known_rows.get(28, [])) | set(cand(m, 28)))      # all of them: the uniform fallback serves 28
    c = case(m.n, m.rows, m.src.tolist(), known_rows)
    assert cand(c, 28) == [] and cand(c, 7) == cand(m, 7)[1::2]
    got = two_hop_negative_targets(c.adj, c.sources, 64, SEED, known=c.known)
    assert torch.equal(got.cpu(), mirror_targets(c, 64))
    k_keys = torch.from_numpy(np.repeat(np.arange(c.n), np.diff(c.k_rowptr)) * c.n + c.k_col.astype(np.int64)).to(DEV)
    live = got >= 0
    assert not bool(torch.isin((c.sources[:, None] * c.n + got)[live], k_keys).any())
    assert not torch.equal(got, two_hop_negative_targets(c.adj, c.sources, 64, SEED))


# ---- 6. membership and coverage -----------------------------------------------------------------------------------------
def test_samples_are_candidates_and_cover_a_small_set(medium):
    from ocn_amd.recommend import two_hop_candidates
    from ocn_amd.sampling import two_hop_negative_targets
    c = medium
    got = two_hop_negative_targets(c.adj, c.sources, 200, SEED + 1, fallback=None)
    ptr, edges = two_hop_candidates(c.adj, None, c.sources)
    keys = edges[:, 0] * c.n + edges[:, 1]
    empty = (ptr[1:] == ptr[:-1])
    assert bool((got[empty] == -1).all()) and bool((got[~empty] >= 0).all()) and bool(empty.any()) and not bool(empty.all())
    assert bool(torch.isin((c.sources[:, None] * c.n + got)[~empty], keys).all())
    # coverage: a source with at most 50 candidates, 4096 draws — a condition on this seed, which the mirror alone meets
    s = next(int(v) for v in c.src if 20 <= len(cand(c, v)) <= 50)
    h = cand(c, s)
    one = np.array([s], dtype=np.int64)
    want = mirror_targets(c, 4096, src=one)
    assert sorted(set(want[0].tolist())) == h
    got = two_hop_negative_targets(c.adj, torch.from_numpy(one).to(DEV), 4096, SEED)
    assert torch.equal(got.cpu(), want)
    counts = torch.bincount(got[0], minlength=c.n)[torch.tensor(h, device=DEV)]
    bound = 5 * math.sqrt(4096 / len(h))                     # five standard deviations of a deterministic sequence
    assert bool(((counts - 4096 / len(h)).abs() <= bound).all())


# ---- 7. prefix and chunking ---------------------------------------------------------------------------------------------
def test_prefix_in_per_and_chunks_in_first(special, medium):
    from ocn_amd.sampling import two_hop_negative_edges, two_hop_negative_targets
    c = special
    long = two_hop_negative_targets(c.adj, c.sources, 1000, SEED)
    assert torch.equal(long[:, :65], two_hop_negative_targets(c.adj, c.sources, 65, SEED))
    assert torch.equal(two_hop_negative_targets(c.adj, c.sources, 65, SEED, fallback=None).cpu(), c.want_hard)
    Q1 = 3
    chunked = torch.cat([two_hop_negative_targets(c.adj, c.sources[:Q1].contiguous(), 65, SEED, first=0),
                         two_hop_negative_targets(c.adj, c.sources[Q1:].contiguous(), 65, SEED, first=Q1)])
    assert torch.equal(chunked, long[:, :65])
    assert not torch.equal(long, two_hop_negative_targets(c.adj, c.sources, 1000, SEED + 1))
    far = (1 << 33) + 5                                      # the high counter word of the query index
    assert torch.equal(two_hop_negative_targets(c.adj, c.sources, 9, SEED, first=far).cpu(), mirror_targets(c, 9, first=far))
    assert two_hop_negative_targets(c.adj, c.sources[:0].contiguous(), 4, SEED).shape == (0, 4)
    m = medium
    pos = torch.stack((m.sources, (m.sources + 1) % m.n))
    whole = two_hop_negative_edges(m.adj, pos, SEED)
    cut = 20
    parts = torch.cat([two_hop_negative_edges(m.adj, pos[:, :cut].contiguous(), SEED),
                       two_hop_negative_edges(m.adj, pos[:, cut:].contiguous(), SEED, first=cut)], dim=1)
    assert torch.equal(parts, whole)
    assert not torch.equal(whole, two_hop_negative_edges(m.adj, pos, SEED + 1))


# ---- 8. corrupted-target pairs ------------------------------------------------------------------------------------------
def test_negative_edges_equal_the_mirror_positive_by_positive(medium):
    """Sources in arbitrary order, repeated; the hub source 7 has 1 000 positives: ragged slots over several chunks of 256."""
    from ocn_amd.sampling import two_hop_negative_edges
    c = medium
    rng = np.random.default_rng(8)
    src = np.concatenate([rng.integers(0, c.n, size=400), np.full(1000, 7), [499, 3, 3, 498]]).astype(np.int64)
    rng.shuffle(src)
    pos = np.stack([src, rng.integers(0, c.n, size=src.size)]).astype(np.int64)
    dpos = torch.from_numpy(pos).to(DEV)
    got = two_hop_negative_edges(c.adj, dpos, SEED, first=17)
    assert got.dtype == torch.int64 and got.shape == pos.shape and torch.equal(got[0], dpos[0])
    assert torch.equal(got.cpu(), torch.from_numpy(TM.two_hop_negative_edges(c.rowptr, c.col, c.n, pos, SEED, first=17)))
    hard = two_hop_negative_edges(c.adj, dpos, SEED, first=17, fallback=None)
    assert torch.equal(hard.cpu(), torch.from_numpy(TM.two_hop_negative_edges(c.rowptr, c.col, c.n, pos, SEED, first=17,
                                                                              fallback=None)))
    # the positives of one source draw independently from one set: the hub's 1 000 draws are its candidates, many of them
    mine = hard[1][dpos[0] == 7]
    h7 = cand(c, 7)
    assert mine.numel() == int((src == 7).sum()) >= 1000     # (the random sources may hold a 7 as well)
    assert set(mine.tolist()) <= set(h7) and mine.unique().numel() > min(len(h7), 1000) // 3
    # the pair is a function of (seed, first + t, its source): the same positive list behind another prefix
    again = two_hop_negative_edges(c.adj, dpos[:, 5:].contiguous(), SEED, first=22)
    assert torch.equal(again, got[:, 5:])


# ---- 9. fallback --------------------------------------------------------------------------------------------------------
def test_fallback_is_the_uniform_sample_exactly_where_there_is_no_candidate(special):
    from ocn_amd.sampling import negative_targets, two_hop_negative_edges, two_hop_negative_targets
    c = special
    none = torch.tensor([len(cand(c, s)) == 0 for s in c.src], device=DEV)
    assert int(none.sum()) == 4                              # rows 0 (twice), 1 and 5
    hard = two_hop_negative_targets(c.adj, c.sources, 65, SEED, fallback=None)
    both = two_hop_negative_targets(c.adj, c.sources, 65, SEED)
    uni = negative_targets(c.adj, c.sources, 65, SEED)
    assert bool((hard[none] == -1).all()) and bool((hard[~none] >= 0).all())
    assert torch.equal(both[none], uni[none]) and torch.equal(both[~none], hard[~none])
    assert not torch.equal(both[~none], uni[~none])
    assert bool((both[1] == -1).all()) and bool((both[5] >= 0).all())            # linked to every node: -1 either way
    first = 40
    pos = torch.stack((c.sources, c.sources.flip(0)))
    e_hard = two_hop_negative_edges(c.adj, pos, SEED, first=first, fallback=None)
    e_both = two_hop_negative_edges(c.adj, pos, SEED, first=first)
    e_uni = negative_targets(c.adj, c.sources, 1, SEED, first)[:, 0]
    assert bool((e_hard[1][none] == -1).all()) and bool((e_hard[1][~none] >= 0).all())
    assert torch.equal(e_both[1][none], e_uni[none]) and torch.equal(e_both[1][~none], e_hard[1][~none])


# ---- 10. example driver -------------------------------------------------------------------------------------------------
def _driver():
    spec = importlib.util.spec_from_file_location("run_like_reference", os.path.join(ROOT, "examples", "run_like_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_driver_trains_on_hard_negatives(hiplib, capsys):
    """examples/run_like_reference.py --hard-negatives 0.5 on the Cora shape, one epoch: half of the training negatives are 2-hop
    corruptions; the loss is finite and the metric line is printed."""
    out = _driver().main(["--dataset", "cora", "--epochs", "1", "--hiddim", "64", "--feat", "64", "--hard-negatives", "0.5"])
    loss, results = out[0]
    assert math.isfinite(loss) and all(0.0 <= v <= 1.0 for v in results["Hits@100"])
    assert "Hits@100 train/valid/test" in capsys.readouterr().out


def test_example_driver_scores_mrr_on_hard_negatives(hiplib, capsys):
    """... and with --hard-eval-negatives on the citation2 shape at a small scale: the MRR of valid and test among negatives
    within two hops of each source."""
    out = _driver().main(["--dataset", "citation2", "--scale", "0.001", "--epochs", "1", "--hiddim", "32", "--predictor", "cn7",
                          "--hard-negatives", "0.5", "--hard-eval-negatives"])
    loss, results = out[0]
    assert math.isfinite(loss) and len(results["MRR"]) == 2 and all(0.0 < v <= 1.0 for v in results["MRR"])
    assert "MRR valid/test" in capsys.readouterr().out
