"""The walk-count route pinned at its edges (cn_walk.hip: the per-candidate two-sided sweeps; walk_group.hip: ocn_walk_prep and
the shared-source sweep; common.h: walk_group, walk_reverse; scan.hip: ocn_chunk_offsets, ocn_walk_rev_offsets) against the exact
mirror of tests/walk_mirror.py.  All outputs are integers: every comparison is ``torch.equal``.

The graphs are constructed (tests/walk_cases.py), not random: node ids that share a bit of a Bloom bitmap, keys whose probe
chains cross the wrap of an 8192-slot table, rows one short of, at and one past every tile size.  The premises of the collision
and wrap cases — that they do contain what they were built to contain — are asserted without a GPU, by the same builders, in
tests/test_walk_edges_host.py; they are asserted again here next to each comparison, through ``ocn_walk_hash``."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import walk_cases as WC
from tests import walk_mirror as WM

pytestmark = pytest.mark.gpu
DEV = "cuda"
ST_CAP = 1
Got = namedtuple("Got", "order off flags wc hist cnt1 cnt2 status ws")


_graphs = {}


def device_graph(c):
    """(rowptr, col, longest row) of a case on the device; the builders cache their cases, so a graph goes up once"""
    key = id(c.rowptr)
    if key not in _graphs:
        if len(_graphs) >= 4:
            _graphs.clear()
        _graphs[key] = (c.rowptr, torch.from_numpy(c.rowptr).to(DEV), torch.from_numpy(c.col).to(DEV), int(np.diff(c.rowptr).max()))
    return _graphs[key][1:]


def buffer(ws, name):
    """the scratch tensor ``name`` of a workspace dict of ocn_amd.ops.buf"""
    hits = [v for k, v in ws.items() if k[0] == name]
    assert len(hits) == 1, name
    return hits[0]


def run(monkeypatch, c, src=None, dst=None, nds=None, share=0, ws=None):
    """ops.cn_flags on the walk route, outputs on the host; ``ws``: the caller's workspace dict (read back through ``buffer``)."""
    from ocn_amd import ops
    monkeypatch.setattr(ops, "walk_share_min", share)
    rowptr, col, max_deg = device_graph(c)
    src, dst = (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in (c.src if src is None else src, c.dst if dst is None else dst))
    ws = {} if ws is None else ws
    nds_t = None if nds is None else torch.from_numpy(np.ascontiguousarray(nds)).to(DEV)
    order, off, flags, wc, hist, c1, c2, status, _ = ops.cn_flags(rowptr, col, None, None, src, dst, rowptr.numel() - 1, max_deg,
                                                                   walk=True, nds=nds_t, wsd=ws)
    torch.cuda.synchronize()
    return Got(None if order is None else order.cpu(), off.cpu(), flags.cpu(), wc.cpu(), ops.hist_counts(hist).cpu(), c1.cpu(),
               c2.cpu(), status.cpu(), ws)


def same(got, want):
    """all raw outputs of the route equal the mirror's"""
    assert int(got.status[0]) == 0
    assert torch.equal(got.off, torch.from_numpy(want.off))
    t = int(want.off[-1])
    assert torch.equal(got.flags[:t], torch.from_numpy(want.flags))
    assert torch.equal(got.wc[:t], torch.from_numpy(want.wc))
    assert torch.equal(got.cnt1, torch.from_numpy(want.cnt1))
    assert torch.equal(got.cnt2, torch.from_numpy(want.cnt2))
    assert torch.equal(got.hist, torch.from_numpy(want.hist))


@functools.lru_cache(maxsize=None)
def mirror_of(key, *args):
    c = getattr(WC, key)(*args)
    return WM.mirror(c.rowptr, c.col, c.src, c.dst)


def cost_vector(c, mode):
    """None, the true nds, or a doctored one: ``forced`` sends every row to the target's side; ``cg1`` / ``cgmid`` / ``cg8`` make
    walk_group (common.h) cut a source row of several chunks into items of 1, 2 and 8 chunks."""
    if mode == "none":
        return None
    if mode == "true":
        return WM.neighbor_degree_sum(c.rowptr, c.col)
    if mode == "forced":
        return WC.forced_reverse(c)
    chunks = (WM.degrees(c.rowptr) + 63) // 64
    return chunks * {"cg1": 16384, "cgmid": 5461, "cg8": 0}[mode]


# ---------------------------------------------------------------------------------------------------------------------------
# per-candidate sweeps (walk_share_min = 0: nothing is shared)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "true", "forced"])
@pytest.mark.parametrize("big", [False, True])
def test_bloom_false_positives_of_the_per_candidate_sweeps(hiplib, monkeypatch, big, mode):
    """A swept element that shares its bit with a member of the probed row and is no member — swept from the source's side, from
    the target's side, and as a neighbour of the source in the cn1 test of the finalise step — counts for nothing.  The probed
    row has 3 entries (resolved in its LDS copy) or 4097 (resolved in memory); the colliding key sorts before its first entry,
    between two, after its last."""
    c = WC.bloom_case(hiplib, big)
    for g in c.info["gadgets"]:                       # the premise, through the library's hash (in full: the host suite)
        probed = WM.row(c.rowptr, c.col, g["probed"])
        assert hiplib.ocn_walk_hash(0, g["elem"]) == hiplib.ocn_walk_hash(0, g["member"])
        assert g["elem"] not in probed and g["member"] in probed and probed.size == (4097 if big else 3)
    want = mirror_of("bloom_case", hiplib, big)
    got = run(monkeypatch, c, nds=cost_vector(c, mode))
    same(got, want)
    for g in c.info["gadgets"]:                       # what the gadgets are about, spelled out: one true hit, no false one
        lo, hi = int(want.off[g["e"]]), int(want.off[g["e"] + 1])
        if g["kind"] == "f1":
            assert int(got.cnt1[g["e"]]) == 1 and int((got.flags[lo:hi] & 1).sum()) == 1
        else:
            assert int(got.wc[lo:hi].sum()) == 1 and int(got.cnt2[g["e"]]) == 1


@pytest.mark.parametrize("mode", ["none", "true", "forced", "cg1", "cgmid", "cg8"])
def test_row_lengths_of_both_endpoints(hiplib, monkeypatch, mode):
    """Source rows of 0, 1, 63, 64, 65, 511, 512, 513 and 1025 neighbours against probed rows of 0, 1, 15, 16, 17, 33, 4095, 4096
    and 4097 (and, for the sweep from the target's side, which probes the source's row, sources of 4095, 4096 and 4097), with
    self-candidates, repeated candidates, isolated endpoints and stored edges, under every cost vector.  The
    forward item count is ceil(ceil(d / 64) / walk_group), the reverse one ceil(d_j / 16) per row swept from the target."""
    c = WC.sizes_case()
    nds = cost_vector(c, mode)
    got = run(monkeypatch, c, nds=nds)
    same(got, mirror_of("sizes_case"))
    fwd, rev = WC.item_counts(c, nds)
    assert int(buffer(got.ws, "chunk_off")[-1]) == fwd
    deg = WM.degrees(c.rowptr)
    if mode == "none":
        assert fwd == int(((deg[c.src] + 63) // 64).sum())
    else:
        assert int(buffer(got.ws, "rev_off")[-1]) == rev
    if mode == "forced":                              # every row with two endpoints of its own is swept from the target's side
        live = (deg[c.src] > 0) & (deg[c.dst] > 0) & (c.src != c.dst)
        assert rev == int(((deg[c.dst] + 15) // 16)[live].sum()) and {15, 16, 17, 33} <= set(deg[c.dst][live])
    s1025 = c.info["s"][1025]
    if mode in ("cg1", "cgmid", "cg8"):
        cg = WC.walk_group_rule(nds, s1025, 1025)
        assert cg == {"cg1": 1, "cgmid": 2, "cg8": 8}[mode]
        assert -(-17 // cg) == {"cg1": 17, "cgmid": 9, "cg8": 3}[mode]       # its 17 chunks: 17, 9 and 3 items


@pytest.mark.parametrize("mode", ["none", "forced"])
@pytest.mark.parametrize("which", ["65x17", "1025x4097", "0x0", "1x4096", "self", "isolated self"])
def test_a_batch_of_one(hiplib, monkeypatch, which, mode):
    c = WC.sizes_case()
    e = {"65x17": WC.SRC_DEGS.index(65) * 9 + WC.TGT_DEGS.index(17), "1025x4097": 80, "0x0": 0,
         "1x4096": 9 + WC.TGT_DEGS.index(4096), "self": 81, "isolated self": 83}[which]
    src, dst = c.src[e:e + 1], c.dst[e:e + 1]
    one = WC.Case(c.rowptr, c.col, src, dst, None)
    got = run(monkeypatch, c, src, dst, nds=cost_vector(one, mode))
    same(got, WM.mirror(c.rowptr, c.col, src, dst))


@pytest.mark.parametrize("mode", ["none", "true", "forced"])
def test_hit_queue_when_every_swept_element_is_a_hit(hiplib, monkeypatch, mode):
    """i - X, X - Y complete, j in X: the 64 rows of 128 elements are all neighbours of j.  Both rounds of 4096 elements fill the
    1024-entry queue and resolve the rest in place.  wc = |Y| + 1 = 128 for every neighbour of i, none is a cn1 entry."""
    c = WC.block_case()
    bits = WC.table(hiplib, 0, c.rowptr.size - 1)
    assert WC.first_round_passes(c, bits) == (WC.ROUND, 2 * WC.ROUND) and WC.ROUND > WC.QUEUE
    got = run(monkeypatch, c, nds=cost_vector(c, mode))
    same(got, mirror_of("block_case"))
    assert (got.wc[:128] == 128).all() and (got.flags[:128] == 2).all()
    assert got.cnt1[:2].tolist() == [0, 0] and got.cnt2[:2].tolist() == [64, 64]


@pytest.mark.parametrize("n_pass", [512, 513])
def test_hit_queue_at_its_flush_threshold(hiplib, monkeypatch, n_pass):
    """A work item's first round (of two) ends with exactly 512 entries queued — half the queue, not more: they wait for the next
    round — and with 513: resolved at once."""
    c = WC.flush_case(hiplib, n_pass)
    assert WC.first_round_passes(c, WC.table(hiplib, 0, c.rowptr.size - 1)) == (n_pass, 5120)
    want = mirror_of("flush_case", hiplib, n_pass)
    assert int(want.wc.sum()) == 63 * 10 + n_pass - 510
    for mode in ("none", "forced"):
        same(run(monkeypatch, c, nds=cost_vector(c, mode)), want)


# ---------------------------------------------------------------------------------------------------------------------------
# ocn_walk_prep and the shared sweep (walk_share_min >= 2, B <= 4096)
# ---------------------------------------------------------------------------------------------------------------------------
def prep_outputs(got, src, dst, c, min_share, nds_free=True):
    """order is a permutation in which equal sources are contiguous; g_head cuts every run into pieces of at most 64; g_active is
    the documented rule (``nds_free``: without a cost vector the rule alone decides).  Returns (g_head, g_active, meta)."""
    B = src.size
    order = got.order.numpy()
    assert sorted(order.tolist()) == list(range(B))
    s = src[order]
    runs = 1 + int((s[1:] != s[:-1]).sum())
    assert runs == np.unique(src).size                                  # contiguous: as many runs as sources
    meta = buffer(got.ws, "walk_meta").cpu().numpy()
    head = buffer(got.ws, "g_head").cpu().numpy()[:meta[0] + 1]
    want_head, want_active = WM.shared_rule(c.rowptr, src, dst, order, min_share)
    assert head.tolist() == want_head.tolist() and (np.diff(head) <= 64).all()
    active = buffer(got.ws, "g_active").cpu().numpy()[:B]
    if nds_free:
        assert active.tolist() == want_active.tolist()
    return head, active, meta


@pytest.mark.parametrize("B", [1, 2, 1023, 1024, 1025, 4095, 4096])
def test_prep_batch_sizes(hiplib, monkeypatch, B):
    c = WC.batch_sizes_case()
    src, dst = c.src[:B], c.dst[:B]
    got = run(monkeypatch, c, src, dst, share=2)
    same(got, WM.prefix(mirror_of("batch_sizes_case"), c.rowptr, c.col, c.src, B))
    _, active, _ = prep_outputs(got, src, dst, c, 2)
    assert B < 1023 or active.sum() > B // 2                            # the shared sweep does carry these batches


def test_path_switch_past_the_prep_limit(hiplib, monkeypatch):
    """4096 candidates go through ocn_walk_prep, 4097 through the general path: the same rows come out."""
    assert hiplib.ocn_walk_prep_max_batch() == 4096
    c = WC.batch_sizes_case()
    small = run(monkeypatch, c, c.src[:4096], c.dst[:4096], share=2, ws={})
    assert any(k[0] == "walk_meta" for k in small.ws)
    large = run(monkeypatch, c, share=2, ws={})
    assert not any(k[0] == "walk_meta" for k in large.ws)
    same(large, mirror_of("batch_sizes_case"))
    t = int(small.off[-1])
    assert torch.equal(small.flags[:t], large.flags[:t]) and torch.equal(small.wc[:t], large.wc[:t])
    assert torch.equal(small.cnt1, large.cnt1[:4096]) and torch.equal(small.cnt2, large.cnt2[:4096])
    assert torch.equal(small.off, large.off[:4097])


@pytest.mark.parametrize("min_share", [2, 3])
def test_group_sizes_key_capacity_and_big_targets(hiplib, monkeypatch, min_share):
    """Sources with 63, 64, 65, 128 and 129 candidates (source rows of 63, 64 and 65 among them: a last chunk short of 64 rows),
    fifty with 2, groups of min_share - 1 and min_share small members, target rows that sum to 4096 (shared) and 4097 (not),
    targets of 512 (shared) and 513 neighbours (not, while the rest of their group is)."""
    c = WC.groups_case()
    got = run(monkeypatch, c, share=min_share)
    same(got, mirror_of("groups_case"))
    _, active, meta = prep_outputs(got, c.src, c.dst, c, min_share)
    assert meta[2] == 1                                                 # few chunks: one per item
    by_src = {}
    for s, j, a in zip(c.src[got.order.numpy()], c.dst[got.order.numpy()], active):
        by_src.setdefault(int(s), []).append((int(j), int(a)))
    deg = WM.degrees(c.rowptr)
    what = {v[0]: s for s, v in c.info["groups"].items()}
    assert sum(a for _, a in by_src[what["keys 4096"]]) == 9 and sum(a for _, a in by_src[what["keys 4097"]]) == 0
    assert sum(a for _, a in by_src[what["two small"]]) == (2 if min_share == 2 else 0)
    assert sum(a for _, a in by_src[what["one small"]]) == 0 and sum(a for _, a in by_src[what["three small"]]) == 3
    assert sorted((int(deg[j]), a) for j, a in by_src[what["mixed"]]) == [(5, 1), (7, 1), (512, 1), (513, 0)]


@pytest.mark.parametrize("cluster", [False, True])
def test_bloom_false_positive_of_the_shared_sweep(hiplib, monkeypatch, cluster):
    """A swept element shares its bit of the shared sweep's bitmap with a key and is no key: its lookup ends at an empty slot —
    its home slot, or the one behind three other keys — and counts for nothing."""
    c = WC.group_bloom_case(hiplib, cluster)
    n = c.rowptr.size - 1
    keys, m, x = WC.group_keys(c), c.info["elem"], c.info["member"]
    assert hiplib.ocn_walk_hash(1, m) == hiplib.ocn_walk_hash(1, x) and m not in keys and x in keys
    used, _ = WC.occupied(keys, WC.table(hiplib, 2, n))
    assert WC.probes(m, used, WC.table(hiplib, 2, n)) == (3 if cluster else 0)
    got = run(monkeypatch, c, share=2)
    same(got, mirror_of("group_bloom_case", hiplib, cluster))
    _, active, _ = prep_outputs(got, c.src, c.dst, c, 2)
    assert active.all()
    assert got.wc[:2].tolist() == [1, 0]              # (i, j1): the true key under the same row counts once; (i, j2): nothing


def test_key_table_wrap_in_the_shared_sweep(hiplib, monkeypatch):
    """Keys of slots 8189, 8190 and three of 8191: the cluster runs through slot 0.  The keys displaced across the wrap are found,
    and an element that is no key, with its home slot in the cluster and past the bitmap, is walked across the wrap to an empty
    slot."""
    c = WC.wrap_sweep_case(hiplib)
    h2 = WC.table(hiplib, 2, c.rowptr.size - 1)
    used, slot_of = WC.occupied(WC.group_keys(c), h2)
    assert {WC.SLOTS - 1, 0} <= used and sorted(slot_of[v] for v in c.info["displaced"]) == [0, 1, WC.SLOTS - 1]
    assert hiplib.ocn_walk_hash(1, c.info["elem"]) == hiplib.ocn_walk_hash(1, c.info["member"])
    assert hiplib.ocn_walk_hash(2, c.info["elem"]) >= WC.SLOTS - 3 and c.info["elem"] not in WC.group_keys(c)
    got = run(monkeypatch, c, share=2)
    same(got, mirror_of("wrap_sweep_case", hiplib))
    _, active, _ = prep_outputs(got, c.src, c.dst, c, 2)
    assert active.all()
    assert got.wc[:6].tolist() == [2, 1, 2, 2, 2, 1]  # (i, j1): a, b under k1 and e under k2; (i, j2): b, c and c, d; (i, j1) again


def test_source_table_wrap_in_the_prep(hiplib, monkeypatch):
    """Seven sources whose slots of the prep's source table cluster across 8191 -> 0."""
    c = WC.wrap_prep_case(hiplib)
    used, _ = WC.occupied(np.unique(c.src), WC.table(hiplib, 2, c.rowptr.size - 1))
    assert {WC.SLOTS - 1, 0} <= used and len(used) == 7
    got = run(monkeypatch, c, share=2)
    same(got, mirror_of("wrap_prep_case", hiplib))
    head, active, _ = prep_outputs(got, c.src, c.dst, c, 2)
    assert active.all() and head.tolist() == list(range(0, 15, 2))


@pytest.mark.parametrize("n_hubs", [48, 96])
def test_chunks_per_item_of_the_shared_sweep(hiplib, monkeypatch, n_hubs):
    """meta[2] chunks of 64 neighbours of the source per work item: one for small batches (asserted with the group sizes), a
    value in 2 .. 7 for 48 sources of 4096 neighbours, 8 for 96.  The source of 13 chunks ends in a ragged item either way."""
    c = WC.cpi_case(n_hubs)
    got = run(monkeypatch, c, share=2)
    same(got, mirror_of("cpi_case", n_hubs))
    head, active, meta = prep_outputs(got, c.src, c.dst, c, 2)
    cpi = int(meta[2])
    assert (2 <= cpi <= 7) if n_hubs == 48 else cpi == 8
    assert active.all() and 13 % cpi != 0
    deg = WM.degrees(c.rowptr)
    chunks = (deg[c.src[got.order.numpy()[head[:-1]]]] + 63) // 64
    assert int(chunks.sum()) == c.info["chunks"]
    items = buffer(got.ws, "g_item_off").cpu().numpy()[:meta[0] + 1]
    assert np.diff(items).tolist() == (-(-chunks // cpi)).tolist()


def test_cost_model_of_the_prep_with_nds(hiplib, monkeypatch):
    """With a cost vector the prep shares a group only where the shared sweep is cheaper than its members' own: 192 candidates
    of a source whose sweep reads 100 000 elements share it; two candidates with light targets are each swept from their
    target's side.  Both equal the mirror."""
    c = WC.cost_case()
    nds = cost_vector(c, "true")
    want = mirror_of("cost_case")
    many = run(monkeypatch, c, nds=nds, share=2)
    same(many, want)
    _, active, _ = prep_outputs(many, c.src, c.dst, c, 2, nds_free=False)
    assert active.all()
    src, dst = c.src[:2], c.dst[:2]
    two = run(monkeypatch, c, src, dst, nds=nds, share=2)
    same(two, WM.prefix(want, c.rowptr, c.col, c.src, 2))
    _, active, _ = prep_outputs(two, src, dst, c, 2, nds_free=False)
    assert not active.any()
    assert int(buffer(two.ws, "rev_off")[-1]) == 2                      # ... from the target's side: one reverse item each


# ---------------------------------------------------------------------------------------------------------------------------
# capacity
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["forward", "reverse", "shared"])
def test_flag_buffer_too_small(hiplib, monkeypatch, mode):
    """ocn_hip.h, ocn_cn_walk_flags: under OCN_ST_CAP a row is written whole or not at all.  Rows that fit are exact; the flags of
    the others keep what the buffer held (their walk counts too, unless a cost vector is given: then wc is cleared up to the
    cap).  Counts and histogram stay whole for rows swept from the source's side and for the shared sweep; a row that does not
    fit and is swept from the target's side reports its cn1 entries only."""
    from ocn_amd import ops
    c = WC.groups_case() if mode == "shared" else WC.sizes_case()
    want = mirror_of("groups_case" if mode == "shared" else "sizes_case")
    B = c.src.size
    fit = B // 2
    cap = int(want.off[fit] + want.off[fit + 1]) // 2
    assert want.off[fit] < cap < want.off[fit + 1] < want.off[-1]
    monkeypatch.setattr(ops, "_flag_capacity", lambda B, max_deg_a, off: cap)
    dev = str(device_graph(c)[0].device)               # (the workspace dict of ops.buf: name, shape, dtype, device)
    ws = {("flags", (cap,), torch.uint8, dev): torch.full((cap,), 0xEE, dtype=torch.uint8, device=DEV),
          ("wc", (cap,), torch.int32, dev): torch.full((cap,), -77, dtype=torch.int32, device=DEV)}
    nds = WC.forced_reverse(c) if mode == "reverse" else None
    got = run(monkeypatch, c, nds=nds, share=2 if mode == "shared" else 0, ws=ws)
    assert got.flags.numel() == cap and got.flags.data_ptr() != 0 and len([k for k in got.ws if k[0] == "flags"]) == 1
    assert int(got.status[0]) & ST_CAP and int(got.status[3]) & ST_CAP
    t = int(want.off[fit])
    assert torch.equal(got.flags[:t], torch.from_numpy(want.flags[:t])) and torch.equal(got.wc[:t], torch.from_numpy(want.wc[:t]))
    assert (got.flags[t:] == 0xEE).all()
    assert (got.wc[t:] == (0 if mode == "reverse" else -77)).all()
    assert torch.equal(got.off, torch.from_numpy(want.off))
    flags, wc, cnt2 = want.flags.copy(), want.wc.copy(), want.cnt2.copy()
    if mode == "reverse":                             # rows that do not fit and were swept from the target's side: no cn2 entry
        deg = WM.degrees(c.rowptr)
        for e in range(fit, B):
            if WC.walk_reverse_rule(nds, c.src[e], c.dst[e], deg[c.src[e]], deg[c.dst[e]]):
                flags[want.off[e]:want.off[e + 1]] &= 1
                wc[want.off[e]:want.off[e + 1]] = 0
                cnt2[e] = 0
        assert (cnt2 != want.cnt2).any()
    assert torch.equal(got.cnt1, torch.from_numpy(want.cnt1)) and torch.equal(got.cnt2, torch.from_numpy(cnt2))
    assert torch.equal(got.hist, torch.from_numpy(WM.hist_of(c.rowptr, c.col, c.src, flags, wc)))
