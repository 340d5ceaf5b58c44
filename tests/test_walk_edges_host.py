"""The walk route's edge suite without a GPU: the exact mirror (tests/walk_mirror.py) against the oracle, the host accessor of
the route's hashes (``ocn_walk_hash``), and the premises of every constructed case of tests/test_walk_edges_gpu.py — that the
colliding element is no member and does share its bit, that a sweep which took the bitmap's "maybe" for "member" would be told
apart, that the probe chains do cross the tables' wrap.  The premises go through the library's own hash, so a change of a
multiplier or a width moves the constructed ids with it instead of turning the GPU cases into cases that test nothing."""
import numpy as np
import pytest
import torch

from ocn_amd import _lib
from oracle import ocn_oracle as O
from tests import walk_cases as WC
from tests import walk_mirror as WM


# ---------------------------------------------------------------------------------------------------------------------------
# the mirror
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_mirror_equals_the_oracle(seed):
    r = np.random.RandomState(seed)
    n, live = 70, 64                                  # nodes live .. n - 1 are isolated
    ei = r.randint(0, live, (2, 90 + 60 * seed))
    ei = torch.from_numpy(ei[:, ei[0] != ei[1]])
    oadj = O.to_symmetric(O.from_edge_index(ei, n))
    rowptr, col = oadj.rowptr().numpy(), oadj.col.numpy().astype(np.int32)
    e = r.randint(0, live, (2, 40))
    e[1, :6] = e[0, :6]                               # self-candidates
    e[:, 6:9] = [[65, 3, 66], [4, 67, 68]]            # an isolated source, an isolated target, both
    e[:, 9:12] = e[:, 12:15]                          # the same candidate twice
    e[:, 15] = [int(oadj.row[0]), int(oadj.col[0])]   # a stored edge
    B = e.shape[1]
    w = WM.mirror(rowptr, col, e[0], e[1])
    oc1, oc2 = O.get_cn1_cn2(oadj, torch.from_numpy(e))
    deg = np.diff(rowptr)
    assert w.off.tolist() == np.concatenate([[0], np.cumsum(deg[e[0]])]).tolist()
    rows = np.repeat(np.arange(B), deg[e[0]])
    cols = np.concatenate([WM.row(rowptr, col, i) for i in e[0]])
    s1, s2 = (w.flags & 1) != 0, (w.flags & 2) != 0
    assert rows[s1].tolist() == oc1.row.tolist() and cols[s1].tolist() == oc1.col.tolist()
    assert rows[s2].tolist() == oc2.row.tolist() and cols[s2].tolist() == oc2.col.tolist()
    assert w.wc[s2].tolist() == oc2.val.long().tolist() and not w.wc[~s2].any()
    assert w.cnt1.tolist() == np.bincount(oc1.row.numpy(), minlength=B).tolist()
    assert w.cnt2.tolist() == np.bincount(oc2.row.numpy(), minlength=B).tolist()
    assert w.hist[:, 0].tolist() == np.bincount(oc1.col.numpy(), minlength=n).tolist()
    assert w.hist[:, 1].tolist() == np.bincount(oc2.col.numpy(), minlength=n).tolist()
    union = np.unique(np.concatenate([oc1.row.numpy() * n + oc1.col.numpy(), oc2.row.numpy() * n + oc2.col.numpy()]))
    assert w.hist[:, 2].tolist() == np.bincount(union % n, minlength=n).tolist()
    assert w.hist[:, 3].tolist() == np.bincount(oc2.col.numpy(), weights=oc2.val.numpy(), minlength=n).astype(np.int64).tolist()
    # the prefix helper and the histogram helper agree with a mirror of the shorter batch
    p, q = WM.prefix(w, rowptr, col, e[0], 17), WM.mirror(rowptr, col, e[0, :17], e[1, :17])
    assert all(np.array_equal(a, b) for a, b in zip(p, q))


def test_shared_rule_on_the_groups_batch():
    """The restated rule of ocn_walk_prep decides the constructed groups as they were built to be decided."""
    c = WC.groups_case()
    order = np.argsort(c.src, kind="stable")
    for min_share in (2, 3):
        head, active = WM.shared_rule(c.rowptr, c.src, c.dst, order, min_share)
        assert (np.diff(head) <= 64).all() and head[0] == 0 and head[-1] == c.src.size
        got = {}
        for s, a in zip(c.src[order], active):
            got.setdefault(int(s), []).append(int(a))
        for s, (what, targets) in c.info["groups"].items():
            a = got[s]
            assert len(a) == len(targets)
            if what == "one small":
                assert sum(a) == 0
            elif what == "two small":
                assert sum(a) == (2 if min_share == 2 else 0)
            elif what == "three small":
                assert sum(a) == 3
            elif what == "keys 4096":
                assert sum(a) == 9
            elif what == "keys 4097":
                assert sum(a) == 0
            elif what == "mixed":
                assert sum(a) == 3                    # the 512-neighbour target shares, the 513-neighbour one does not
            elif what == "pair":
                assert sum(a) == (2 if min_share == 2 else 0)
            else:                                     # "65 candidates": a piece of 64 and a lone candidate, which shares with nobody
                assert sum(a) == len(a) - (len(a) % 64 if len(a) % 64 < min_share else 0)


# ---------------------------------------------------------------------------------------------------------------------------
# ocn_walk_hash
# ---------------------------------------------------------------------------------------------------------------------------
def test_walk_hash_is_an_addition_to_abi_9(hiplib):
    assert "ocn_walk_hash" in _lib.SIGNATURES and hasattr(hiplib, "ocn_walk_hash")
    assert "int32_t ocn_walk_hash(int32_t which, int32_t node);" in open(_lib.INCLUDE + "/ocn_hip.h").read()
    assert hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9


def test_walk_hash_ranges_and_known_answers(hiplib):
    n = 140_000
    for which, top in ((0, 1 << 17), (1, 1 << 17), (2, WC.SLOTS)):
        h = WC.table(hiplib, which, n)
        assert h.min() >= 0 and h.max() < top
        assert np.unique(h).size > top // 2                      # it does spread
    for which in (-1, 3, 4, 1 << 20):
        assert hiplib.ocn_walk_hash(which, 1) == -1              # OCN_EINVAL
    for v in (0x7fffffff, -1, -(1 << 31)):                       # any int32 is hashed, none is refused
        assert 0 <= hiplib.ocn_walk_hash(0, v) < 1 << 17 and 0 <= hiplib.ocn_walk_hash(2, v) < WC.SLOTS
    h0, h1, h2 = (WC.table(hiplib, w, n) for w in range(3))
    # the first two ids that share a bit of the per-candidate bitmap / of the shared sweep's: beyond every random-graph test
    assert h0[1] == h0[50550] and np.unique(h0[:50550]).size == 50550
    assert h1[1] == h1[57461] and np.unique(h1[:57461]).size == 57461
    assert [int(h2[v]) for v in (6765, 17711, 28657)] == [WC.SLOTS - 1] * 3


# ---------------------------------------------------------------------------------------------------------------------------
# premises of the GPU cases
# ---------------------------------------------------------------------------------------------------------------------------
def _differs(a, b):
    return not (np.array_equal(a.flags, b.flags) and np.array_equal(a.wc, b.wc))


@pytest.mark.parametrize("big", [False, True])
def test_premises_of_the_per_candidate_collisions(hiplib, big):
    c = WC.bloom_case(hiplib, big)
    bits = WC.table(hiplib, 0, c.rowptr.size - 1)
    exact = WM.mirror(c.rowptr, c.col, c.src, c.dst)
    seen = set()
    for g in c.info["gadgets"]:
        probed = WM.row(c.rowptr, c.col, g["probed"])
        assert probed.size == (4097 if big else 3)
        assert g["elem"] not in probed and g["member"] in probed and bits[g["elem"]] == bits[g["member"]]
        assert {"before": g["elem"] < probed[0], "after": g["elem"] > probed[-1],
                "between": probed[0] < g["elem"] < probed[-1]}[g["where"]]
        e = g["e"]
        i, j = int(c.src[e]), int(c.dst[e])
        if g["kind"] == "fwd":            # swept from i's side, probed against N(j)
            assert g["probed"] == j and any(g["elem"] in WM.row(c.rowptr, c.col, k) for k in WM.row(c.rowptr, c.col, i))
        elif g["kind"] == "rev":          # swept from j's side, probed against N(i)
            assert g["probed"] == i and any(g["elem"] in WM.row(c.rowptr, c.col, m) for m in WM.row(c.rowptr, c.col, j))
        else:                             # a neighbour of i, tested against N(j)
            assert g["probed"] == j and g["elem"] in WM.row(c.rowptr, c.col, i)
        side = "rev" if g["kind"] == "rev" else "fwd"
        one = WM.mirror(c.rowptr, c.col, c.src[e:e + 1], c.dst[e:e + 1], bloom_only=0, side=side, bits=bits)
        assert _differs(one, WM.prefix(WM.mirror(c.rowptr, c.col, c.src[e:e + 1], c.dst[e:e + 1]), c.rowptr, c.col, c.src[e:e + 1], 1))
        if g["kind"] == "f1":
            assert not np.array_equal(one.flags & 1, exact.flags[exact.off[e]:exact.off[e + 1]] & 1)
        else:
            assert not np.array_equal(one.wc, exact.wc[exact.off[e]:exact.off[e + 1]])
        seen.add((g["kind"], g["where"]))
    assert len(seen) == 9


def test_premises_of_the_hit_queue_cases(hiplib):
    c = WC.block_case()
    bits = WC.table(hiplib, 0, c.rowptr.size - 1)
    passes, total = WC.first_round_passes(c, bits)
    assert total == 2 * WC.ROUND and passes == WC.ROUND > WC.QUEUE        # every swept element passes: the queue overflows
    w = WM.mirror(c.rowptr, c.col, c.src[:1], c.dst[:1])
    assert (w.wc == c.info["walks"]).all() and w.wc.size == c.info["rows"] and (w.flags == 2).all()
    for n_pass in (512, 513):
        c = WC.flush_case(hiplib, n_pass)
        passes, total = WC.first_round_passes(c, WC.table(hiplib, 0, c.rowptr.size - 1))
        assert total > WC.ROUND and passes == n_pass                     # QUEUE / 2 is met and not exceeded / exceeded by one
    assert WC.QUEUE // 2 == 512


@pytest.mark.parametrize("cluster", [False, True])
def test_premises_of_the_shared_sweep_collision(hiplib, cluster):
    c = WC.group_bloom_case(hiplib, cluster)
    n = c.rowptr.size - 1
    h1, h2 = WC.table(hiplib, 1, n), WC.table(hiplib, 2, n)
    keys = WC.group_keys(c)
    m, x = c.info["elem"], c.info["member"]
    assert m not in keys and x in keys and h1[m] == h1[x]
    i = int(c.src[0])
    assert (c.src == i).all() and any(m in WM.row(c.rowptr, c.col, k) for k in WM.row(c.rowptr, c.col, i))      # it is swept
    used, _ = WC.occupied(keys, h2)
    assert WC.probes(m, used, h2) == (3 if cluster else 0)
    head, active = WM.shared_rule(c.rowptr, c.src, c.dst, np.arange(c.src.size), 2)
    assert active.all() and head.tolist() == [0, 2]                     # the two candidates do share a sweep
    exact = WM.mirror(c.rowptr, c.col, c.src, c.dst)
    assert _differs(exact, WM.mirror(c.rowptr, c.col, c.src, c.dst, bloom_only=1, bits=h1))


def test_premises_of_the_wrap_cases(hiplib):
    c = WC.wrap_sweep_case(hiplib)
    n = c.rowptr.size - 1
    h1, h2 = WC.table(hiplib, 1, n), WC.table(hiplib, 2, n)
    keys = WC.group_keys(c)
    used, slot_of = WC.occupied(keys, h2)
    assert {WC.SLOTS - 3, WC.SLOTS - 2, WC.SLOTS - 1, 0, 1} <= used and 2 not in used
    disp = c.info["displaced"]
    assert all(int(h2[v]) == WC.SLOTS - 1 and v in keys for v in disp)
    assert sorted(slot_of[v] for v in disp) == [0, 1, WC.SLOTS - 1]      # whichever of the three gets the home slot
    swept = np.concatenate([WM.row(c.rowptr, c.col, k) for k in WM.row(c.rowptr, c.col, int(c.src[0]))])
    assert all(v in swept for v in disp)                                # the displaced keys are looked up
    z, y = c.info["elem"], c.info["member"]
    assert z in swept and z not in keys and y in keys and h1[z] == h1[y] and h2[z] >= WC.SLOTS - 3
    assert WC.probes(z, used, h2) >= 3 and (int(h2[z]) + WC.probes(z, used, h2)) % WC.SLOTS == 2     # ... across the wrap
    head, active = WM.shared_rule(c.rowptr, c.src, c.dst, np.arange(c.src.size), 2)
    assert active.all() and head.tolist() == [0, c.src.size]
    exact = WM.mirror(c.rowptr, c.col, c.src, c.dst)
    assert exact.wc.any() and _differs(exact, WM.mirror(c.rowptr, c.col, c.src, c.dst, bloom_only=1, bits=h1))
    # the prep's source table: distinct sources, probed linearly with the same hash
    c = WC.wrap_prep_case(hiplib)
    h2 = WC.table(hiplib, 2, c.rowptr.size - 1)
    srcs = np.unique(c.src)
    assert srcs.tolist() == sorted(c.info["sources"]) and srcs.size == 7
    used, _ = WC.occupied(srcs, h2)
    assert used == {WC.SLOTS - 2, WC.SLOTS - 1, 0, 1, 2, 3, 4}


def test_premises_of_the_size_cases():
    c = WC.sizes_case()
    deg = WM.degrees(c.rowptr)
    assert sorted(set(deg[c.src[:81]])) == sorted(WC.SRC_DEGS) and sorted(set(deg[c.dst[:81]])) == sorted(WC.TGT_DEGS)
    assert deg[c.src[-3:]].tolist() == [4095, 4096, 4097]               # the probed rows of the sweep from the target's side
    true = WM.neighbor_degree_sum(c.rowptr, c.col)
    rev = [WC.walk_reverse_rule(true, i, j, deg[i], deg[j]) for i, j in zip(c.src, c.dst)]
    assert any(rev) and not all(rev)                                    # the true costs send some rows to either side
    forced = WC.forced_reverse(c)
    assert all(WC.walk_reverse_rule(forced, i, j, deg[i], deg[j]) == (deg[i] > 0 and deg[j] > 0 and i != j)
               for i, j in zip(c.src, c.dst))
