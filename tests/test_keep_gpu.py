"""``ocn_segment_keep_best`` on the GPU against the numpy restatement of its contract (tests/keep_mirror.py): the kept
positions, the offsets and the cut key, ``torch.equal`` throughout.  The score families put the cut where a radix select and
an ordered compaction can go wrong: inside a tie class, in the lowest and in the highest byte of the image, across the sign,
among the NaNs.  The segment lengths straddle ``m``, the workgroup (256) and the compaction tile (1 024)."""
import numpy as np
import pytest
import torch

from tests import keep_mirror

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

MS = (1, 2, 127, 128, 129, 200, 256, 257, 1000, 4096, 6000)


def lengths_for(m):
    """Every length of the list — 0, 1, m - 1, m, m + 1, 255, 256, 257, 1 023, 1 024, 1 025, 5 000 — in one call; the empty
    segment stands at the front, in the middle and at the end, which makes fourteen segments of the twelve lengths."""
    return [0, 1, m - 1, m, m + 1, 255, 256, 0, 257, 1023, 1024, 1025, 5000, 0]


def from_bits(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


# ---- the score families: (lengths, m, rng) -> float32 [sum(lengths)] -------------------------------------------------------
def all_equal(lens, m, rng):
    return np.full(sum(lens), 1.5, dtype=np.float32)


def three_values(lens, m, rng):                                          # the cut falls inside a tie class: r matters
    return rng.choice(np.array([1.0, 2.0, 3.0], dtype=np.float32), sum(lens))


def lowest_byte(lens, m, rng):                                           # images that differ in their last byte alone
    return from_bits(0x3f800000 | rng.integers(0, 256, sum(lens)).astype(np.uint32))


def highest_byte(lens, m, rng):
    """Images that differ in their first byte alone, all of them 0x..400000: a positive number's image is its bits with the
    sign set, a negative one's the inverted bits (so its low bits are the inverse here; 0xff would be a NaN and is left out)."""
    n = sum(lens)
    t = rng.integers(0, 128, n).astype(np.uint32)
    pos = (t << 24) | 0x00400000
    neg = 0x80000000 | (np.minimum(t, 126) << 24) | 0x00bfffff
    x = from_bits(np.where(rng.random(n) < 0.5, pos, neg))
    assert not np.isnan(x).any() and set((keep_mirror.image(x) & 0x00ffffff).tolist()) <= {0x00400000}
    return x


def mixed_signs(lens, m, rng):
    return rng.standard_normal(sum(lens)).astype(np.float32)


def signed_zeros(lens, m, rng):
    return rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], dtype=np.float32), sum(lens))


def nan_tail(lens, m, rng):
    """Every segment ends in NaNs and holds fewer numbers than ``min(m, len)``: the cut lands among the NaNs (image 0), which are
    kept by position."""
    parts = []
    for n in lens:
        seg = rng.standard_normal(n).astype(np.float32)
        seg[min(n, m) // 2:] = np.nan
        parts.append(seg)
    x = np.concatenate(parts)
    x[np.isnan(x) & (rng.random(x.shape[0]) < 0.3)] = from_bits([0xffc00001])[0]      # some of them negative, with a payload
    return x


def infinities(lens, m, rng):
    return rng.choice(np.array([np.inf, -np.inf, 0.0, 1.0, -1.0, 3e38, -3e38], dtype=np.float32), sum(lens))


def denormals(lens, m, rng):
    n = sum(lens)
    return from_bits(rng.integers(1, 0x00800000, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31))


def ascending(lens, m, rng):
    return np.concatenate([np.arange(n, dtype=np.float32) - 100.0 for n in lens])


def descending(lens, m, rng):
    return np.concatenate([100.0 - np.arange(n, dtype=np.float32) for n in lens])


FAMILIES = (all_equal, three_values, lowest_byte, highest_byte, mixed_signs, signed_zeros, nan_tail, infinities, denormals,
            ascending, descending)


def check(scores, ptr, m):
    """One launch with the cut, one without: offsets, positions and cut keys equal the mirror's."""
    from ocn_amd import ops
    want_ptr, want_keep, want_cut = keep_mirror.keep_best(scores, ptr, m)
    s, p = torch.from_numpy(np.ascontiguousarray(scores)).to(DEV), torch.from_numpy(np.asarray(ptr, dtype=np.int64)).to(DEV)
    ptr_m, keep, cut = ops.segment_keep_best(s, p, m, return_cut=True)
    assert ptr_m.dtype == keep.dtype == cut.dtype == torch.int64
    assert torch.equal(ptr_m.cpu(), torch.from_numpy(want_ptr))
    assert torch.equal(keep.cpu(), torch.from_numpy(want_keep))
    assert torch.equal(cut.cpu(), torch.from_numpy(want_cut.view(np.int64)))
    ptr2, keep2 = ops.segment_keep_best(s, p, m)
    assert torch.equal(ptr2, ptr_m) and torch.equal(keep2, keep)
    return want_ptr, want_keep


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__)
@pytest.mark.parametrize("m", MS)
def test_every_length_and_m_against_the_mirror(hiplib, family, m):
    lens = lengths_for(m)
    rng = np.random.default_rng(1000 * FAMILIES.index(family) + m)
    scores = family(lens, m, rng)
    assert scores.dtype == np.float32 and scores.shape == (sum(lens),)
    ptr = np.concatenate([[0], np.cumsum(lens)])
    want_ptr, _ = check(scores, ptr, m)
    assert (want_ptr[1:] - want_ptr[:-1]).tolist() == [min(n, m) for n in lens]


def test_three_hundred_ragged_segments_one_segment_and_none(hiplib):
    from ocn_amd import ops
    rng = np.random.default_rng(77)
    lens = rng.integers(0, 701, 300)
    lens[[0, 17, 150, 299]] = 0
    assert (lens > 150).sum() > 100 and (lens == 0).sum() >= 4
    scores = np.round(rng.standard_normal(lens.sum()) * 4).astype(np.float32) / 4                 # quarter steps: ties everywhere
    ptr = np.concatenate([[0], np.cumsum(lens)])
    check(scores, ptr, 150)
    one = rng.standard_normal(3000).astype(np.float32)
    for m in (1, 999, 3000, 3001):
        check(one, np.array([0, 3000]), m)
    check(one[:0], np.array([0]), 5)                                     # Q = 0
    ptr_m, keep = ops.segment_keep_best(torch.zeros(0, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), 300)
    assert ptr_m.tolist() == [0] and keep.shape == (0,)
    check(one[:0], np.array([0, 0, 0]), 5)                               # segments, all empty


def test_more_segments_than_workgroups(hiplib):
    """The launch has at most 2 048 workgroups: with 5 000 segments a workgroup takes several, and its LDS histogram and
    selection words are reused."""
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 40, 5000)
    scores = rng.choice(np.array([0.5, 1.0, 2.0, np.nan, -1.0], dtype=np.float32), lens.sum())
    check(scores, np.concatenate([[0], np.cumsum(lens)]), 7)


@pytest.mark.parametrize("m", (1, 64, 65, 128))
def test_within_the_top_k_limit_it_equals_the_existing_route(hiplib, m):
    """The same (ptr, edges, val) through ``recommend._keep_m_best`` — ``ocn_segment_topk``, a [Q, m] rectangle, a sort — and
    through the new selection."""
    from ocn_amd import recommend as R
    rng = np.random.default_rng(m)
    lens = np.array([0, 1, m - 1, m, m + 1, 64, 65, 127, 128, 129, 300, 0, 1000, 63, 0])
    T = int(lens.sum())
    val = torch.from_numpy(rng.choice(np.array([1.0, 2.0, 3.0, 0.5, 0.25], dtype=np.float32), T)).to(DEV)
    ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).to(DEV)
    ids = np.concatenate([np.sort(rng.choice(5000, n, replace=False)) for n in lens])
    edges = torch.from_numpy(np.stack([np.repeat(np.arange(lens.shape[0]), lens), ids], 1).astype(np.int64)).to(DEV)
    old_ptr, old_edges = R._keep_m_best(ptr, edges, val, m)
    new_ptr, new_edges = R._keep_m_long(ptr, edges, val, m)
    assert torch.equal(new_ptr, old_ptr) and torch.equal(new_edges, old_edges) and new_edges.shape[0] > 0
