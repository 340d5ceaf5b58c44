"""A numpy restatement of ``ocn_segment_keep_best`` (include/ocn_hip.h), for the tests: the ``topk_key`` of every score, a
sort by the uint64 key, the first ``min(m, len)``, their positions ascending.  No radix, no histogram, no compaction — the
contract, not the kernel."""
import numpy as np


def image(scores: np.ndarray) -> np.ndarray:
    """The high word of ``topk_key`` (topk_key.h): the monotone uint32 image of an fp32 score — -0.0 folded onto +0.0, a
    negative number's bits inverted, a non-negative one's sign bit set, every NaN 0."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    b = scores.view(np.uint32).copy()
    b[b == np.uint32(0x80000000)] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    u = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    u[np.isnan(scores)] = 0
    return u


def keys(segment: np.ndarray) -> np.ndarray:
    """``topk_key`` of every entry of one segment: image in the high word, ~(position in the segment) in the low word."""
    n = segment.shape[0]
    low = np.uint64(0xffffffff) - np.arange(n, dtype=np.uint64)
    return (image(segment).astype(np.uint64) << np.uint64(32)) | low


def order(segment: np.ndarray) -> np.ndarray:
    """The positions of a segment, best first: descending key (keys are distinct)."""
    return np.argsort(keys(segment), kind="stable")[::-1]


def keep_best(scores: np.ndarray, ptr: np.ndarray, m: int):
    """(``ptr_m`` int64 [Q + 1], ``keep_pos`` int64 [ptr_m[-1]], ``cut`` uint64 [Q]): per segment the flat positions of the
    ``min(m, len)`` best entries, ascending, and the key of the worst of them (0 for an empty segment)."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    ptr = np.asarray(ptr, dtype=np.int64)
    Q = ptr.shape[0] - 1
    ptr_m = np.zeros(Q + 1, dtype=np.int64)
    keep, cut = [], np.zeros(Q, dtype=np.uint64)
    for q in range(Q):
        seg = scores[ptr[q]:ptr[q + 1]]
        k = keys(seg)
        first = np.argsort(k, kind="stable")[::-1][:m]
        keep.append(np.sort(first) + ptr[q])
        ptr_m[q + 1] = ptr_m[q] + first.shape[0]
        if first.shape[0]:
            cut[q] = k[first[-1]]
    keep_pos = np.concatenate(keep).astype(np.int64) if keep else np.zeros(0, dtype=np.int64)
    return ptr_m, keep_pos, cut
