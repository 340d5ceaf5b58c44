"""GPU suite: ocn_cn_colsum_exact hand-fed (tests/colsum_cases.py) against the numpy float32 mirror (tests/colsum_mirror.py).
Every comparison is bit equality of S2 (and S3 for cn6) on every column the entry writes; a column it must not write keeps
the sentinel the output was filled with.  tests/test_colsum_host.py holds the conditions under which these cases can tell a
wrong order from the right one, and under which each sort path is reached."""
import functools

import numpy as np
import pytest
import torch

from ocn_amd import ops
from ocn_amd._lib import ptr, stream_ptr
from tests import colsum_cases as C
from tests import colsum_mirror as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = np.float32(-12345.678)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(lib, case, ip, rows=None, s2_init=None, keep=None):
    """One call of the C entry on the case (``rows``: an edge shard's row range) with sentinel-filled outputs.
    ``keep``: a dict that carries the workspace and the statistics scratch over to the next call."""
    rowptr, col, src, off, fa, fb, wc, hist = (_dev(a) for a in C.args(case, rows))
    N, cap = case.N, case.flagsA.size
    s2 = torch.full((N,), float(SENTINEL), dtype=torch.float32, device=DEV)
    s3 = torch.full((N,), float(SENTINEL), dtype=torch.float32, device=DEV) if fb is not None else None
    init = _dev(s2_init)
    inner = torch.tensor([ip], dtype=torch.float32, device=DEV)
    keep = {} if keep is None else keep
    if "ws" not in keep:
        keep["ws"] = torch.empty(int(lib.ocn_cn_colsum_workspace_bytes(N, cap)) // 8 + 1, dtype=torch.int64, device=DEV)
        keep["scal"] = torch.zeros(4, dtype=torch.int32, device=DEV)
    rc = lib.ocn_cn_colsum_exact(ptr(rowptr), ptr(col), ptr(src), src.numel(), ptr(off), ptr(fa), ptr(fb), ptr(wc), cap, ptr(hist), N,
                                 ptr(inner), ptr(keep["scal"]), ptr(init), ptr(s2), ptr(s3), ptr(keep["ws"]), stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return s2.cpu().numpy(), None if s3 is None else s3.cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(maker, key, ip):
    """The mirror's sums of a whole case: computed once, shared by the tests, read only."""
    return M.colsum(*C.args(maker(*key)), ip)


def assert_bits(case, got, want, written, what):
    """``got`` == ``want`` in bits on the written columns, the sentinel on the others; names the first columns that differ
    with their entry counts (the length and the layout name the path)."""
    gb, wb = M.bits(got), M.bits(want)
    bad = np.flatnonzero(written & (gb != wb))
    if bad.size:
        length = np.bincount(M.union_entries(*C.args(case)[:6])[0], minlength=case.N)
        pytest.fail("%s %s/%s: %d columns differ, first (column, entries, got, want): %s" % (
            what, case.name, case.variant, bad.size, [(int(c), int(length[c]), float(got[c]), float(want[c])) for c in bad[:8]]))
    assert (gb[~written] == M.bits(SENTINEL)).all(), "%s %s: a column that is not part of the batch was written" % (what, case.name)


def check(lib, case, ref, ip, **kw):
    s2, s3 = run(lib, case, ip, **kw)
    assert_bits(case, s2, ref.s2, ref.written, "S2 at innerprod %g" % ip)
    if case.flagsB is not None:
        assert_bits(case, s3, ref.s3, ref.written, "S3 at innerprod %g" % ip)
    return s2, s3


@pytest.mark.parametrize("ip", C.INNERPRODS)
@pytest.mark.parametrize("variant", C.VARIANTS)
def test_length_ladder(hiplib, variant, ip):
    """Columns of exactly 1, 2, 3, 63 .. 65, 127 .. 129, 255 .. 257, 511 .. 513, 2047 .. 2049, 4095 .. 4097 and 5000 entries in
    one batch of 5000 rows — every path's first and last length —, next to an untouched column, a closed-form one and (cn6) one
    that has cn3 entries only: plain cn5, walk counts of 1 .. 5, and cn6 with entries outside the stage-1 union (S2 and S3)."""
    case = C.ladder(variant)
    check(hiplib, case, reference(C.ladder, (variant,), ip), ip)


def test_length_ladder_through_ops(hiplib):
    """The same through ops.cn_colsum_exact (which allocates outputs and workspace itself), on the columns it writes."""
    for variant in C.VARIANTS:
        case, ip = C.ladder(variant), C.INNERPRODS[0]
        ref = reference(C.ladder, (variant,), ip)
        s2, s3 = ops.cn_colsum_exact(*(_dev(a) for a in C.args(case)), torch.tensor([ip], device=DEV),
                                     torch.zeros(4, dtype=torch.int32, device=DEV))
        w = ref.written
        assert np.array_equal(M.bits(s2.cpu().numpy())[w], M.bits(ref.s2)[w])
        assert (s3 is None) == (variant != "cn6") and (s3 is None or np.array_equal(M.bits(s3.cpu().numpy())[w], M.bits(ref.s3)[w]))


@pytest.mark.parametrize("variant", C.VARIANTS)
@pytest.mark.parametrize("layout", [l for l in C.LAYOUTS if l != "even"])
def test_position_layouts(hiplib, layout, variant):
    """Where the positions of the columns of 513 .. 4096 entries lie in the flag buffer decides how they are sorted ("even",
    the bucket sort with a few entries per bin, is test_length_ladder's).  "tail": a flag buffer 64 times longer than the batch
    needs, as in production — every position in the first bins, the bitonic network.  "rows": members in consecutive rows, 58
    entries per bin — the network.  "full" / "over": bins of exactly CS_BIN_MAX entries — the bucket sort at its limit — and of
    one more."""
    case = C.layout_case(variant, layout)
    for ip in C.INNERPRODS:
        check(hiplib, case, reference(C.layout_case, (variant, layout), ip), ip)


@pytest.mark.parametrize("cuts", C.SHARD_CUTS, ids=lambda c: "%d-shards" % (len(c) - 1))
@pytest.mark.parametrize("variant", ("plain", "valued"))
def test_edge_shards_chain_to_the_single_call(hiplib, variant, cuts):
    """The ladder's rows split into contiguous ranges, s2_init chained through the calls from zeros (the same flag buffer, the
    global hist): every intermediate vector equals the mirror's, the last one the single call's.  The "early" column has all
    its entries in the first shard and is passed through; the closed-form column is written from the global counts."""
    case = C.ladder(variant)
    for ip in C.INNERPRODS:
        ref = reference(C.ladder, (variant,), ip)
        single, _ = check(hiplib, case, ref, ip)
        run_g = run_m = np.zeros(case.N, np.float32)
        everything = np.ones(case.N, bool)
        for rows in zip(cuts[:-1], cuts[1:]):
            run_m = M.colsum(*C.args(case, rows), ip, s2_init=run_m).s2
            run_g, _ = run(hiplib, case, ip, rows=rows, s2_init=run_g)
            assert_bits(case, run_g, run_m, everything, "rows %d..%d at innerprod %g" % (rows + (ip,)))
        w = ref.written
        assert np.array_equal(M.bits(run_g)[w], M.bits(single)[w]) and np.array_equal(M.bits(run_g)[w], M.bits(ref.s2)[w])
        assert not run_g[~w].any()


def test_integer_sums_from_two_to_the_24_are_ordered(hiplib):
    """Walk counts, t = 0 in every column: walks = 2^24 - 1 is written in closed form, walks > 2^24 (twenty entries of
    2^21 or 2^21 + 1) is the sequential fp32 sum — which is neither float(walks) nor the sum in another order (host test)."""
    case = C.two24()
    ref = reference(C.two24, (), 0.37)
    s2, _ = check(hiplib, case, ref, 0.37)
    assert s2[0] == float((1 << 24) - 1) and s2[1] == ref.s2[1] != np.float32(M.hist_counts(case.hist)[3][1])


@pytest.mark.parametrize("variant", ("plain", "cn6"))
def test_more_columns_than_workgroups(hiplib, variant):
    """1000 columns of 513 .. 600 entries for the long kernel's 768 workgroups (some draw a second ticket and reuse their LDS)
    and 5000 of 65 .. 70 for the medium kernel's 1024 x 4 waves."""
    case = C.many(variant)
    check(hiplib, case, reference(C.many, (variant,), C.MANY_IP), C.MANY_IP)


@pytest.mark.parametrize("variant", ("plain", "valued"))
def test_no_column_with_two_cn1_entries(hiplib, variant):
    """nip = innerprod, t = 0 everywhere: every touched column — of up to 600 entries — is n2 (or walks), none is sorted."""
    case = C.singletons(variant)
    s2, _ = check(hiplib, case, reference(C.singletons, (variant,), 0.37), 0.37)
    n2, walks = M.hist_counts(case.hist)[1], M.hist_counts(case.hist)[3]
    touched = case.hist[:, 0] != 0
    assert np.array_equal(s2[touched], (walks if variant == "valued" else n2)[touched].astype(np.float32))


def test_empty_batch_writes_nothing(hiplib):
    """B = 0, N > 0, a zero histogram: returns 0 and leaves s2 alone."""
    N = 1000
    s2 = torch.full((N,), float(SENTINEL), dtype=torch.float32, device=DEV)
    hist = torch.zeros(N, 2, dtype=torch.int64, device=DEV)
    inner = torch.tensor([0.37], dtype=torch.float32, device=DEV)
    scal = torch.zeros(4, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(hiplib.ocn_cn_colsum_workspace_bytes(N, 0)) // 8 + 1, dtype=torch.int64, device=DEV)
    rc = hiplib.ocn_cn_colsum_exact(None, None, None, 0, None, None, None, None, 0, ptr(hist), N, ptr(inner), ptr(scal), None,
                                    ptr(s2), None, ptr(ws), stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and (M.bits(s2.cpu().numpy()) == M.bits(SENTINEL)).all()


@pytest.mark.parametrize("maker,key,ip", [(C.ladder, ("cn6",), C.INNERPRODS[1]), (C.many, ("plain",), C.MANY_IP)],
                         ids=["ladder-cn6", "many-plain"])
def test_second_call_on_the_same_workspace(hiplib, maker, key, ip):
    """The entry zeroes its own tickets, list counters and scan state: a second call on the workspace (and the statistics
    scratch) the first one left gives the same bits."""
    case, ref, keep = maker(*key), reference(maker, key, ip), {}
    first = check(hiplib, case, ref, ip, keep=keep)
    second = check(hiplib, case, ref, ip, keep=keep)
    assert np.array_equal(M.bits(first[0]), M.bits(second[0]))
    assert first[1] is None or np.array_equal(M.bits(first[1]), M.bits(second[1]))
