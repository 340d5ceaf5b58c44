"""Embedding retrieval (``ocn_mips_topm_i8``; ocn_amd/ops.py: ``quantize_rows_i8``, ``mips_topm_i8``; ocn_amd/recommend.py:
``EmbeddingIndex``, ``EmbeddingNeighbours``, ``ShortListUnion``) without a GPU: the symbols, the entry's argument checks, the
refusals of the Python layers, the quantiser, and the mirror of the contract on cases small enough to do by hand."""
from ctypes import c_void_p

import pytest
import torch

from ocn_amd import _lib
from tests import mips_mirror as MM

P = c_void_p(4096)             # a non-NULL, 16-byte aligned address that is never read: every call below returns before its first HIP call
Z = c_void_p(0)


def test_new_entries_are_additions_to_abi_9(hiplib):
    for name in ("ocn_mips_max_m", "ocn_mips_h_align", "ocn_mips_workspace_bytes", "ocn_mips_topm_i8"):
        assert name in _lib.SIGNATURES and hasattr(hiplib, name)
    hdr = open(_lib.INCLUDE + "/ocn_hip.h").read()
    for name in ("ocn_mips_max_m(void)", "ocn_mips_h_align(void)", "ocn_mips_workspace_bytes(", "ocn_mips_topm_i8("):
        assert name in hdr
    assert hiplib.ocn_abi_version() == _lib.ABI_VERSION == 9
    assert hiplib.ocn_mips_max_m() == hiplib.ocn_segment_topk_max_k()
    assert hiplib.ocn_mips_h_align() in (32, 64)
    assert len(_lib.SIGNATURES["ocn_mips_topm_i8"][1]) == 16


def test_entry_rejects_bad_arguments_before_any_hip_call(hiplib):
    mmax, align = hiplib.ocn_mips_max_m(), hiplib.ocn_mips_h_align()

    def topm(**kw):
        a = dict(query=P, keys=P, kscale=P, Q=4, N=100, H=2 * align, rows=P, rpM=P, cM=P, drop=1, m=10, ns=0, val=P, node=P, ws=P)
        a.update(kw)
        return hiplib.ocn_mips_topm_i8(a["query"], a["keys"], a["kscale"], a["Q"], a["N"], a["H"], a["rows"], a["rpM"], a["cM"],
                                       a["drop"], a["m"], a["ns"], a["val"], a["node"], a["ws"], Z)

    for name in ("query", "keys", "kscale", "val", "node", "ws"):
        assert topm(**{name: Z}) == -1, name
    assert topm(Q=-1) == -1
    assert topm(N=0) == -1 and topm(N=-5) == -1 and topm(N=1 << 31) == -1
    for H in (0, -align, align - 1, align + 1, 1024 + align, 3 * align // 2):
        assert topm(H=H) == -1, H
    for m in (0, -1, mmax + 1):
        assert topm(m=m) == -1, m
    assert topm(ns=-1) == -1
    assert topm(rpM=Z) == -1 and topm(cM=Z) == -1            # one half of M
    assert topm(rows=Z) == -1                                # M without rows
    assert topm(query=c_void_p(4100)) == -1                  # (fragments are read 16 bytes at a time)
    # an empty call is still checked, and a valid one launches nothing: with M, with rows alone, with neither
    assert topm(Q=0, m=0) == -1 and topm(Q=0, keys=Z) == -1 and topm(Q=0, rows=Z) == -1
    assert topm(Q=0) == 0 and topm(Q=0, rpM=Z, cM=Z) == 0 and topm(Q=0, rows=Z, rpM=Z, cM=Z) == 0
    assert topm(Q=0, H=1024, m=mmax, ns=7) == 0


def test_workspace_bytes(hiplib):
    ws = hiplib.ocn_mips_workspace_bytes
    mmax = hiplib.ocn_mips_max_m()
    assert ws(-1, 10, 1, 0) == -1 and ws(1, 0, 1, 0) == -1 and ws(1, 1 << 31, 1, 0) == -1
    assert ws(1, 10, 0, 0) == -1 and ws(1, 10, mmax + 1, 0) == -1 and ws(1, 10, 1, -1) == -1
    assert ws(0, 10, 1, 0) >= 8 and ws(5, 10, 4, 1) >= 8
    assert ws(5, 4099, 7, 3) == 5 * 3 * 7 * 8                # three partial lists of 7 keys per query
    assert ws(5, 10, 7, 16) == 8                             # no more slices than 32-key tiles: one, no partial lists
    assert ws(5, 65, 7, 16) == 5 * 3 * 7 * 8
    assert 8 <= ws(4096, 235868, 128, 0) <= 4096 * 64 * 128 * 8


def test_python_layers_refuse_misuse(hiplib):
    from ocn_amd import ops, recommend as R
    from ocn_amd.sparse import SparseTensor
    mmax = ops.mips_max_m()
    assert mmax == ops.segment_topk_max_k() and ops.mips_h_align() == hiplib.ocn_mips_h_align()
    q, k, s = torch.zeros(2, 64, dtype=torch.int8), torch.zeros(5, 64, dtype=torch.int8), torch.ones(5)
    for m in (0, -1, mmax + 1, True, 2.0):
        with pytest.raises(ValueError, match="m must be in 1.."):
            ops.mips_topm_i8(q, k, s, m)
    for m in (0, mmax + 1):
        with pytest.raises(ValueError, match="m must be in 1.."):
            R.EmbeddingNeighbours(m)
        with pytest.raises(ValueError, match="m must be in 1.."):
            R.embedding_candidates(R.EmbeddingIndex(torch.randn(5, 8)), torch.randn(2, 8), torch.tensor([0, 1]), m)
    with pytest.raises(ValueError, match="m must be an int"):
        R.EmbeddingNeighbours(4.0)
    with pytest.raises(ValueError, match="normalize must be a bool"):
        R.EmbeddingNeighbours(4, normalize=1)
    with pytest.raises(ValueError, match="keys must be None"):
        R.EmbeddingNeighbours(4, keys=torch.zeros(5, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="indexed with normalize"):
        R.EmbeddingNeighbours(4, normalize=True, keys=R.EmbeddingIndex(torch.randn(5, 8)))
    with pytest.raises(ValueError, match="n_split"):
        ops.mips_topm_i8(q, k, s, 1, n_split=-1)
    with pytest.raises(ValueError, match="at least one stage"):
        R.ShortListUnion()
    with pytest.raises(ValueError, match="a stage must be"):
        R.ShortListUnion("ra")
    # k above what the short list keeps: the existing refusal
    with pytest.raises(ValueError, match="fewer than k = 9"):
        R._check_prefilter(R.EmbeddingNeighbours(8), 9)
    with pytest.raises(ValueError, match="fewer than k = 33"):
        R._check_prefilter(R.ShortListUnion(("ra", 32), R.EmbeddingNeighbours(16)), 33)
    assert isinstance(R._check_prefilter(R.ShortListUnion(("ra", 32), R.EmbeddingNeighbours(16)), 32), R.ShortListUnion)
    with pytest.raises(ValueError, match="prefilter must be None or"):
        R._check_prefilter(R.ShortListUnion(("ra", 32, 0.5), R.EmbeddingNeighbours(16)), 4)       # a 3-tuple under hops=2
    with pytest.raises(ValueError, match="hops = 2"):
        R._check_prefilter(R.ShortListUnion(R.RandomWalks(8, 64, 3, 0.5)), 4)
    # wrong dtypes and shapes, CPU tensors
    with pytest.raises(ValueError, match="float32"):
        ops.quantize_rows_i8(torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        R.EmbeddingIndex(torch.zeros(3, 4, dtype=torch.float16))
    with pytest.raises(ValueError, match="queries must be float32"):
        R.embedding_candidates(R.EmbeddingIndex(torch.randn(5, 8)), torch.randn(2, 9), torch.tensor([0, 1]), 2)
    with pytest.raises(ValueError, match="sources must be a 1-d int64"):
        R.embedding_candidates(R.EmbeddingIndex(torch.randn(5, 8)), torch.randn(2, 8), torch.tensor([0, 1]).int(), 2)
    other = SparseTensor.from_edge_index(torch.tensor([[0, 1], [1, 0]]), sparse_sizes=(6, 6))
    with pytest.raises(ValueError, match="known is"):
        R.embedding_candidates(R.EmbeddingIndex(torch.randn(5, 8)), torch.randn(2, 8), torch.tensor([0, 1]), 2, other)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        ops.mips_topm_i8(q, k, s, 1)
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        R.embedding_candidates(R.EmbeddingIndex(torch.randn(5, 8)), torch.randn(2, 8), torch.tensor([0, 1]), 2)
    for bad in (float("nan"), float("inf"), float("-inf")):
        x = torch.randn(4, 8)
        x[2, 3] = bad
        with pytest.raises(ValueError, match="not finite"):
            ops.quantize_rows_i8(x)
        with pytest.raises(ValueError, match="not finite"):
            R.EmbeddingIndex(x)


def test_recommend_links_refusals_with_the_new_stages(hiplib):
    from ocn_amd import recommend as R
    from ocn_amd.model import predictor_dict
    from ocn_amd.sparse import SparseTensor
    adj = SparseTensor.from_edge_index(torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]), sparse_sizes=(4, 4))
    src = torch.tensor([0, 2])
    pred = predictor_dict["cn5"](8, 8, 1, 3, 0.0).eval()
    h = torch.randn(4, 8)
    with pytest.raises(ValueError, match="fewer than k = 3"):
        R.recommend_links(pred, h, adj, adj, src, 3, 64, prefilter=R.EmbeddingNeighbours(2))
    with pytest.raises(ValueError, match="fewer than k = 3"):
        R.recommend_links(pred, h, adj, adj, src, 3, 64, prefilter=R.ShortListUnion(("ra", 2), R.EmbeddingNeighbours(2)))
    with pytest.raises(_lib.OcnHipError, match="no CPU path"):
        R.recommend_links(pred, h, adj, adj, src, 2, 64, prefilter=R.EmbeddingNeighbours(2))
    with pytest.raises(ValueError, match="hold 5 nodes"):
        R.recommend_links(pred, h, adj, adj, src, 2, 64, prefilter=R.EmbeddingNeighbours(2, keys=torch.randn(5, 8)))


@pytest.mark.parametrize("normalize", [False, True])
def test_quantiser(hiplib, normalize):
    from ocn_amd import ops
    align = ops.mips_h_align()
    g = torch.Generator().manual_seed(5)
    for H in (1, 16, 48, align, align + 1, 256):
        x = torch.randn(37, H, generator=g) * torch.logspace(-3, 3, 37)[:, None]
        x[5] = 0
        x[6, : H // 2] = 0
        q, scale = ops.quantize_rows_i8(x, normalize)
        Hp = (H + align - 1) // align * align
        assert q.dtype == torch.int8 and scale.dtype == torch.float32 and q.shape == (37, Hp) and scale.shape == (37,)
        assert q.is_contiguous() and int(q.abs().max()) <= 127 and int(q.to(torch.int16).min()) >= -127
        assert not q[:, H:].any()                            # the padding
        assert float(scale[5]) == 1.0 and not q[5].any()     # an all-zero row
        ref = x
        if normalize:
            nrm = x.norm(dim=1, keepdim=True)
            ref = x / torch.where(nrm > 0, nrm, torch.ones_like(nrm))
            assert torch.allclose((q[:, :H].float() * scale[:, None]).norm(dim=1)[torch.arange(37) != 5], torch.ones(36), atol=2e-2)
        assert torch.equal(scale, torch.where(ref.abs().amax(1) > 0, ref.abs().amax(1) / 127.0, torch.ones(37)))
        assert int(q.abs().amax(1)[6]) == 127                # the largest entry of a row maps to +-127
        # |x - q * scale| <= scale / 2, up to one ulp of x / scale (<= 127): the division rounds before the rounding to an integer
        err = (ref.double() - q[:, :H].double() * scale.double()[:, None]).abs()
        assert bool((err <= scale.double()[:, None] * (0.5 + 127 * 2.0 ** -23)).all())
    q0, s0 = ops.quantize_rows_i8(torch.zeros(0, 8), normalize)
    assert q0.shape == (0, align) and s0.shape == (0,)


def test_mirror_hand_cases():
    """Four nodes, by hand."""
    i8 = lambda rows: torch.tensor(rows, dtype=torch.int8)   # noqa: E731
    ones = torch.ones(4)
    # ties: nodes 0 and 2 hold one row — the lower id first, and the cut between them keeps 0
    keys = i8([[1, 2], [3, 4], [1, 2], [0, 0]])
    query = i8([[1, 0], [0, 1], [-1, 0]])
    val, node = MM.topm(query, keys, ones, 3)
    assert node.tolist() == [[1, 0, 2], [1, 0, 2], [3, 0, 2]] and val.tolist() == [[3, 1, 1], [4, 2, 2], [0, -1, -1]]
    assert MM.topm(query, keys, ones, 2)[1].tolist() == [[1, 0], [1, 0], [3, 0]]
    # a -0.0 product: node 3 has dot 0 and a negative scale; -0.0 == +0.0, so the id decides between nodes 1 and 3
    keys = i8([[1, 0], [0, 5], [2, 0], [0, 7]])
    scale = torch.tensor([1.0, 1.0, 1.0, -2.0])
    val, node = MM.topm(i8([[1, 0]]), keys, scale, 4)
    assert node.tolist() == [[2, 0, 1, 3]] and val.tolist() == [[2.0, 1.0, 0.0, 0.0]]
    assert str(float(MM.values(i8([[1, 0]]), keys, scale)[0, 3])) == "-0.0"
    val, node = MM.topm(i8([[-1, 0]]), keys, scale, 4)       # now node 1 holds the -0.0 and still precedes node 3
    assert node.tolist() == [[1, 3, 0, 2]]
    # an excluded best node; the source itself; padding
    rp, col = torch.tensor([0, 1, 1, 1, 1]), torch.tensor([2], dtype=torch.int32)        # row 0 knows node 2
    rows = torch.tensor([0])
    val, node = MM.topm(i8([[1, 0]]), keys, scale, 4, rows, (rp, col), True)
    assert node.tolist() == [[1, 3, -1, -1]] and val[0, :2].tolist() == [0.0, 0.0] and val[0, 2:].tolist() == [float("-inf")] * 2
    assert MM.topm(i8([[1, 0]]), keys, scale, 4, rows, (rp, col), False)[1].tolist() == [[0, 1, 3, -1]]
    assert MM.topm(i8([[1, 0]]), keys, scale, 4, rows, None, True)[1].tolist() == [[2, 1, 3, -1]]
    # the ranks of the same case: node 2 is excluded (0), the source itself too, node 3 stands second
    tptr, tnode = torch.tensor([0, 5]), torch.tensor([2, 0, 3, 1, 9])
    assert MM.ranks(i8([[1, 0]]), keys, scale, rows, (rp, col), True, tptr, tnode).tolist() == [0, 0, 2, 1, 0]
    assert MM.ranks(i8([[1, 0]]), keys, scale, None, None, True, tptr, tnode).tolist() == [1, 2, 4, 3, 0]
