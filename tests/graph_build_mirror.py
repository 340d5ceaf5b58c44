"""Plain CPU restatements of the graph-build kernels (coo_csr.hip / rowsort.h, spgemm.hip, dense_adj2.hip): python ints and
sets, or torch int64 on the CPU, nothing of the product.  Everything here is integer and order-canonical, so the GPU tests
(tests/test_graph_build_gpu.py) compare with ``torch.equal``; tests/test_graph_build_host.py holds these functions against
brute force on inputs small enough to enumerate."""
import torch


def _i64(t):
    return torch.as_tensor(t).detach().cpu().to(torch.int64)


def csr_of_coo(row, col, n_rows, n_cols, symmetrize, dedupe):
    """(rowptr int64[n_rows + 1], col int32) of the entries (row[q], col[q]) — plus the transposed entries with
    ``symmetrize`` — sorted by (row, col), duplicates dropped with ``dedupe``."""
    row, col = _i64(row), _i64(col)
    if symmetrize:
        assert n_rows == n_cols
        row, col = torch.cat([row, col]), torch.cat([col, row])
    if row.numel():
        assert 0 <= int(row.min()) and int(row.max()) < n_rows and 0 <= int(col.min()) and int(col.max()) < n_cols
    key = row * n_cols + col                                             # < 2^62: n_rows, n_cols < 2^31
    key = torch.unique(key) if dedupe else torch.sort(key).values
    r, c = torch.div(key, n_cols, rounding_mode="floor"), key % n_cols
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(r, minlength=n_rows), 0)
    return rowptr, c.to(torch.int32)


def rows_of(rowptr, col):
    """The CSR as a python list of per-row column lists."""
    rp, c = _i64(rowptr).tolist(), _i64(col).tolist()
    return [c[rp[r]:rp[r + 1]] for r in range(len(rp) - 1)]


def csr_of_rows(rows):
    """(rowptr int64, col int32) of per-row column collections, ascending per row."""
    rowptr, col = [0], []
    for cols in rows:
        col.extend(sorted(cols))
        rowptr.append(len(col))
    return torch.tensor(rowptr, dtype=torch.int64), torch.tensor(col, dtype=torch.int32)


def pattern_of_product(rowptrA, colA, rowptrB, colB, n_cols_b):
    """(rowptrC, colC) of the pattern of A·B: row r is the union of B's rows named by A's row r, ascending."""
    B = rows_of(rowptrB, colB)
    out = []
    for cols in rows_of(rowptrA, colA):
        s = set()
        for m in cols:
            s.update(B[m])
        assert all(0 <= k < n_cols_b for k in s)
        out.append(s)
    return csr_of_rows(out)


def bit_rows(rowptr, col, n_cols, stride_words):
    """int32 [n_rows, stride_words]: column c of row r is bit ``c & 31`` of word ``c >> 5``; every bit at or beyond ``n_cols``
    and every padding word stays zero."""
    rowptr, col = _i64(rowptr), _i64(col)
    n = rowptr.numel() - 1
    assert stride_words * 32 >= n_cols
    if col.numel():
        assert 0 <= int(col.min()) and int(col.max()) < n_cols
    r = torch.repeat_interleave(torch.arange(n, dtype=torch.int64), rowptr[1:] - rowptr[:-1])
    key = torch.unique(r * n_cols + col)                                 # a bit is set once however often it is listed
    r, c = torch.div(key, n_cols, rounding_mode="floor"), key % n_cols
    words = torch.zeros(n * stride_words, dtype=torch.int64)
    words.index_add_(0, r * stride_words + (c >> 5), torch.ones_like(c) << (c & 31))
    words = torch.where(words >= 1 << 31, words - (1 << 32), words)      # the same 32 bits as a signed word
    return words.to(torch.int32).reshape(n, stride_words)


def cols_of_bit_rows(bits, n_cols):
    """(rowptr int64, col int32) of the set bits below ``n_cols`` in the first ceil(n_cols / 32) words of every row, ascending.
    Words beyond those are padding and are not looked at; a set bit at or beyond ``n_cols`` in the last word is an error."""
    bits = _i64(bits)
    n, words = bits.shape[0], (n_cols + 31) // 32
    assert bits.shape[1] >= words
    w = bits[:, :words] & 0xFFFFFFFF
    on = ((w.unsqueeze(-1) >> torch.arange(32, dtype=torch.int64)) & 1).reshape(n, words * 32)
    assert not on[:, n_cols:].any(), "a bit beyond n_cols is set"
    r, c = torch.nonzero(on[:, :n_cols], as_tuple=True)                  # row-major: ascending column per row
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
    return rowptr, c.to(torch.int32)


def dense_of_csr(rowptr, col, n_rows, n_cols):
    d = torch.zeros(n_rows, n_cols, dtype=torch.int64)
    for r, cols in enumerate(rows_of(rowptr, col)):
        for c in cols:
            d[r, c] = 1
    return d


def csr_of_dense(d):
    r, c = torch.nonzero(d, as_tuple=True)
    rowptr = torch.zeros(d.shape[0] + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(r, minlength=d.shape[0]), 0)
    return rowptr, c.to(torch.int32)


def block_adj2(rowptr, col, n, block, fold):
    """The tile loop of ``ops.dense_block_adj2`` on a dense 0/1 integer matrix: every (row block, column block) of ``block``
    multiplied on its own, the non-zero pattern ORed into an n x n 0/1 matrix — at its own place, or with ``fold`` at
    (row - r0, col - c0): every block on the top-left corner."""
    A = dense_of_csr(rowptr, col, n, n)
    out = torch.zeros(n, n, dtype=torch.int64)
    for r0 in range(0, n, block):
        r1 = min(r0 + block, n)
        for c0 in range(0, n, block):
            c1 = min(c0 + block, n)
            nz = ((A[r0:r1] @ A[:, c0:c1]) > 0).to(torch.int64)
            if fold:
                out[:r1 - r0, :c1 - c0] |= nz
            else:
                out[r0:r1, c0:c1] |= nz
    return out
