"""Edge removal from a resident graph against the rebuild it replaces, on a synthetic graph of a named shape: per size of Δ
(undirected edges drawn from the graph), three routes to the same pair (A′, A′²), alternating in one process, each call
between two device events:

    donate      — ``update.remove_edges(adj, Δ, adj2, donate=True)``  (the bit rows of A² updated in place; the edges are put
                  back by ``insert_edges(..., donate=True)`` outside the timed call, which restores the pair exactly)
    clone       — the same with ``donate=False``                       (the bit rows are cloned first)
    rebuild     — ``from_edge_index(remaining).to_symmetric()`` plus ``A @ A`` with bit rows

The first results of the update and of the rebuild are compared (row pointers of A′ and A′², columns of A′, bit rows).  Also reported: the
number of candidate bits Δ enumerates and the share of them whose shorter list is longer than the kernel's lane limit (those
the whole wave decides), computed from the row lengths in torch.

    python tools/removebench.py --config collab [--sizes 1000,60000,1%] [--reps 7] [--out profiles/removebench_collab.log]

Prints a progress line per size, then (and with ``--out`` writes) one JSON line.  No figure is a pass condition.  Needs a GPU: without one it fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LANE_MAX = 32                  # graph_update.hip: BR_LANE_MAX


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sizes", default="1000,60000,1%", help="undirected edges per Δ; N%% = that share of the graph's edges")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.synth import dataset_like
    from ocn_amd.update import insert_edges, remove_edges
    if not torch.cuda.is_available():
        raise SystemExit("removebench needs a GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda:0")
    ei, n, _ = dataset_like(a.config, seed=0, scale=a.scale)
    adj = SparseTensor.from_edge_index(ei.to(dev), sparse_sizes=(n, n), trust_data=True).to_symmetric()
    del ei

    def product(m):
        sp = m.to_torch_sparse_coo_tensor()
        return SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        res = fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1), res

    def stats(ts):
        return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))

    row, col = adj.storage.row(), adj.storage.col().to(torch.int64)
    upper = torch.stack([row, col])[:, row < col]                  # one entry per undirected edge (self loops stay out of Δ)
    loops = torch.stack([row, col])[:, row == col]
    deg = adj.storage.rowcount()
    out = {"tool": "removebench", "config": a.config, "scale": a.scale, "nodes": n, "nnz": adj.nnz(), "max_deg": adj.max_rowcount(),
           "reps": a.reps, "device": torch.cuda.get_device_name(0), "sizes": {}}
    with torch.no_grad():
        adj2 = product(adj)
        out["adj2_bit_row_bytes"] = int(adj2.product_bit_rows().numel()) * 4
        g = torch.Generator().manual_seed(11)
        for spec in a.sizes.split(","):
            e = int(upper.shape[1] * float(spec[:-1]) / 100) if spec.endswith("%") else int(spec)
            e = min(e, upper.shape[1])
            pick = torch.randperm(upper.shape[1], generator=g)[:e].to(dev)
            keep = torch.ones(upper.shape[1], dtype=torch.bool, device=dev)
            keep[pick] = False
            delta = upper[:, pick].contiguous()
            remaining = torch.cat([upper[:, keep], loops], dim=1).contiguous()

            def rebuild():
                m = SparseTensor.from_edge_index(remaining, sparse_sizes=(n, n), trust_data=True).to_symmetric()
                return m, product(m)

            ts = {"donate": [], "clone": [], "rebuild": []}
            equal = None
            for rep in range(a.warmup + a.reps):
                t_d, (d1, d2) = timed(lambda: remove_edges(adj, delta, adj2, donate=True))
                t_r, (r1, r2) = timed(rebuild)
                if equal is None:
                    equal = bool(torch.equal(d1._rowptr, r1._rowptr) and torch.equal(d1._col, r1._col)
                                 and torch.equal(d2._rowptr, r2._rowptr)
                                 and torch.equal(d2.product_bit_rows(), r2.product_bit_rows()))
                    new_deg = d1.storage.rowcount()
                del r1, r2
                _, adj2 = insert_edges(d1, delta, d2, donate=True)         # (untimed: A′ ∪ Δ = A, the pair as it was)
                del d1, d2
                t_c, c = timed(lambda: remove_edges(adj, delta, adj2, donate=False))
                del c
                if rep >= a.warmup:
                    ts["donate"].append(t_d); ts["clone"].append(t_c); ts["rebuild"].append(t_r)
            # candidates: per directed entry (u, v) of Δ, (u, k) for k in old row v and (r, v) for r in old row u (A symmetric)
            du = torch.cat([delta[0], delta[1]])
            dv = torch.cat([delta[1], delta[0]])
            start = adj._rowptr[dv]
            cnt = deg[dv]
            owner = torch.repeat_interleave(torch.arange(du.numel(), device=dev), cnt)
            pos = torch.arange(owner.numel(), device=dev) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
            k = adj._col[start[owner] + pos].to(torch.int64)
            short = torch.minimum(new_deg[du[owner]], new_deg[k])          # kind (a); kind (b) is its mirror image
            out["sizes"][spec] = {"undirected_edges": e, "equal_to_the_rebuild": equal,
                                  "donate_ms": stats(ts["donate"]), "clone_ms": stats(ts["clone"]), "rebuild_ms": stats(ts["rebuild"]),
                                  "candidates": 2 * int(owner.numel()),
                                  "wave_cooperative_share": round(float((short > LANE_MAX).float().mean()) if owner.numel() else 0.0, 5)}
            print(json.dumps({spec: out["sizes"][spec]}), flush=True)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
