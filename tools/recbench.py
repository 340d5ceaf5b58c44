"""Candidate generation of link recommendation with and without a materialised A² — ``recommend.two_hop_candidates(adj, None,
...)`` (``ocn_two_hop_diff_count`` / ``_fill``: the 2-hop set expanded from A, a workgroup per source) against
``two_hop_candidates(adj, A², ...)`` (``ocn_row_diff_*``: a wave per source over the stored product) — on a synthetic graph
of a named shape, Q random sources, each arm timed by device events:

    count / fill      — each pass of the A-only route alone (ids validated once, outside the timed calls)
    candidates        — the whole ``two_hop_candidates(adj, None, sources)`` call (two passes, the scan, its two host syncs)
    with --adj2:      — the time to form A², and the same three figures for the route through it (outputs compared)
    with --recommend: — one ``recommend_links(predictor, h, adj, None, sources, k, batch)`` call (walk-route scoring of every
                        candidate, top-k) and the share of it that candidate generation takes

    python tools/recbench.py --config collab --adj2 [--sources 4096] [--reps 20] [--out profiles/recbench_collab.log]
    python tools/recbench.py --config citation2 --recommend --predictor cn7 --hiddim 32 --batch 2048

Prints (and with ``--out`` writes) one JSON line.  No figure is a pass condition.  Needs a GPU: without one it fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sources", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--adj2", action="store_true", help="also form A² and time the route through it")
    ap.add_argument("--recommend", action="store_true", help="also time one recommend_links(adj2=None) call")
    ap.add_argument("--predictor", default="cn7")
    ap.add_argument("--hiddim", type=int, default=32)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from types import SimpleNamespace
    from ocn_amd import ops, recommend as R
    from ocn_amd.model import predictor_dict
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.synth import dataset_like
    if not torch.cuda.is_available():
        raise SystemExit("recbench needs a GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda:0")
    ei, n, _ = dataset_like(a.config, seed=0, scale=a.scale)
    adj = SparseTensor.from_edge_index(ei.to(dev), sparse_sizes=(n, n), trust_data=True).to_symmetric()
    del ei
    src = torch.randint(0, n, (a.sources,), generator=torch.Generator().manual_seed(7)).to(dev)

    def timed(fn, reps):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ts.append(t0.elapsed_time(t1))
        return dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))

    def route(rp, col, count_fn, fill_fn, cand_fn):
        with ops.prevalidated(src, src, n, n):
            off = ops.scan_i32(count_fn(rp, col, adj._rowptr, adj._col, src))
            total = int(off[-1].item())
            res = {"count_ms": timed(lambda: count_fn(rp, col, adj._rowptr, adj._col, src), a.reps),
                   "fill_ms": timed(lambda: fill_fn(rp, col, adj._rowptr, adj._col, src, off, total=total), a.reps)}
        res["candidates_call_ms"] = timed(cand_fn, a.reps)
        return res

    out = {"tool": "recbench", "config": a.config, "scale": a.scale, "nodes": n, "nnz": adj.nnz(), "max_deg": adj.max_rowcount(),
           "sources": a.sources, "reps": a.reps, "window_cols": ops.two_hop_window_cols(),
           "windows": -(-n // ops.two_hop_window_cols()), "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        ptr, edges = R.two_hop_candidates(adj, None, src)
        sizes = ptr[1:] - ptr[:-1]
        out.update(candidates=int(edges.shape[0]), longest=int(sizes.max()), empty_sources=int((sizes == 0).sum()))
        out["from_A"] = route(adj._rowptr, adj._col, ops.two_hop_diff_count, ops.two_hop_diff_fill,
                              lambda: R.two_hop_candidates(adj, None, src))
        if a.adj2:
            torch.cuda.synchronize()
            t0 = time.time()
            sp = adj.to_torch_sparse_coo_tensor()
            adj2 = SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False)
            adj2._col                                             # (the deferred fill pass: the row difference reads the ids)
            torch.cuda.synchronize()
            out["adj2_build_ms"] = round((time.time() - t0) * 1e3, 2)
            out["adj2_nnz"] = adj2.nnz()
            ptr2, edges2 = R.two_hop_candidates(adj, adj2, src)
            out["equal_to_the_route_through_adj2"] = bool(torch.equal(ptr, ptr2) and torch.equal(edges, edges2))
            out["from_adj2"] = route(adj2._rowptr, adj2._col, ops.row_diff_count, ops.row_diff_fill,
                                     lambda: R.two_hop_candidates(adj, adj2, src))
            del adj2, ptr2, edges2
        if a.recommend:
            del ptr, edges
            torch.manual_seed(0)
            H = a.hiddim
            h = torch.randn(n, H, device=dev)
            pred = predictor_dict[a.predictor](H, H, 1, 3, 0.0, 0.0, True).to(dev).eval()
            args = SimpleNamespace(sum=1.0)
            call = timed(lambda: R.recommend_links(pred, h, adj, None, src, a.k, a.batch, args), max(a.reps // 10, 1))
            out["recommend_links"] = dict(predictor=a.predictor, H=H, batch=a.batch, k=a.k, call_ms=call)
            out["candidate_share_of_recommend_links"] = round(out["from_A"]["candidates_call_ms"]["median"] / call["median"], 4)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
