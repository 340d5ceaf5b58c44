"""Ranking held-out links at a named shape (collab by default): what ``ocn_segment_rank`` costs beside ``ocn_segment_topk`` and
beside a torch restatement of the same ranks, and what the candidate lists and short lists of ``ocn_amd.recommend`` keep of
held-out edges.  Device events around every call, warm-up, medians and ranges.  One GPU process at a time: every arm runs in a
child of its own under its own time limit, and the first arm that fails or runs over ends the tool.

    k   the kernels, Q random sources as in tools/hop3bench.py, one target per source (a member of its list where it has one):
        on the 2-hop list (``two_hop_scored_candidates(adj, src, "ra")``) and on the 3-hop list (``path_scored_candidates(adj,
        src, "ra", 3, D)``) the time of ``ops.segment_rank``, of ``ops.segment_topk(k=128)``, and of the ranks restated in torch
        — ``repeat_interleave`` + comparison + segmented integer sum — whose result is compared with the kernel's in the run;
    m   the metrics: the training graph and the held-out test edges of ``synth.loaddataset_like``, the first Q distinct test
        sources: ``coverage`` at ``hops=2`` against ``hops=3`` and the ``retention`` of ("ra", 32) and ("ra", 128) at both, from
        one ``rank_path_index`` call each (a short list of m keeps the targets with ``1 <= rank <= m``), and its time.

    python tools/rankbench.py --out profiles/rankbench_collab.json

Prints (and with ``--out`` writes) one JSON line.  No figure is a pass condition.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("k", "m")


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    from ocn_amd import ops, ranking as K, recommend as R
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.synth import dataset_like, loaddataset_like
    if not torch.cuda.is_available():
        raise SystemExit("rankbench needs a GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda:0")
    D = a.decay

    def run_arms(arms, reps, warmup=a.warmup):
        for fn in arms.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
        ts = {name: [] for name in arms}
        for _ in range(reps):
            for name, fn in arms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                ts[name].append(round(t0.elapsed_time(t1), 4))
        return ts

    out = {"arm": a.arm}
    with torch.no_grad():
        if a.arm == "k":
            ei, n, _ = dataset_like(a.config, seed=0, scale=a.scale)
            adj = SparseTensor.from_edge_index(ei.to(dev), sparse_sizes=(n, n), trust_data=True).to_symmetric()
            del ei
            Q = a.sources
            src = torch.randint(0, n, (Q,), generator=torch.Generator().manual_seed(7)).to(dev)
            out.update(nodes=n, nnz=adj.nnz(), max_deg=adj.max_rowcount(), lists={})
            tptr = torch.arange(Q + 1, device=dev)
            draw = torch.randint(0, 1 << 40, (Q,), generator=torch.Generator().manual_seed(8)).to(dev)
            for name, make in (("hops2", lambda: R.two_hop_scored_candidates(adj, src, "ra")),
                               ("hops3", lambda: R.path_scored_candidates(adj, src, "ra", 3, D))):
                ptr, edges, val = make()
                size = ptr[1:] - ptr[:-1]
                at = ptr[:-1] + draw % size.clamp(min=1)                 # a member of every list that has one
                tnode = torch.where(size > 0, edges[at.clamp(max=max(edges.shape[0] - 1, 0)), 1], torch.full_like(at, -1))
                rank, pos = ops.segment_rank(val, ptr, edges, tptr, tnode)

                def restated():
                    seg = torch.repeat_interleave(torch.arange(Q, device=dev), size)
                    tv = val[at.clamp(max=val.numel() - 1)][seg]
                    ahead = (val > tv) | ((val == tv) & (torch.arange(val.numel(), device=dev) < at[seg]))   # (path sums: no NaN, no -0.0)
                    return torch.where(size > 0, 1 + torch.zeros(Q, dtype=torch.int64, device=dev).index_add_(0, seg, ahead.long()),
                                       torch.zeros_like(size))
                equal = bool(torch.equal(restated(), rank) and torch.equal(pos, torch.where(size > 0, at, torch.full_like(at, -1))))
                ms = run_arms({"segment_rank": lambda: ops.segment_rank(val, ptr, edges, tptr, tnode),
                               "segment_topk_128": lambda: ops.segment_topk(val, ptr, 128),
                               "torch_restatement": restated}, a.reps)
                out["lists"][name] = dict(candidates=int(ptr[-1]), longest=int(size.max()), targets=Q, found=int((rank > 0).sum()),
                                          median_rank=int(rank[rank > 0].median()) if bool((rank > 0).any()) else 0,
                                          ranks_equal_torch=equal, ms=ms)
                del ptr, edges, val, rank, pos
        else:
            data, split_edge = loaddataset_like(a.config, False, scale=a.scale)
            adj = data.adj_t.to_device(dev)
            n = adj.size(0)
            test = split_edge["test"]["edge"].to(dev)
            src = torch.tensor(list(dict.fromkeys(test[:, 0].tolist()))[:a.sources], dtype=torch.int64, device=dev)
            truth = SparseTensor.from_edge_index(test.t().contiguous(), sparse_sizes=(n, n)).to_symmetric()
            out.update(nodes=n, nnz=adj.nnz(), max_deg=adj.max_rowcount(), test_edges=int(test.shape[0]), sources=int(src.numel()), hops={})
            for hops in (2, 3):
                call = (lambda: K.rank_path_index(adj, src, truth, "ra", 2)) if hops == 2 else \
                    (lambda: K.rank_path_index(adj, src, truth, "ra", 3, decay=D))
                res = call()
                met = K.ranking_metrics(res, ks=(10, 32, 128))
                cand = int((res.rank > 0).sum())
                out["hops"][str(hops)] = dict(
                    pairs=met["n_pairs"], candidates=int(res.n_cand.sum()), coverage=round(met["coverage"], 6),
                    retention_ra_32=round(int(((res.rank >= 1) & (res.rank <= 32)).sum()) / max(cand, 1), 6),
                    retention_ra_128=round(int(((res.rank >= 1) & (res.rank <= 128)).sum()) / max(cand, 1), 6),
                    mrr=round(met["mrr"], 6), recall_at_10=round(met["recall@10"], 6), ndcg_at_10=round(met["ndcg@10"], 6),
                    ms=run_arms({"rank_path_index": call}, a.request_reps, 1))
    print("RANKBENCH " + json.dumps(out), flush=True)


def summary(samples):
    return dict(median=round(statistics.median(samples), 4), min=round(min(samples), 4), max=round(max(samples), 4), n=len(samples))


def summarise(r):
    if isinstance(r, dict):
        return {k: ({name: summary(ts) for name, ts in v.items()} if k == "ms" else summarise(v)) for k, v in r.items()}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default=None, choices=ARMS, help="(internal) run one arm")
    ap.add_argument("--arms", default="km", help="the arms to run, in this order")
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sources", type=int, default=4096)
    ap.add_argument("--decay", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--request-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=240, help="seconds one arm may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        return child(a)
    passed = [f"--{k.replace('_', '-')}={v}" for k, v in vars(a).items() if k not in ("arm", "arms", "out", "limit")]
    out = {"tool": "rankbench", "config": a.config, "scale": a.scale, "sources": a.sources, "decay": a.decay, "arms": {}}
    rc = 0
    for arm in a.arms:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm] + passed, capture_output=True, text=True,
                               timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"arm {arm}: over its {a.limit} s limit; stopping", flush=True)
            out["arms"][arm] = f"over its {a.limit} s limit"
            rc = 2
            break
        line = [l for l in p.stdout.splitlines() if l.startswith("RANKBENCH ")]
        if p.returncode != 0 or not line:
            print(f"arm {arm}: exit {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            out["arms"][arm] = f"exit {p.returncode}"
            rc = 2
            break
        r = summarise(json.loads(line[0][len("RANKBENCH "):]))
        r.pop("arm")
        out["arms"][arm] = r
        print(f"arm {arm}: done", flush=True)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
