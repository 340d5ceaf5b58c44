"""Short lists beyond 128 at a named shape (collab by default), Q random sources as in tools/prefilterbench.py: what the
selection costs, what a whole request costs with a longer short list, and what the longer list keeps of the held-out links.
Device events around every call, warm-up, medians and ranges; the arms of an arm group are interleaved call by call.

    Arm "k", the selection on the scored 2-hop lists ("ra") of the sources: ``ops.segment_keep_best`` followed by the gather
        of the kept pairs (``recommend._keep_m_long``) against ``recommend._keep_m_best`` (``ocn_segment_topk``, a [Q, m]
        rectangle, a sort, the gather) at m = 32 and m = 128 — the results compared with ``torch.equal`` in the same run — and
        the new selection alone at m = 256, 512, 1 024.
    Arm "r", the request: ``recommend_links(..., prefilter=PathSums("ra", m))`` for every m, k = 20, cn5 at H = 256, beside
        the tuple stage at m <= 128 and the unfiltered call.
    Arm "m", the held-out links: on the test pairs of the shape, ``coverage`` (the pair is a 2-hop candidate), ``retention`` of
        every m (the share of the covered pairs a short list of m keeps) and their product, the share handed to the model —
        from one ``rank_path_index`` call: a short list of m keeps exactly the targets with ``1 <= rank <= m``.

    python tools/keepbench.py --out profiles/keepbench_collab.json

The graph is synthetic (``ocn_amd.synth``: the shape's size and degree law, not its links).  Every arm runs in a process of its
own.  Prints (and with ``--out`` writes) one JSON line.  No figure is a pass condition.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("k", "r", "m")
BOTH = (32, 128)               # m the existing route takes too
LONG = (256, 512, 1024)


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    from ocn_amd import ops, ranking as K, recommend as R
    from ocn_amd.model import predictor_dict
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.synth import dataset_like, loaddataset_like
    if not torch.cuda.is_available():
        raise SystemExit("keepbench needs a GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda:0")

    def run_arms(arms, reps, warmup=a.warmup):
        """{name: [ms per call]}: warm-up calls first, then ``reps`` rounds over the arms in turn."""
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
        if a.arm == "m":
            data, split_edge = loaddataset_like(a.config, False, scale=a.scale)
            adj = data.adj_t.to_device(dev)
            n = adj.size(0)
            test = split_edge["test"]["edge"].to(dev)
            src = torch.tensor(list(dict.fromkeys(test[:, 0].tolist()))[:a.sources], dtype=torch.int64, device=dev)
            truth = SparseTensor.from_edge_index(test.t().contiguous(), sparse_sizes=(n, n)).to_symmetric()
            res = K.rank_path_index(adj, src, truth, "ra", 2)
            met = K.ranking_metrics(res, ks=(20,))
            cand = int((res.rank > 0).sum())
            out.update(nodes=n, nnz=adj.nnz(), test_edges=int(test.shape[0]), sources=int(src.numel()), pairs=met["n_pairs"],
                       candidates=int(res.n_cand.sum()), coverage=round(met["coverage"], 6), short_lists={})
            for m in BOTH + LONG:
                kept = int(((res.rank >= 1) & (res.rank <= m)).sum())
                out["short_lists"][str(m)] = dict(retention=round(kept / max(cand, 1), 6),
                                                  handed_to_the_model=round(kept / max(met["n_pairs"], 1), 6))
            print("KEEPBENCH " + json.dumps(out), flush=True)
            return
        ei, n, _ = dataset_like(a.config, seed=0, scale=a.scale)
        adj = SparseTensor.from_edge_index(ei.to(dev), sparse_sizes=(n, n), trust_data=True).to_symmetric()
        del ei
        src = torch.randint(0, n, (a.sources,), generator=torch.Generator().manual_seed(7)).to(dev)
        out.update(nodes=n, nnz=adj.nnz(), max_deg=adj.max_rowcount())
        if a.arm == "k":
            ptr, edges, val = R.two_hop_scored_candidates(adj, src, "ra")
            size = ptr[1:] - ptr[:-1]
            out.update(candidates=int(ptr[-1]), longest=int(size.max()), mean=round(int(ptr[-1]) / a.sources, 1),
                       lists_longer_than={str(m): int((size > m).sum()) for m in BOTH + LONG}, equal={}, kept={})
            arms = {}
            for m in BOTH:
                old, new = R._keep_m_best(ptr, edges, val, m), R._keep_m_long(ptr, edges, val, m)
                out["equal"][str(m)] = bool(torch.equal(old[0], new[0]) and torch.equal(old[1], new[1]))
                assert out["equal"][str(m)], f"m = {m}: the two routes keep different lists"
                out["kept"][str(m)] = int(new[0][-1])
                arms[f"keep_m_best_{m}"] = lambda m=m: R._keep_m_best(ptr, edges, val, m)
                arms[f"segment_keep_best_{m}"] = lambda m=m: R._keep_m_long(ptr, edges, val, m)
            for m in LONG:
                out["kept"][str(m)] = int(R._keep_m_long(ptr, edges, val, m)[0][-1])
                arms[f"segment_keep_best_{m}"] = lambda m=m: R._keep_m_long(ptr, edges, val, m)
            out["ms"] = run_arms(arms, a.reps)
            # the kernel without the host's part (the offsets' scan and its one sync, the gather of the pairs)
            lib_arms = {}
            for m in BOTH + LONG:
                ptr_m, keep = ops.segment_keep_best(val, ptr, m)
                lib_arms[f"kernel_{m}"] = lambda m=m, ptr_m=ptr_m, keep=keep: ops.check(
                    ops._lib.lib().ocn_segment_keep_best(ops.ptr(val), ops.ptr(ptr), a.sources, m, ops.ptr(ptr_m), ops.ptr(keep),
                                                         ops.ptr(None), ops.stream_ptr()), "ocn_segment_keep_best")
            lib_arms["segment_topk_128"] = lambda: ops.segment_topk(val, ptr, 128)
            out["kernel_ms"] = run_arms(lib_arms, a.reps)
        else:
            sp = adj.to_torch_sparse_coo_tensor()
            adj2 = SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False)
            adj2._col
            del sp
            torch.manual_seed(0)
            H = a.hiddim
            h = torch.randn(n, H, device=dev)
            pred = predictor_dict[a.predictor](H, H, 1, 3, 0.0, 0.0, True).to(dev).eval()
            args = SimpleNamespace(sum=1.0)
            arms = {"unfiltered": lambda: R.recommend_links(pred, h, adj, adj2, src, a.k, a.batch, args)}
            for m in BOTH:
                arms[f"tuple_ra_{m}"] = lambda m=m: R.recommend_links(pred, h, adj, adj2, src, a.k, a.batch, args, prefilter=("ra", m))
            for m in BOTH + LONG:
                arms[f"path_sums_ra_{m}"] = lambda m=m: R.recommend_links(pred, h, adj, adj2, src, a.k, a.batch, args,
                                                                         prefilter=R.PathSums("ra", m))
            out["equal"] = {}
            for m in BOTH:
                x, y = arms[f"tuple_ra_{m}"](), arms[f"path_sums_ra_{m}"]()
                out["equal"][str(m)] = bool(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]))
                assert out["equal"][str(m)], f"m = {m}: the tuple stage and PathSums return different rows"
            full = arms["unfiltered"]()[0]
            out["kept_of_unfiltered_top_k"] = {}
            for m in BOTH + LONG:
                got = arms[f"path_sums_ra_{m}"]()[0]
                hit = ((got[:, :, None] == full[:, None, :]) & (full[:, None, :] >= 0)).any(1).sum().item()
                out["kept_of_unfiltered_top_k"][str(m)] = round(hit / max(int((full >= 0).sum()), 1), 4)
            out["ms"] = run_arms(arms, a.request_reps)
    print("KEEPBENCH " + json.dumps(out), flush=True)


def summary(samples):
    return dict(median=round(statistics.median(samples), 4), min=round(min(samples), 4), max=round(max(samples), 4), n=len(samples))


def summarise(r):
    if isinstance(r, dict):
        return {k: ({name: summary(ts) for name, ts in v.items()} if k in ("ms", "kernel_ms") else summarise(v)) for k, v in r.items()}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default=None, choices=ARMS, help="(internal) run one arm")
    ap.add_argument("--arms", default="krm", help="the arms to run, in this order")
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sources", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--request-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--predictor", default="cn5")
    ap.add_argument("--hiddim", type=int, default=256)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds one arm may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        return child(a)
    passed = [f"--{k.replace('_', '-')}={v}" for k, v in vars(a).items() if k not in ("arm", "arms", "out", "limit")]
    out = {"tool": "keepbench", "config": a.config, "scale": a.scale, "sources": a.sources, "k": a.k, "predictor": a.predictor,
           "H": a.hiddim, "batch": a.batch, "graph": "synthetic (ocn_amd.synth)", "arms": {}}
    rc = 0
    for arm in a.arms:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm] + passed, capture_output=True, text=True,
                               timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"arm {arm}: over its {a.limit} s limit; stopping", flush=True)
            rc = 2
            break
        line = [l for l in p.stdout.splitlines() if l.startswith("KEEPBENCH ")]
        if p.returncode != 0 or not line:
            print(f"arm {arm}: exit {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            rc = 2
            break
        out["arms"][arm] = summarise(json.loads(line[0][len("KEEPBENCH "):]))
        print(f"arm {arm}: done", flush=True)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out and rc == 0:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
