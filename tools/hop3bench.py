"""Link recommendation over three hops at a named shape (collab by default), Q random sources as in tools/prefilterbench.py:
what the 3-hop retrieval costs beside the 2-hop one and beside torch's sparse products, and what a whole request costs.
Device events around every call, warm-up, medians and ranges.  One GPU process at a time: every arm runs in a child of its own
under its own time limit, and the first arm that fails or runs over ends the tool.

    a   the existing 2-hop retrieval, as context: ``prefilter_candidates(adj, src, "ra", 128)``;
    b   the 3-hop retrieval: ``prefilter_candidates(adj, src, kind, 128, hops=3, decay=D)`` for "ra" and for "cn" — the count pass,
        both expansions and the top-M, chunked by ``ops.prefilter_budget`` — and its parts: the first expansion with the count
        pass (``_ThreeHop``), and the second expansion alone on the first chunk;
    c   the yardstick for b: the rows A² + D·A³ of the same sources by ``torch.sparse.mm`` chained on the device, ``--mm-chunk``
        sources at a time (unit weights: the values of the first chunk are compared exactly with ``path_scored_candidates``);
    d   a whole k = 20 request of a cn5 model at H = 256: ``hops=3`` with ``("ra", 128, D)`` against ``hops=2`` with
        ``("ra", 128)``, and for ``--unfiltered-sources`` sources only against the unfiltered ``hops=3`` call.

    python tools/hop3bench.py --out profiles/hop3bench_collab.json

Prints (and with ``--out`` writes) one JSON line.  No figure is a pass condition.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("a", "b", "c", "d")


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    from ocn_amd import ops, recommend as R
    from ocn_amd.model import predictor_dict
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.synth import dataset_like
    if not torch.cuda.is_available():
        raise SystemExit("hop3bench needs a GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda:0")
    ei, n, _ = dataset_like(a.config, seed=0, scale=a.scale)
    adj = SparseTensor.from_edge_index(ei.to(dev), sparse_sizes=(n, n), trust_data=True).to_symmetric()
    del ei
    src = torch.randint(0, n, (a.sources,), generator=torch.Generator().manual_seed(7)).to(dev)
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

    out = {"arm": a.arm, "nodes": n, "nnz": adj.nnz(), "max_deg": adj.max_rowcount()}
    with torch.no_grad():
        if a.arm == "a":
            ptr, _ = R.prefilter_candidates(adj, src, "ra", a.m)
            p2, _ = R.two_hop_candidates(adj, None, src)
            out.update(candidates_2hop=int(p2[-1]), retained=int(ptr[-1]))
            out["ms"] = run_arms({"retrieve_2hop_ra": lambda: R.prefilter_candidates(adj, src, "ra", a.m)}, a.reps)
        elif a.arm == "b":
            plan = R._ThreeHop(adj, src, "ra", D, adj)
            sizes = plan.count.long()
            chunks = list(R._budget_chunks(plan.count, ops.prefilter_budget))
            out.update(frontier_entries=int(plan.ptr2[-1]), longest_frontier=int((plan.ptr2[1:] - plan.ptr2[:-1]).max()),
                       candidates_3hop=int(sizes.sum()), longest=int(sizes.max()), mean=round(float(sizes.sum()) / a.sources, 1),
                       chunks=len(chunks), window_cols=ops.frontier_window_cols(), windows=-(-n // ops.frontier_window_cols()))
            a0, b0, t0 = chunks[0]
            arms = {f"retrieve_3hop_{kind}": (lambda kind=kind: R.prefilter_candidates(adj, src, kind, a.m, hops=3, decay=D))
                    for kind in ("ra", "cn")}
            arms["first_expansion_and_count"] = lambda: R._ThreeHop(adj, src, "ra", D, adj)
            arms["second_expansion_first_chunk"] = lambda: plan.fill(a0, b0, t0)
            out["first_chunk"] = dict(sources=b0 - a0, candidates=t0)
            out["ms"] = run_arms(arms, a.reps)
        elif a.arm == "c":
            A = adj.to_torch_sparse_coo_tensor().to_torch().coalesce()    # torch's own sparse tensor: its products, not the project's
            c = a.mm_chunk

            def rows_of(s):
                q = s.numel()
                E = torch.sparse_coo_tensor(torch.stack([torch.arange(q, device=dev), s]), torch.ones(q, device=dev), (q, n)).coalesce()
                X2 = torch.sparse.mm(torch.sparse.mm(E, A), A)
                return (X2 + D * torch.sparse.mm(X2, A)).coalesce()

            def all_rows():
                for i in range(0, a.sources, c):
                    rows_of(src[i:i + c])
            # unit weights: the values of the first chunk against the project's, exactly
            first = torch.unique(src[:c])                                 # (distinct: a repeated source would be summed by the selection)
            X = rows_of(first)
            r, t = X.indices()
            s_of = first[r]
            known = torch.zeros(first.numel(), n, dtype=torch.bool, device=dev)
            kr = adj._rowptr
            for i, s in enumerate(first.tolist()):
                known[i, adj._col[kr[s]:kr[s + 1]].long()] = True
                known[i, s] = True
            keep = ~known[r, t]
            ptr, edges, val = R.path_scored_candidates(adj, first, "cn", 3, D)
            out["values_equal"] = bool(torch.equal(edges, torch.stack([s_of[keep], t[keep]], 1)) and torch.equal(val, X.values()[keep]))
            out["compared_pairs"] = int(edges.shape[0])
            del X, known
            out["ms"] = run_arms({f"torch_sparse_mm_chunks_of_{c}": all_rows}, a.reps)
        else:
            sp = adj.to_torch_sparse_coo_tensor()
            adj2 = SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False)
            adj2._col
            del sp
            torch.manual_seed(0)
            H = a.hiddim
            h = torch.randn(n, H, device=dev)
            pred = predictor_dict["cn5"](H, H, 1, 3, 0.0, 0.0, True).to(dev).eval()
            args = SimpleNamespace(sum=1.0)
            few = src[:a.unfiltered_sources].contiguous()
            arms = {"hops2_ra_128": lambda: R.recommend_links(pred, h, adj, adj2, src, a.k, a.batch, args, prefilter=("ra", a.m)),
                    "hops3_ra_128": lambda: R.recommend_links(pred, h, adj, adj2, src, a.k, a.batch, args, prefilter=("ra", a.m, D), hops=3)}
            out["ms"] = run_arms(arms, a.request_reps, 1)
            few_arms = {"hops3_ra_128": lambda: R.recommend_links(pred, h, adj, adj2, few, a.k, a.batch, args, prefilter=("ra", a.m, D), hops=3),
                        "hops3_unfiltered": lambda: R.recommend_links(pred, h, adj, adj2, few, a.k, a.batch, args, hops=3)}
            out["few_sources"] = int(few.numel())
            out["few_candidates_3hop"] = int(R.three_hop_candidates(adj, few)[0][-1])
            out["few_ms"] = run_arms(few_arms, a.request_reps, 1)
    print("HOP3BENCH " + json.dumps(out), flush=True)


def summary(samples):
    return dict(median=round(statistics.median(samples), 4), min=round(min(samples), 4), max=round(max(samples), 4), n=len(samples))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default=None, choices=ARMS, help="(internal) run one arm")
    ap.add_argument("--arms", default="abcd", help="the arms to run, in this order")
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sources", type=int, default=4096)
    ap.add_argument("--unfiltered-sources", type=int, default=256)
    ap.add_argument("--decay", type=float, default=0.5)
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--hiddim", type=int, default=256)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--mm-chunk", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--request-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=240, help="seconds one arm may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        return child(a)
    passed = [f"--{k.replace('_', '-')}={v}" for k, v in vars(a).items() if k not in ("arm", "arms", "out", "limit")]
    out = {"tool": "hop3bench", "config": a.config, "scale": a.scale, "sources": a.sources, "decay": a.decay, "m": a.m, "k": a.k,
           "H": a.hiddim, "batch": a.batch, "arms": {}}
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
        line = [l for l in p.stdout.splitlines() if l.startswith("HOP3BENCH ")]
        if p.returncode != 0 or not line:
            print(f"arm {arm}: exit {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            out["arms"][arm] = f"exit {p.returncode}"
            rc = 2
            break
        r = json.loads(line[0][len("HOP3BENCH "):])
        for key in ("ms", "few_ms"):
            if key in r:
                r[key] = {name: summary(ts) for name, ts in r[key].items()}
        for key in ("nodes", "nnz", "max_deg"):
            out[key] = r.pop(key)
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
