"""Random-walk retrieval beside the exact path-sum retrieval at a named shape (collab by default), Q random sources as in
tools/hop3bench.py: what a walk short list costs, how much of the exact "ra" short list it holds, and what it keeps of held-out
links.  Device events around every call, every shape warmed, the alternatives interleaved inside every repeat, medians and
ranges.  One GPU process at a time: every arm runs in a child of its own under its own time limit, and the first arm that fails
or runs over ends the tool.  The graph is a synthetic Chung-Lu graph of the named shape, not the dataset.

    t   time: ``random_walk_short_list`` for (W, L) in {(256, 2), (1024, 2), (1024, 3), (max, 3)} (and the two kernel passes
        alone, ``random_walk_candidates``) against the yardsticks ``prefilter_candidates(adj, src, "ra", m)`` and
        ``prefilter_candidates(adj, src, "ra", m, hops=3, decay=D)``, all in one interleaved run; and per (W, L) the share of
        the exact short list of the same hops and decay that the walk short list contains (overlap@m per source: mean and
        10th percentile over the sources whose exact list is not empty) and the mean number of visited candidates;
    q   keep: the training graph and held-out test edges of ``synth.loaddataset_like``, the first Q distinct test sources;
        ``rank_links`` of an untrained cn5 model on the walk route with every short list of arm t — coverage (exact stages: a
        candidate within the hops; walks: visited at all) and retention (kept by the short list) do not depend on the model.

    python tools/rwbench.py --out profiles/rwbench_collab.json
    python tools/rwbench.py --config citation2 --arms t --sources 1024 --skip-exact3 --out profiles/rwbench_citation2.json

Prints (and with ``--out`` writes) one JSON line.  No figure is a pass condition.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("t", "q")


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    from ocn_amd import ops, ranking as K, recommend as R
    from ocn_amd.model import predictor_dict
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.synth import dataset_like, loaddataset_like
    if not torch.cuda.is_available():
        raise SystemExit("rwbench needs a GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda:0")
    D, m = a.decay, a.m
    shapes = [(256, 2), (1024, 2), (1024, 3), (ops.rw_max_walks(), 3)]

    def stage(W, L):
        return R.RandomWalks(m, W, L, D if L == 3 else None, a.seed)

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

    out = {"arm": a.arm, "max_walks": ops.rw_max_walks()}
    with torch.no_grad():
        if a.arm == "t":
            ei, n, _ = dataset_like(a.config, seed=0, scale=a.scale)
            adj = SparseTensor.from_edge_index(ei.to(dev), sparse_sizes=(n, n), trust_data=True).to_symmetric()
            del ei
            src = torch.randint(0, n, (a.sources,), generator=torch.Generator().manual_seed(7)).to(dev)
            Q = src.numel()
            out.update(nodes=n, nnz=adj.nnz(), max_deg=adj.max_rowcount())
            arms = {"exact_ra_hops2": lambda: R.prefilter_candidates(adj, src, "ra", m)}
            if not a.skip_exact3:
                arms["exact_ra_hops3"] = lambda: R.prefilter_candidates(adj, src, "ra", m, hops=3, decay=D)
            for W, L in shapes:
                arms[f"rw_short_list_W{W}_L{L}"] = lambda W=W, L=L: R.random_walk_short_list(adj, src, stage(W, L))
                arms[f"rw_visits_W{W}_L{L}"] = lambda W=W, L=L: R.random_walk_candidates(adj, src, W, L, D if L == 3 else None,
                                                                                         seed=a.seed)

            def keys(ptr, edges):
                q = torch.repeat_interleave(torch.arange(Q, device=dev), ptr[1:] - ptr[:-1], output_size=edges.shape[0])
                return q, q * n + edges[:, 1]

            exact = {2: R.prefilter_candidates(adj, src, "ra", m)}
            if not a.skip_exact3:
                exact[3] = R.prefilter_candidates(adj, src, "ra", m, hops=3, decay=D)
            out["exact"] = {str(h): dict(retained=int(p[-1])) for h, (p, _) in exact.items()}
            out["overlap"] = {}
            for W, L in shapes:
                vptr = R.random_walk_candidates(adj, src, W, L, D if L == 3 else None, seed=a.seed)[0]
                row = dict(visited_mean=round(float(vptr[-1]) / Q, 1), visited_max=int((vptr[1:] - vptr[:-1]).max()))
                if L in exact:
                    eptr, eedges = exact[L]
                    wptr, wedges = R.random_walk_short_list(adj, src, stage(W, L))
                    eq, ek = keys(eptr, eedges)
                    hit = torch.isin(ek, keys(wptr, wedges)[1])
                    per = torch.zeros(Q, dtype=torch.float64, device=dev).index_add_(0, eq, hit.double())
                    size = (eptr[1:] - eptr[:-1]).double()
                    share = (per / size.clamp(min=1))[size > 0]
                    row.update(sources_with_exact_list=int(share.numel()), overlap_mean=round(float(share.mean()), 4),
                               overlap_p10=round(float(torch.quantile(share, 0.1)), 4), retained=int(wptr[-1]))
                out["overlap"][f"W{W}_L{L}"] = row
            out["ms"] = run_arms(arms, a.reps)
        else:
            data, split_edge = loaddataset_like(a.config, False, scale=a.scale)
            adj = data.adj_t.to_device(dev)
            n = adj.size(0)
            test = split_edge["test"]["edge"].to(dev)
            src = torch.tensor(list(dict.fromkeys(test[:, 0].tolist()))[:a.sources], dtype=torch.int64, device=dev)
            truth = SparseTensor.from_edge_index(test.t().contiguous(), sparse_sizes=(n, n)).to_symmetric()
            out.update(nodes=n, nnz=adj.nnz(), max_deg=adj.max_rowcount(), test_edges=int(test.shape[0]), sources=int(src.numel()))
            torch.manual_seed(0)
            H = a.hiddim
            h = torch.randn(n, H, device=dev)
            pred = predictor_dict["cn5"](H, H, 1, 3, 0.0, 0.0, True).to(dev).eval()
            args = SimpleNamespace(sum=1.0)
            stages = {"exact_ra_hops2": (("ra", m), 2)}
            if not a.skip_exact3:
                stages["exact_ra_hops3"] = (("ra", m, D), 3)
            for W, L in shapes:
                stages[f"rw_W{W}_L{L}"] = (stage(W, L), L)
            out["keep"] = {}
            for name, (pf, hops) in stages.items():
                met = K.ranking_metrics(K.rank_links(pred, h, adj, None, src, truth, a.batch, args, prefilter=pf, hops=hops), ks=(10,))
                out["keep"][name] = dict(pairs=met["n_pairs"], coverage=round(met["coverage"], 6), retention=round(met["retention"], 6),
                                         kept=round(met["coverage"] * met["retention"], 6))
    print("RWBENCH " + json.dumps(out), flush=True)


def summary(samples):
    return dict(median=round(statistics.median(samples), 4), min=round(min(samples), 4), max=round(max(samples), 4), n=len(samples))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default=None, choices=ARMS, help="(internal) run one arm")
    ap.add_argument("--arms", default="tq", help="the arms to run, in this order")
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sources", type=int, default=4096)
    ap.add_argument("--decay", type=float, default=0.5)
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--hiddim", type=int, default=64)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--skip-exact3", action="store_true", help="leave the exact 3-hop stage out (a shape where it does not fit)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds one arm may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        return child(a)
    passed = [f"--{k.replace('_', '-')}={v}" for k, v in vars(a).items() if k not in ("arm", "arms", "out", "limit", "skip_exact3")]
    if a.skip_exact3:
        passed.append("--skip-exact3")
    out = {"tool": "rwbench", "graph": f"synthetic Chung-Lu graph of the {a.config} shape", "config": a.config, "scale": a.scale,
           "sources": a.sources, "decay": a.decay, "m": a.m, "seed": a.seed, "arms": {}}
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
        line = [l for l in p.stdout.splitlines() if l.startswith("RWBENCH ")]
        if p.returncode != 0 or not line:
            print(f"arm {arm}: exit {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            out["arms"][arm] = f"exit {p.returncode}"
            rc = 2
            break
        r = json.loads(line[0][len("RWBENCH "):])
        if "ms" in r:
            r["ms"] = {name: summary(ts) for name, ts in r["ms"].items()}
        for key in ("nodes", "nnz", "max_deg", "max_walks"):
            if key in r and arm == a.arms[0]:
                out[key] = r[key]
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
