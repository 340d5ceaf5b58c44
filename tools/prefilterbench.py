"""Two-stage link recommendation at a named shape (collab by default), Q random sources as in tools/recbench.py: what the
retrieval half costs, and what a whole request costs with and without it.  Device events around every call, warm-up, medians
and ranges; the arms of a process are interleaved call by call, the processes alternated round by round.

    Arm 1, retrieval: ``ops.two_hop_sums_fill`` (the candidates with their ra score from one expansion; window_cols = the
        default, 1/2 and 1/4 of it) against ``ops.two_hop_diff_fill`` + ``heuristics.score_edges_heuristic`` over the same
        candidates (an intersection per candidate).  The outputs are compared with ``torch.equal`` in the same run.  The new
        pass is also timed on subsets of the sources: the heaviest alone, those of degree <= 16, the lightest alone.
    Arm 2, the request: ``recommend_links(..., prefilter=("ra", 128))`` and ``("ra", 32)`` against the unfiltered call, k = 20,
        cn5 at H = 256, batch-coupled and with frozen column weights; ``--walk`` scores on the walk route (``adj2=None``: the
        ppa / citation2 way) instead of through A².

    python tools/prefilterbench.py --baseline-lib PATH --out profiles/prefilterbench_collab.json
    python tools/prefilterbench.py --config citation2 --walk --predictor cn7 --hiddim 32 --batch 2048 --reps 3

``--baseline-lib``: a libocn_hip.so built from the parent commit; the two baselines (the intersection route of arm 1, the
unfiltered request of arm 2) then also run on it, in a process of their own (``base_lib``), beside the same calls on the
in-tree library.  Prints (and with ``--out`` writes) one JSON line.  No figure is a pass condition.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("ocn_two_hop_sums_window_cols", "ocn_two_hop_sums_fill")


def child(a):
    sys.path.insert(0, ROOT)
    from ocn_amd import _lib
    base = a.arm == "base"
    if base:
        for name in NEW_ENTRIES:                                  # (the parent's library does not export them; no baseline calls them)
            _lib.SIGNATURES.pop(name, None)
    import torch
    from ocn_amd import ops, recommend as R
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.heuristics import score_edges_heuristic
    from ocn_amd.model import predictor_dict
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.synth import dataset_like
    if not torch.cuda.is_available():
        raise SystemExit("prefilterbench needs a GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda:0")
    ei, n, _ = dataset_like(a.config, seed=0, scale=a.scale)
    adj = SparseTensor.from_edge_index(ei.to(dev), sparse_sizes=(n, n), trust_data=True).to_symmetric()
    del ei
    src = torch.randint(0, n, (a.sources,), generator=torch.Generator().manual_seed(7)).to(dev)
    adj2 = None
    if not a.walk:
        sp = adj.to_torch_sparse_coo_tensor()
        adj2 = SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False)
        adj2._col
        del sp

    def run_arms(arms, reps):
        """{name: [ms per call]}: warm-up calls first, then ``reps`` rounds over the arms in turn."""
        for fn in arms.values():
            for _ in range(a.warmup):
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

    out = {"arm": a.arm, "lib": os.environ.get("OCN_LIB_PATH", "in-tree"), "nodes": n, "nnz": adj.nnz(), "max_deg": adj.max_rowcount()}
    rpa, cola = adj._rowptr, adj._col
    with torch.no_grad(), ops.prevalidated(src, src, n, n):
        off = ops.scan_i32(ops.two_hop_diff_count(rpa, cola, rpa, cola, src))
        total = int(off[-1].item())
        sizes = off[1:] - off[:-1]
        out.update(candidates=total, longest=int(sizes.max()), mean=round(total / a.sources, 1))
        # ---- arm 1 ----
        hb = a.heur_batch

        def intersect():
            edges = ops.two_hop_diff_fill(rpa, cola, rpa, cola, src, off, total=total)
            return edges, score_edges_heuristic(adj, None, edges, hb, "ra")
        arms = {"diff_fill+score_edges_heuristic": intersect}
        if not base:
            from ocn_amd.heuristics import node_table
            W = ops.two_hop_sums_window_cols()
            w = node_table(adj)
            out.update(sums_window_cols=W, sums_windows=-(-n // W), diff_windows=-(-n // ops.two_hop_window_cols()))
            for name, wc in (("sums_fill", 0), ("sums_fill_half_window", W // 2 // 64 * 64), ("sums_fill_quarter_window", W // 4 // 64 * 64)):
                arms[name] = lambda wc=wc: ops.two_hop_sums_fill(rpa, cola, rpa, cola, src, off, w, 1, total=total, window_cols=wc)
            want_e, want_v = intersect()
            out["retrieval_equal"] = {name: bool(torch.equal(e, want_e) and torch.equal(v, want_v))
                                      for name, (e, v) in ((nm, arms[nm]()) for nm in list(arms)[1:])}
            arms["count"] = lambda: ops.two_hop_diff_count(rpa, cola, rpa, cola, src)
            del want_e, want_v
        out["retrieval_ms"] = run_arms(arms, a.reps)
        if not base:
            # where the retrieval pass spends its time: the heaviest source alone (the tail one workgroup cannot shorten) and the
            # light sources alone (the per-window fixed work), beside an all-but-empty launch
            deg = (rpa[1:] - rpa[:-1])[src]
            picks = {"heaviest_source": deg.argsort(descending=True)[:1], "degree_le_16": (deg <= 16).nonzero().flatten(),
                     "lightest_source": deg.argsort()[:1]}
            sub, out["retrieval_subsets"] = {}, {}
            for name, sel in picks.items():
                s = src[sel].contiguous()
                off_s = ops.scan_i32(ops.two_hop_diff_count(rpa, cola, rpa, cola, s))
                tot = int(off_s[-1].item())
                out["retrieval_subsets"][name] = dict(sources=int(s.numel()), candidates=tot, max_degree=int(deg[sel].max()))
                sub[name] = lambda s=s, off_s=off_s, tot=tot: ops.two_hop_sums_fill(rpa, cola, rpa, cola, s, off_s, w, 1, total=tot)
            out["retrieval_subsets_ms"] = run_arms(sub, a.reps)
        # ---- arm 2 ----
        torch.manual_seed(0)
        H = a.hiddim
        h = torch.randn(n, H, device=dev)
        pred = predictor_dict[a.predictor](H, H, 1, 3, 0.0, 0.0, True).to(dev).eval()
        args = SimpleNamespace(sum=1.0)
        filters = [None] if base else [None, ("ra", 128), ("ra", 32)]
        names = {None: "unfiltered", ("ra", 128): "ra_128", ("ra", 32): "ra_32"}

        def request(f):
            if f is None:
                return R.recommend_links(pred, h, adj, adj2, src, a.k, a.batch, args)
            return R.recommend_links(pred, h, adj, adj2, src, a.k, a.batch, args, prefilter=f)
        out["request_ms"], out["kept_of_unfiltered_top_k"] = {}, {}
        for mode in (("coupled", "frozen") if a.predictor in ("cn5", "cn7") else ("coupled",)):
            if mode == "frozen":
                ptr, edges = R.two_hop_candidates(adj, adj2, src)
                pick = torch.randperm(edges.shape[0], generator=torch.Generator().manual_seed(3))[:min(a.batch, ops.MAX_BATCH)].to(dev)
                pred.set_frozen_columns(freeze_columns(pred, adj, adj2, edges[pick].contiguous(), args), args)
                del ptr, edges, pick
            out["request_ms"][mode] = run_arms({names[f]: (lambda f=f: request(f)) for f in filters}, a.request_reps)
            if not base:
                full = request(None)[0]
                for f in filters[1:]:
                    got = request(f)[0]
                    hit = ((got[:, :, None] == full[:, None, :]) & (full[:, None, :] >= 0)).any(1).sum().item()
                    out["kept_of_unfiltered_top_k"][f"{mode}_{names[f]}"] = round(hit / max(int((full >= 0).sum()), 1), 4)
    print("PREFILTERBENCH " + json.dumps(out), flush=True)


def summary(samples):
    return dict(median=round(statistics.median(samples), 4), min=round(min(samples), 4), max=round(max(samples), 4), n=len(samples))


def merge(runs, key):
    """{arm: summary} (or {mode: {arm: summary}}) over the per-call samples of all rounds."""
    first = runs[0][key]
    if all(isinstance(v, list) for v in first.values()):
        return {name: summary([t for r in runs for t in r[key][name]]) for name in first}
    return {mode: {name: summary([t for r in runs for t in r[key][mode][name]]) for name in first[mode]} for mode in first}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default=None, choices=["new", "base"], help="(internal) run one process's arms")
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sources", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--request-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--predictor", default="cn5")
    ap.add_argument("--hiddim", type=int, default=256)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--heur-batch", type=int, default=65536)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--walk", action="store_true", help="score on the walk route (adj2=None) instead of through A²")
    ap.add_argument("--baseline-lib", default=None, help="libocn_hip.so built from the parent commit, for the baselines")
    ap.add_argument("--limit", type=int, default=400, help="seconds one child may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        return child(a)
    passed = [f"--{k.replace('_', '-')}" + (f"={v}" if not isinstance(v, bool) else "") for k, v in vars(a).items()
              if k not in ("arm", "baseline_lib", "out", "limit", "rounds") and v not in (None, False)]
    runs = {"new": [], "base": []}
    for rnd in range(a.rounds):
        for arm in ("base", "new") if a.baseline_lib else ("new",):
            env = dict(os.environ)
            env.pop("OCN_LIB_PATH", None)
            if arm == "base":
                env["OCN_LIB_PATH"] = os.path.abspath(a.baseline_lib)
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm] + passed, env=env, capture_output=True,
                                   text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(f"arm {arm} round {rnd}: over its {a.limit} s limit; stopping", flush=True)
                return 2
            line = [l for l in p.stdout.splitlines() if l.startswith("PREFILTERBENCH ")]
            if p.returncode != 0 or not line:
                print(f"arm {arm} round {rnd}: exit {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
                return 2
            runs[arm].append(json.loads(line[0][len("PREFILTERBENCH "):]))
            print(f"round {rnd} {arm}: done", flush=True)
    new = runs["new"]
    out = {"tool": "prefilterbench", "config": a.config, "scale": a.scale, "sources": a.sources, "k": a.k, "predictor": a.predictor,
           "H": a.hiddim, "batch": a.batch, "route": "walk" if a.walk else "adj2", "rounds": a.rounds,
           **{key: new[0][key] for key in ("nodes", "nnz", "max_deg", "candidates", "longest", "mean", "sums_window_cols", "sums_windows",
                                           "diff_windows")},
           "retrieval_equal": {name: all(r["retrieval_equal"][name] for r in new) for name in new[0]["retrieval_equal"]},
           "retrieval_ms": merge(new, "retrieval_ms"), "retrieval_subsets": new[0]["retrieval_subsets"],
           "retrieval_subsets_ms": merge(new, "retrieval_subsets_ms"), "request_ms": merge(new, "request_ms"),
           "kept_of_unfiltered_top_k": new[-1]["kept_of_unfiltered_top_k"]}
    if runs["base"]:
        out["base_lib"] = {"retrieval_ms": merge(runs["base"], "retrieval_ms"), "request_ms": merge(runs["base"], "request_ms")}
    else:
        out["base_lib"] = "not taken"
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
