"""Embedding retrieval at a named shape (collab by default): what the exact int8 short list costs beside the same short list
from chunked fp32 torch, and what the stage keeps of held-out links beside the graph-local "ra" stage.  Device events around
every call, every arm warmed, the alternatives interleaved inside every repeat, medians and ranges.  One GPU process at a time:
every arm runs in a child of its own under its own time limit, and the first arm that fails or runs over ends the tool.  The
graph is a synthetic Chung-Lu graph of the named shape, not the dataset; the embeddings are random features smoothed by two
rounds of mean aggregation over it (an encoder without weights), not a trained model's.

    t   time, Q random sources, width H, exclusion by ``adj``, the index built once outside the timing:
        ``int8_stage``   ``embedding_candidates``: the queries' quantisation, ``ops.mips_topm_i8``, the ragged layout;
        ``int8_kernel``  ``ops.mips_topm_i8`` alone on queries quantised beforehand;
        ``torch_fp32``   the same short list from torch on the same device: per chunk of ``--chunk`` queries an fp32 ``matmul``
                         against all keys, the excluded entries set to -inf, ``topk``; then the same ragged layout.
        Also the baseline's peak extra memory, the share of the int8 lists' entries the fp32 lists hold (quantisation moves
        near-ties), and the kernel's share of the int8 MFMA peak (2 x the ~2.5 PF dense BF16 figure: ~5.0e15 op/s).
    q   keep: the training graph and held-out test edges of ``synth.loaddataset_like``, the first ``--eval-sources`` distinct test
        sources; ``rank_links`` of an untrained cn5 model on the walk route with ("ra", m), ``EmbeddingNeighbours(m)`` without
        and with ``normalize``, and their union: coverage, retention, recall@20 after the model.
    s   sweep, the kernel alone at the shape of arm t: ``ops.mips_topm_i8`` for m in {128, 64, 16} at n_split in {1, 2, 4, 8, 16,
        32, 64} with the exclusion by ``adj`` (``m<M>_ns<S>_excl``), and at the automatic split (``ns0``) with the exclusion,
        with the sources alone (``rows_only``: only the source itself is dropped) and without sources (``plain``).  Not among
        the default ``--arms``.

    python tools/mipsbench.py --out profiles/mipsbench_collab.json
    python tools/mipsbench.py --arms s --out profiles/mipsbench_collab_split_sweep.json

Prints (and with ``--out`` writes) one JSON line.  No figure is a pass condition.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("t", "q", "s")
INT8_PEAK = 5.0e15               # op/s: the int8 MFMA forms run at twice the BF16 rate, ~2.5 PF dense


def smoothed_features(adj, n, H, dev, rounds=2):
    """Random features after ``rounds`` of mean aggregation with a self term: neighbours end up near each other."""
    import torch
    torch.manual_seed(0)
    h = torch.randn(n, H, device=dev)
    row, col = adj.storage.row().long(), adj.storage.col().long()
    deg = (adj._rowptr[1:] - adj._rowptr[:-1]).float().clamp(min=1)[:, None]
    for _ in range(rounds):
        h = 0.5 * h + 0.5 * torch.zeros_like(h).index_add_(0, row, h[col]) / deg
    return h.contiguous()


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    from ocn_amd import ops, ranking as K, recommend as R
    from ocn_amd.model import predictor_dict
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.synth import dataset_like, loaddataset_like
    if not torch.cuda.is_available():
        raise SystemExit("mipsbench needs a GPU: a CPU run says nothing about this kernel")
    dev = torch.device("cuda:0")
    m, H = a.m, a.hiddim

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
        if a.arm in ("t", "s"):
            ei, n, _ = dataset_like(a.config, seed=0, scale=a.scale)
            adj = SparseTensor.from_edge_index(ei.to(dev), sparse_sizes=(n, n), trust_data=True).to_symmetric()
            del ei
            src = torch.randint(0, n, (a.sources,), generator=torch.Generator().manual_seed(7)).to(dev)
            Q = src.numel()
            h = smoothed_features(adj, n, H, dev)
            index = R.EmbeddingIndex(h)
            queries = h[src]
            qq, _ = ops.quantize_rows_i8(queries)
            excl = (adj._rowptr, adj._col)
            out.update(nodes=n, nnz=adj.nnz(), width=H, width_padded=int(index.keys_q.shape[1]), chunk=a.chunk)
        if a.arm == "s":
            arms = {}
            for mm in (128, 64, 16):
                for ns in (1, 2, 4, 8, 16, 32, 64):
                    arms[f"m{mm}_ns{ns}_excl"] = lambda mm=mm, ns=ns: ops.mips_topm_i8(qq, index.keys_q, index.kscale, mm, src, excl, True, ns)
                arms[f"m{mm}_ns0_excl"] = lambda mm=mm: ops.mips_topm_i8(qq, index.keys_q, index.kscale, mm, src, excl, True, 0)
                arms[f"m{mm}_ns0_rows_only"] = lambda mm=mm: ops.mips_topm_i8(qq, index.keys_q, index.kscale, mm, src, None, True, 0)
                arms[f"m{mm}_ns0_plain"] = lambda mm=mm: ops.mips_topm_i8(qq, index.keys_q, index.kscale, mm, None, None, True, 0)
            out["ms"] = run_arms(arms, a.reps)
        elif a.arm == "t":

            def ragged(val, node):
                have = node >= 0
                big = torch.iinfo(torch.int64).max
                ids, at = torch.where(have, node, torch.full_like(node, big)).sort(dim=1)
                keep = ids < big
                return torch.stack([src[:, None].expand(Q, m)[keep], ids[keep]], 1), val.gather(1, at)[keep]

            def torch_fp32():
                vals, nodes = [], []
                rp, col = excl
                for c0 in range(0, Q, a.chunk):
                    s = src[c0:c0 + a.chunk]
                    score = queries[c0:c0 + a.chunk] @ h.t()
                    score[torch.arange(s.numel(), device=dev), s] = float("-inf")
                    start = rp[s]
                    cnt = rp[s + 1] - start
                    seg = torch.repeat_interleave(torch.arange(s.numel(), device=dev), cnt)
                    at = torch.arange(seg.numel(), device=dev) - (torch.cumsum(cnt, 0) - cnt)[seg] + start[seg]
                    score[seg, col[at].long()] = float("-inf")
                    v, i = torch.topk(score, m, dim=1)
                    vals.append(v)
                    nodes.append(torch.where(torch.isinf(v), torch.full_like(i, -1), i))
                return ragged(torch.cat(vals), torch.cat(nodes))

            arms = {"int8_stage": lambda: R.embedding_candidates(index, queries, src, m, adj),
                    "int8_kernel": lambda: ops.mips_topm_i8(qq, index.keys_q, index.kscale, m, src, excl, True),
                    "torch_fp32": torch_fp32}
            _, e8, _ = R.embedding_candidates(index, queries, src, m, adj)
            e32, _ = torch_fp32()
            out["retained"] = dict(int8=int(e8.shape[0]), fp32=int(e32.shape[0]))
            out["int8_entries_in_fp32_lists"] = round(float(torch.isin(e8[:, 0] * n + e8[:, 1], e32[:, 0] * n + e32[:, 1]).float().mean()), 6)
            del e8, e32
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            torch_fp32()
            torch.cuda.synchronize()
            out["torch_fp32_peak_extra_bytes"] = int(torch.cuda.max_memory_allocated() - base)
            torch.cuda.reset_peak_memory_stats()
            R.embedding_candidates(index, queries, src, m, adj)
            torch.cuda.synchronize()
            out["int8_stage_peak_extra_bytes"] = int(torch.cuda.max_memory_allocated() - base)
            out["ops"] = 2.0 * Q * n * int(index.keys_q.shape[1])
            out["ms"] = run_arms(arms, a.reps)
        else:
            data, split_edge = loaddataset_like(a.config, False, scale=a.scale)
            adj = data.adj_t.to_device(dev)
            n = adj.size(0)
            test = split_edge["test"]["edge"].to(dev)
            src = torch.tensor(list(dict.fromkeys(test[:, 0].tolist()))[:a.eval_sources], dtype=torch.int64, device=dev)
            truth = SparseTensor.from_edge_index(test.t().contiguous(), sparse_sizes=(n, n)).to_symmetric()
            out.update(nodes=n, nnz=adj.nnz(), test_edges=int(test.shape[0]), sources=int(src.numel()), width=a.eval_hiddim)
            He = a.eval_hiddim
            h = smoothed_features(adj, n, He, dev)
            torch.manual_seed(0)
            pred = predictor_dict["cn5"](He, He, 1, 3, 0.0, 0.0, True).to(dev).eval()
            args = SimpleNamespace(sum=1.0)
            emb, cos = R.EmbeddingNeighbours(m), R.EmbeddingNeighbours(m, normalize=True)
            stages = {"ra": ("ra", m), "embedding": emb, "embedding_cos": cos, "union_ra_embedding": R.ShortListUnion(("ra", m), emb),
                      "union_ra_embedding_cos": R.ShortListUnion(("ra", m), cos)}
            out["keep"] = {}
            for name, pf in stages.items():
                met = K.ranking_metrics(K.rank_links(pred, h, adj, None, src, truth, a.batch, args, prefilter=pf), ks=(20,))
                row = dict(pairs=met["n_pairs"], coverage=round(met["coverage"], 6), recall_at_20=round(met["recall@20"], 6))
                if "retention" in met:
                    row.update(retention=round(met["retention"], 6), kept=round(met["coverage"] * met["retention"], 6))
                out["keep"][name] = row
    print("MIPSBENCH " + json.dumps(out), flush=True)


def summary(samples):
    return dict(median=round(statistics.median(samples), 4), min=round(min(samples), 4), max=round(max(samples), 4), n=len(samples))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default=None, choices=ARMS, help="(internal) run one arm")
    ap.add_argument("--arms", default="tq", help="the arms to run, in this order")
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sources", type=int, default=4096)
    ap.add_argument("--eval-sources", type=int, default=1024)
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--hiddim", type=int, default=256)
    ap.add_argument("--eval-hiddim", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=1024, help="queries per fp32 matmul of the torch baseline")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds one arm may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        return child(a)
    passed = [f"--{k.replace('_', '-')}={v}" for k, v in vars(a).items() if k not in ("arm", "arms", "out", "limit")]
    out = {"tool": "mipsbench", "graph": f"synthetic Chung-Lu graph of the {a.config} shape",
           "embeddings": "random features after two rounds of mean aggregation (no trained encoder)", "config": a.config,
           "scale": a.scale, "sources": a.sources, "m": a.m, "int8_peak_ops": INT8_PEAK, "arms": {}}
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
        line = [l for l in p.stdout.splitlines() if l.startswith("MIPSBENCH ")]
        if p.returncode != 0 or not line:
            print(f"arm {arm}: exit {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            out["arms"][arm] = f"exit {p.returncode}"
            rc = 2
            break
        r = json.loads(line[0][len("MIPSBENCH "):])
        if "ms" in r:
            r["ms"] = {name: summary(ts) for name, ts in r["ms"].items()}
        if "ms" in r and "torch_fp32" in r["ms"]:
            r["ratio_torch_fp32_over_int8_stage"] = round(r["ms"]["torch_fp32"]["median"] / r["ms"]["int8_stage"]["median"], 3)
            r["int8_kernel_share_of_peak"] = round(r["ops"] / (r["ms"]["int8_kernel"]["median"] * 1e-3) / INT8_PEAK, 4)
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
