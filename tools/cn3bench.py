"""The A³-free cn3 pass of cn6 (``ocn_cn3_flags``) at the collab shape — B = 65 536 candidates of bench.py's synthetic graph —
beside the (A, A, A²) intersection pass (``ocn_cn_flags``) of the same batch, both timed as stages of
``CNState3(adj, adj2, None, e)`` by device events through ``ops.stage_timer``; then the end-to-end rate of
``pipeline.score_edges`` with a cn6 predictor at H = 256.

    python tools/cn3bench.py [--config collab] [--scale 1.0] [--batch 65536] [--reps 20] [--loop-batches 4] [--out FILE]

Prints (and with ``--out`` writes) one JSON line: the median and range of the ``cn_flags`` and ``cn3_flags`` stages in ms, the
batch's probe bound Σ nds(src) (an upper bound: a neighbour's sweep ends at its first hit), the longest work item in elements,
the probe bound over the median time, and candidates/s of the scoring loop.  No figure is a pass condition.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Timer:
    """``ops.stage_timer``: an event per mark on the current stream; a stage lasts from the mark before it to its own."""

    def __init__(self):
        self.events = []

    def mark(self, name, flops=0.0):
        import torch
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.events.append((name, ev))

    def stages(self):
        out = {}
        for (_, p), (name, ev) in zip(self.events, self.events[1:]):
            if name != "begin":
                out.setdefault(name, []).append(p.elapsed_time(ev))
        return out


def _longest_item(adj, nds, src):
    """Elements of the longest work item of the batch: the items of ocn_chunk_offsets (common.h: walk_group)."""
    import torch
    i = torch.unique(src)
    deg = adj._rowptr[1:] - adj._rowptr[:-1]
    d = deg[i]
    chunks = (d + 63) // 64
    per_chunk = nds[i] // chunks.clamp(min=1) + 1
    cg = torch.where(chunks <= 1, torch.ones_like(d), (16384 // per_chunk).clamp(min=1).minimum(chunks.clamp(max=8)))
    sub = adj[i]
    r, c, _ = sub.coo()
    p = torch.arange(r.numel(), device=r.device) - sub._rowptr[:-1][r]
    item = p // (cg[r] * 64)
    key = r * (int(item.max()) + 1 if item.numel() else 1) + item
    tot = torch.zeros(int(key.max()) + 1 if key.numel() else 1, dtype=torch.int64, device=r.device).index_add_(0, key, deg[c])
    return int(tot.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-batches", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    from ocn_amd.pipeline import score_edges
    from ocn_amd.sparse import SparseTensor
    from ocn_amd.synth import dataset_like, sample_edges
    from ocn_amd.utils import CNState3
    if not torch.cuda.is_available():
        raise SystemExit("cn3bench needs a GPU: a CPU run says nothing about this kernel")
    dev = torch.device("cuda:0")
    ei, n, _ = dataset_like(a.config, seed=0, scale=a.scale)
    adj = SparseTensor.from_edge_index(ei.to(dev), sparse_sizes=(n, n), trust_data=True).to_symmetric()
    with torch.no_grad():
        sp = adj.to_torch_sparse_coo_tensor()
        adj2 = SparseTensor.from_torch_sparse_coo_tensor(sp @ sp, False)
    if adj2.product_bit_rows() is None:
        raise SystemExit("this A² has no bit rows: the A³-free route does not apply")
    r, c, _ = adj.coo()
    edges = sample_edges(r.cpu(), c.cpu(), n, a.batch * max(a.loop_batches, 1), seed=1).to(dev)
    e = edges[:, :a.batch].contiguous()
    nds = adj.neighbor_degree_sum()
    bound = int(nds[e[0]].sum())
    longest = _longest_item(adj, nds, e[0])
    with ops.prevalidated(e[0], e[1], n, n), torch.no_grad():
        for _ in range(a.warmup):
            st = CNState3(adj, adj2, None, e)
        torch.cuda.synchronize()
        timer = _Timer()
        ops.stage_timer = timer
        try:
            for _ in range(a.reps):
                st = CNState3(adj, adj2, None, e)
                torch.cuda.synchronize()
        finally:
            ops.stage_timer = None
    stages = timer.stages()
    entries = int(st.cnt3.sum())
    H = 256
    torch.manual_seed(0)
    pred = predictor_dict["cn6"](H, H, 1, 3, 0.0, 0.0, True).eval().to(dev)
    x = torch.randn(n, H, device=dev)
    loop_edges = edges.t().contiguous()
    score_edges(pred, x, adj, adj2, loop_edges[:a.batch], a.batch)            # warm-up: caches, panels
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    scores = score_edges(pred, x, adj, adj2, loop_edges, a.batch)
    t1.record()
    t1.synchronize()
    loop_ms = t0.elapsed_time(t1)

    def stat(v):
        return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), n=len(v))
    med3 = statistics.median(stages["cn3_flags"])
    out = {"tool": "cn3bench", "config": a.config, "scale": a.scale, "nodes": n, "nnz": adj.nnz(), "max_deg": adj.max_rowcount(),
           "batch": a.batch, "reps": a.reps, "bit_row_bytes": int(adj2.product_bit_rows().shape[1]) * 4,
           "stages_ms": {k: stat(v) for k, v in stages.items() if k in ("cn_prep", "cn_flags", "cn3_prep", "cn3_flags")},
           "probe_bound": bound, "longest_item_elements": longest, "cn3_entries": entries,
           "probe_bound_per_second": round(bound / (med3 * 1e-3), 1),
           "score_edges": {"H": H, "candidates": int(scores.numel()), "ms": round(loop_ms, 3),
                           "candidates_per_second": round(scores.numel() / (loop_ms * 1e-3), 1)},
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
