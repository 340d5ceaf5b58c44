"""Hard negatives at a named shape (collab by default): what the 2-hop sampler (``ocn_sample_two_hop``) costs beside the route
that can be composed without it — materialise ``two_hop_candidates`` in chunks under ``ops.prefilter_budget`` and index the
``r``-th candidate of every slot — in time and in peak memory.  Both routes draw the same ``r`` (the composed one through
``ops.philox4x32`` and a multiply-high restated in torch), so their results are compared for equality inside the run.  Device
events around every call, warm-up, medians and ranges.  One GPU process at a time: every arm runs in a child of its own under
its own time limit, and the first arm that fails or runs over ends the tool.

    e   one epoch's draw: ``two_hop_negative_edges`` for the training positives of ``synth.loaddataset_like`` (1.18 M at the
        collab shape), grouped by their unique sources;
    t   evaluation negatives: ``two_hop_negative_targets`` for Q random sources x PER targets (4 096 x 1 000).

    python tools/hardnegbench.py --out profiles/hardnegbench_collab.json

Prints (and with ``--out`` writes) one JSON line.  No figure is a pass condition.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("e", "t")


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    from ocn_amd import ops, sampling as S
    from ocn_amd.synth import loaddataset_like
    if not torch.cuda.is_available():
        raise SystemExit("hardnegbench needs a GPU: a CPU run says nothing about these kernels")
    dev = torch.device("cuda:0")
    seed = a.seed
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32

    def ranks(ctr, c):
        """floor(u * c / 2^64) for the 64-bit word of every counter row (int64 [T, 4] of uint32 values) and c < 2^30."""
        bits = torch.where(ctr >= (1 << 31), ctr - (1 << 32), ctr).to(torch.int32).contiguous()
        w = ops.philox4x32(bits, k0, k1).to(torch.int64) & 0xFFFFFFFF
        return (w[:, 1] * c + ((w[:, 0] * c) >> 32)) >> 32

    def composed(adj, rows, sptr, ctr_of):
        """The samples of ``ops.sample_two_hop(adj, adj, rows, sptr, ..)`` from materialised candidate lists: the sources in
        chunks whose lists stay under ``ops.prefilter_budget`` pairs; ``ctr_of(q, j, i)``: the counter rows of the slots."""
        a_ = (adj._rowptr, adj._col)
        count = ops.two_hop_diff_count(*a_, *a_, rows)
        assert int(count.max()) < (1 << 30)
        ends = torch.cumsum(count.to(torch.int64), 0).cpu()
        host_sptr = sptr.cpu()
        out = torch.full((int(host_sptr[-1]),), -1, dtype=torch.int64, device=dev)
        q0, chunks = 0, 0
        while q0 < rows.numel():
            done = int(ends[q0 - 1]) if q0 else 0
            q1 = max(q0 + 1, int(torch.searchsorted(ends, done + ops.prefilter_budget, right=True)))
            ptr = ops.scan_i32(count[q0:q1])                 # two_hop_candidates' count -> scan -> fill, the count pass shared
            edges = ops.two_hop_diff_fill(*a_, *a_, rows[q0:q1], ptr, total=int(ends[q1 - 1]) - done)
            s0, s1 = int(host_sptr[q0]), int(host_sptr[q1])
            lens = sptr[q0 + 1:q1 + 1] - sptr[q0:q1]
            q = torch.repeat_interleave(torch.arange(q1 - q0, device=dev), lens)
            i = torch.arange(s0, s1, device=dev)
            c = count[q0:q1].to(torch.int64)[q]
            r = ranks(ctr_of(q + q0, i - sptr[q0:q1][q], i), c)
            live = c > 0
            out[s0:s1][live] = edges[(ptr[:-1][q] + r)[live], 1]
            q0, chunks = q1, chunks + 1
            del ptr, edges
        return out, chunks

    def measure(fn, reps):
        """([ms], peak bytes above what was allocated before the call, the last result)"""
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts, peak, res = [], 0, None
        for _ in range(reps):
            res = None
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            res = fn()
            t1.record()
            t1.synchronize()
            ts.append(round(t0.elapsed_time(t1), 3))
            peak = max(peak, torch.cuda.max_memory_allocated() - before)
        return ts, peak, res

    out = {"arm": a.arm}
    with torch.no_grad():
        data, split_edge = loaddataset_like(a.config, False, scale=a.scale)
        adj = data.adj_t.to_device(dev)
        n = adj.size(0)
        out.update(nodes=n, nnz=adj.nnz(), max_deg=adj.max_rowcount())
        zero = torch.zeros(1, dtype=torch.int64, device=dev)
        if a.arm == "e":
            pos = split_edge["train"]["edge"].to(dev).t().contiguous()
            E = pos.shape[1]

            def direct():
                return S.two_hop_negative_edges(adj, pos, seed, fallback=None)[1]

            def by_lists():
                src = pos[0].contiguous()
                rows, inverse, counts = torch.unique(src, return_inverse=True, return_counts=True)
                order = torch.argsort(inverse, stable=True)
                sptr = torch.cat((zero, torch.cumsum(counts, 0)))
                slots, chunks = composed(adj, rows, sptr,
                                         lambda q, j, i: torch.stack((order[i] & 0xFFFFFFFF, order[i] >> 32, torch.zeros_like(i),
                                                                      torch.full_like(i, 4)), 1))
                tgt = torch.empty_like(slots)
                tgt[order] = slots
                by_lists.chunks, by_lists.sources = chunks, rows.numel()
                return tgt
            reps = a.reps
        else:
            Q, per = a.sources, a.per
            src = torch.randint(0, n, (Q,), generator=torch.Generator().manual_seed(7)).to(dev)
            E = Q * per

            def direct():
                return S.two_hop_negative_targets(adj, src, per, seed, fallback=None).view(-1)

            def by_lists():
                sptr = torch.arange(Q + 1, device=dev) * per
                slots, chunks = composed(adj, src, sptr,
                                         lambda q, j, i: torch.stack((j, q & 0xFFFFFFFF, q >> 32, torch.full_like(i, 3)), 1))
                by_lists.chunks, by_lists.sources = chunks, Q
                return slots
            reps = a.reps
        ms_d, peak_d, got = measure(direct, reps)
        ms_c, peak_c, want = measure(by_lists, reps)
        out.update(samples=E, sources=by_lists.sources, chunks=by_lists.chunks, without_candidate=int((got < 0).sum()),
                   results_equal=bool(torch.equal(got, want)),
                   sampler=dict(ms=ms_d, peak_bytes=int(peak_d)), composed=dict(ms=ms_c, peak_bytes=int(peak_c)))
    print("HARDNEGBENCH " + json.dumps(out), flush=True)


def summary(samples):
    return dict(median=round(statistics.median(samples), 4), min=round(min(samples), 4), max=round(max(samples), 4), n=len(samples))


def summarise(r):
    if isinstance(r, dict):
        return {k: (summary(v) if k == "ms" else summarise(v)) for k, v in r.items()}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default=None, choices=ARMS, help="(internal) run one arm")
    ap.add_argument("--arms", default="et", help="the arms to run, in this order")
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sources", type=int, default=4096)
    ap.add_argument("--per", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=20250101)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=240, help="seconds one arm may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        return child(a)
    passed = [f"--{k.replace('_', '-')}={v}" for k, v in vars(a).items() if k not in ("arm", "arms", "out", "limit")]
    out = {"tool": "hardnegbench", "config": a.config, "scale": a.scale, "sources": a.sources, "per": a.per, "arms": {}}
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
        line = [l for l in p.stdout.splitlines() if l.startswith("HARDNEGBENCH ")]
        if p.returncode != 0 or not line:
            print(f"arm {arm}: exit {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            out["arms"][arm] = f"exit {p.returncode}"
            rc = 2
            break
        r = summarise(json.loads(line[0][len("HARDNEGBENCH "):]))
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
