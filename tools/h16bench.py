"""Half-precision embedding tables at the collab shape (gin, H = 256, B = 65 536, cn5, the bench graph): what the pooling costs
from an fp32, a bf16 and an f16 table, what the ``score_edges`` loop makes of it, and what the rounding of the table does to
the scores.  One process, the three arms interleaved pass by pass.

    python tools/h16bench.py [--batches 4] [--repeats 20] [--loop-repeats 5] [--sources 4096] [--out profiles/h16bench_collab.json]

    pooling  ``st.gather`` on prepared batch states (intersection pass, weights, class order and schedule done, as phase A of a
             scoring loop leaves them): per pass, each batch state is pooled once from each table, between two device events
             that end in a synchronise.  The fp32 arm is ``ocn_cn_gather``, untouched by the half tables: the yardstick.
    loop     ``pipeline.score_edges`` over the same batches, ms per batch, for the three tables.
    rounding against the scores of the un-rounded fp32 embeddings on the same batches: max and 99.9th percentile of |dscore|;
             ``recommend_links(k = 20)`` for ``--sources`` sources: the share of identical lists and the mean overlap, over the
             sources that have candidates; table bytes.  (``cn_entries_per_batch``: the flag positions of a batch, i.e. the summed
             source-row lengths its pooling walks.)

Every shape is warmed before it is timed.  The figures are those of a synthetic graph under an untrained model: recorded, not
gates, and no claim about a dataset."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("fp32", "bf16", "f16")


def event_ms(fn):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def spread(t):
    return dict(median=round(statistics.median(t), 4), min=round(min(t), 4), max=round(max(t), 4), passes=[round(x, 4) for x in t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20, help="passes of the pooling timing")
    ap.add_argument("--loop-repeats", type=int, default=5, help="passes of the score_edges timing")
    ap.add_argument("--sources", type=int, default=4096, help="sources of the recommend_links comparison")
    ap.add_argument("--innerprod", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from ocn_amd.pipeline import embedding_table, score_edges
    from ocn_amd.recommend import recommend_links
    from ocn_amd.utils import adjoverlap, fuse
    dev = torch.device("cuda:0")
    wl = bench.build_workload(SimpleNamespace(dataset=a.config, hiddim=None, predictor="cn5", batch=a.batch, scale=a.scale,
                                              full=False, batches=a.batches, innerprod=a.innerprod), dev, 0, 1)
    pred, h, adj, adj2, args = wl["pred"], wl["h"], wl["adj"], wl["adj2"], wl["args"]
    B, H = wl["cfg"]["batch"], h.shape[1]
    tables = {arm: embedding_table(h, arm) for arm in ARMS}
    edges = torch.cat(wl["edges"], dim=1).t().contiguous()               # [batches * B, 2]: the split_edge layout
    out = {"workload": f"{a.config}-shaped synthetic graph (bench.py's), cn5 with innerprod = {a.innerprod}, B = {B}, H = {H}, "
                       f"{a.batches} batches; times in ms between device events",
           "batch": B, "H": H, "n": wl["n"], "nnz": wl["nnz"], "nnz2": wl["nnz2"], "max_deg": wl["max_deg"],
           "table_bytes": {arm: int(t.numel() * t.element_size()) for arm, t in tables.items()}}
    with torch.no_grad():
        # ---- the pooling alone, on prepared batch states
        states = []
        for e in wl["edges"]:
            e = e.contiguous()
            st = fuse(adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e), e, {}, adj=adj)
            w = pred._weights(st, args)
            pred._class_order(st, h)
            st.prepare_schedule(H)
            states.append((st, w, st.cls[1] if st.cls is not None else None))
        pool = lambda st, w, out_row, t: st.gather(w, t, out_row=out_row)
        for st, w, out_row in states:                                    # warm: every state from every table, twice
            for _ in range(2):
                for arm in ARMS:
                    pool(st, w, out_row, tables[arm])
        torch.cuda.synchronize()
        times = {arm: [] for arm in ARMS}
        for rep in range(a.repeats):
            order = ARMS[rep % 3:] + ARMS[:rep % 3]                      # the arms change places from pass to pass
            for st, w, out_row in states:
                for arm in order:
                    times[arm].append(event_ms(lambda: pool(st, w, out_row, tables[arm])))
        # (bit equality of the two half arms with the fp32 entry on the widened table, on the bench's own batch)
        st, w, out_row = states[0]
        same = {}
        for arm in ARMS[1:]:
            got = [o.clone() for o in pool(st, w, out_row, tables[arm])]
            ref = pool(st, w, out_row, tables[arm].float())
            same[arm] = all(torch.equal(g.view(torch.int32), r.view(torch.int32)) for g, r in zip(got, ref))
        out["pooling_ms"] = {arm: spread(t) for arm, t in times.items()}
        out["pooling_bits_equal_fp32_entry_on_widened_table"] = same
        out["class_major_rows"] = states[0][2] is not None
        out["cn_entries_per_batch"] = [int(st.off[-1]) for st, _, _ in states]
        for arm in ARMS:
            print(f"pooling {arm:5s}: median {out['pooling_ms'][arm]['median']:.4f} ms  (min {out['pooling_ms'][arm]['min']:.4f}, "
                  f"max {out['pooling_ms'][arm]['max']:.4f})", flush=True)
        del states
        # ---- the score_edges loop
        run = lambda t: score_edges(pred, t, adj, adj2, edges, B, args)
        scores = {}
        for arm in ARMS:
            for _ in range(2):
                scores[arm] = run(tables[arm])
        torch.cuda.synchronize()
        loop = {arm: [] for arm in ARMS}
        for rep in range(a.loop_repeats):
            for arm in ARMS[rep % 3:] + ARMS[:rep % 3]:
                loop[arm].append(event_ms(lambda: run(tables[arm])) / a.batches)
        out["score_edges_ms_per_batch"] = {arm: spread(t) for arm, t in loop.items()}
        for arm in ARMS:
            print(f"score_edges {arm:5s}: median {out['score_edges_ms_per_batch'][arm]['median']:.4f} ms per batch", flush=True)
        # ---- what the rounding costs
        ref = scores["fp32"].double()
        out["score_abs"] = dict(mean=float(ref.abs().mean()), std=float(ref.std()))
        out["rounding"] = {}
        sources = torch.randperm(wl["n"], generator=torch.Generator().manual_seed(1))[:a.sources].sort()[0].to(dev)
        k = 20
        lists = {arm: recommend_links(pred, tables[arm], adj, adj2, sources, k, B, args)[0] for arm in ARMS}
        for arm in ARMS[1:]:
            d = (scores[arm].double() - ref).abs()
            a_, b_ = lists[arm], lists["fp32"]
            some = (b_ >= 0).any(1)                                      # (a source without candidates has an empty list in every arm)
            a_, b_ = a_[some], b_[some]
            hit = ((a_[:, :, None] == b_[:, None, :]) & (b_[:, None, :] >= 0)).any(2).sum(1).double()
            full = (b_ >= 0).sum(1).double()
            out["rounding"][arm] = dict(max_abs_dscore=float(d.max()), p999_abs_dscore=float(torch.quantile(d, 0.999)),
                                        identical_lists=float((a_ == b_).all(1).double().mean()),
                                        mean_overlap=float((hit / full).mean()), sources=int(sources.numel()),
                                        sources_with_candidates=int(some.sum()), k=k)
            print(f"rounding {arm}: {json.dumps(out['rounding'][arm])}", flush=True)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
