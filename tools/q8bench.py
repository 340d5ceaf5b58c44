"""An int8 embedding table at the collab shape (gin, H = 256, B = 65 536, cn5, the bench graph): what the pooling costs from an
fp32, a bf16 and an int8 table — exact, and capped at ``--cap`` rows per candidate (fp32 and int8: a capped predictor refuses a
half table) — what the ``score_edges`` loop makes of it, what the tables weigh, and what the quantisation does to the scores.
One process, the arms interleaved pass by pass.

    python tools/q8bench.py [--batches 4] [--repeats 20] [--loop-repeats 5] [--cap 32] [--sources 4096] [--out profiles/q8bench_collab.json]

    pooling  ``st.gather`` on prepared batch states (intersection pass, weights, class order and schedule done, as phase A of a
             scoring loop leaves them): per pass, each batch state is pooled once per arm, between two device events that end
             in a synchronise.  The fp32 arms are ``ocn_cn_gather`` / ``ocn_cn_gather_cap``, untouched by the int8 table: the
             yardsticks.
    loop     ``pipeline.score_edges`` over the same batches, ms per batch, exact (three tables) and capped (fp32, int8).
    size     the resident bytes of each table (int8: padded rows and the scales — the image ``EmbeddingIndex.from_table`` shares).
    error    against the scores of the un-rounded fp32 embeddings on the same batches: max and RMS of |dscore| beside the
             scores' standard deviation; ``recommend_links(k = 20)`` for ``--sources`` sources: the share of identical lists and
             the mean overlap, over the sources that have candidates.

Every shape is warmed before it is timed.  The figures are those of a synthetic graph under an untrained model: recorded, not
gates, and no claim about a dataset, a trained model or a ranking metric."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("fp32", "bf16", "int8")
CAPPED = ("fp32", "int8")


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


def rotated(arms, rep):
    """The arms change places from pass to pass."""
    r = rep % len(arms)
    return arms[r:] + arms[:r]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20, help="passes of the pooling timing")
    ap.add_argument("--loop-repeats", type=int, default=5, help="passes of the score_edges timing")
    ap.add_argument("--cap", type=int, default=32, help="rows per candidate of the capped arms")
    ap.add_argument("--sources", type=int, default=4096, help="sources of the recommend_links comparison")
    ap.add_argument("--innerprod", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from ocn_amd.pipeline import embedding_table, embedding_table_int8, score_edges
    from ocn_amd.recommend import recommend_links
    from ocn_amd.utils import adjoverlap, fuse
    dev = torch.device("cuda:0")
    wl = bench.build_workload(SimpleNamespace(dataset=a.config, hiddim=None, predictor="cn5", batch=a.batch, scale=a.scale,
                                              full=False, batches=a.batches, innerprod=a.innerprod), dev, 0, 1)
    pred, h, adj, adj2, args = wl["pred"], wl["h"], wl["adj"], wl["adj2"], wl["args"]
    B, H = wl["cfg"]["batch"], h.shape[1]
    tables = {"fp32": h, "bf16": embedding_table(h, "bf16"), "int8": embedding_table_int8(h)}
    q8 = tables["int8"]
    edges = torch.cat(wl["edges"], dim=1).t().contiguous()               # [batches * B, 2]: the split_edge layout
    out = {"workload": f"{a.config}-shaped synthetic graph (bench.py's), cn5 with innerprod = {a.innerprod}, B = {B}, H = {H}, "
                       f"{a.batches} batches, cap = {a.cap}; times in ms between device events",
           "batch": B, "H": H, "n": wl["n"], "nnz": wl["nnz"], "nnz2": wl["nnz2"], "max_deg": wl["max_deg"], "cap": a.cap,
           "table_bytes": {"fp32": int(h.numel() * 4), "bf16": int(h.numel() * 2),
                           "int8": int(q8.rows.numel() + q8.scale.numel() * 4)}}
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
        pool = lambda st, w, out_row, t, cap=None: st.gather(w, t, out_row=out_row, cap=cap)
        cap = (a.cap, 0)
        arms = [(arm, None) for arm in ARMS] + [(arm, cap) for arm in CAPPED]
        name = lambda arm, c: arm if c is None else f"{arm}_cap{a.cap}"
        for st, w, out_row in states:                                    # warm: every state from every arm, twice
            for _ in range(2):
                for arm, c in arms:
                    pool(st, w, out_row, tables[arm], c)
        torch.cuda.synchronize()
        times = {name(*x): [] for x in arms}
        for rep in range(a.repeats):
            for st, w, out_row in states:
                for arm, c in rotated(arms, rep):
                    times[name(arm, c)].append(event_ms(lambda: pool(st, w, out_row, tables[arm], c)))
        # (bit equality of the int8 arms with the fp32 entries on the dequantised table, on the bench's own batch)
        st, w, out_row = states[0]
        qf = q8.float()
        same = {}
        for c in (None, cap):
            got = [o.clone() for o in pool(st, w, out_row, q8, c)]
            ref = pool(st, w, out_row, qf, c)
            same[name("int8", c)] = all(torch.equal(g.view(torch.int32), r.view(torch.int32)) for g, r in zip(got, ref))
        del qf
        out["pooling_ms"] = {k: spread(t) for k, t in times.items()}
        out["pooling_bits_equal_fp32_entry_on_dequantised_table"] = same
        out["class_major_rows"] = states[0][2] is not None
        out["cn_entries_per_batch"] = [int(st.off[-1]) for st, _, _ in states]
        for k, v in out["pooling_ms"].items():
            print(f"pooling {k:11s}: median {v['median']:.4f} ms  (min {v['min']:.4f}, max {v['max']:.4f})", flush=True)
        del states
        # ---- the score_edges loop

        def run(arm, c):
            pred.set_cn_cap(*(c or (None,)))
            try:
                return score_edges(pred, tables[arm], adj, adj2, edges, B, args)
            finally:
                pred.set_cn_cap(None)
        scores = {}
        for arm, c in arms:
            for _ in range(2):
                scores[name(arm, c)] = run(arm, c)
        torch.cuda.synchronize()
        loop = {name(*x): [] for x in arms}
        for rep in range(a.loop_repeats):
            for arm, c in rotated(arms, rep):
                loop[name(arm, c)].append(event_ms(lambda: run(arm, c)) / a.batches)
        out["score_edges_ms_per_batch"] = {k: spread(t) for k, t in loop.items()}
        for k, v in out["score_edges_ms_per_batch"].items():
            print(f"score_edges {k:11s}: median {v['median']:.4f} ms per batch", flush=True)
        # ---- what the quantisation costs: against the exact scores of the un-rounded table
        ref = scores["fp32"].double()
        out["score_abs"] = dict(mean=float(ref.abs().mean()), std=float(ref.std()))
        out["error"] = {}
        sources = torch.randperm(wl["n"], generator=torch.Generator().manual_seed(1))[:a.sources].sort()[0].to(dev)
        k = 20

        def top(arm, c):
            pred.set_cn_cap(*(c or (None,)))
            try:
                return recommend_links(pred, tables[arm], adj, adj2, sources, k, B, args)[0]
            finally:
                pred.set_cn_cap(None)
        lists = {name(*x): top(*x) for x in arms}
        for key in list(scores)[1:]:
            d = (scores[key].double() - ref).abs()
            a_, b_ = lists[key], lists["fp32"]
            some = (b_ >= 0).any(1)                                      # (a source without candidates has an empty list in every arm)
            a_, b_ = a_[some], b_[some]
            hit = ((a_[:, :, None] == b_[:, None, :]) & (b_[:, None, :] >= 0)).any(2).sum(1).double()
            full = (b_ >= 0).sum(1).double()
            out["error"][key] = dict(max_abs_dscore=float(d.max()), rms_abs_dscore=float(d.pow(2).mean().sqrt()),
                                     identical_lists=float((a_ == b_).all(1).double().mean()),
                                     mean_overlap=float((hit / full).mean()), sources=int(sources.numel()),
                                     sources_with_candidates=int(some.sum()), k=k)
            print(f"error {key}: {json.dumps(out['error'][key])}", flush=True)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
