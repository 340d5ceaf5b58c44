"""The capped pooling at the collab shape (gin, H = 256, B = 65 536, cn5, the bench graph): what ``predictor.set_cn_cap`` makes
of the pooling and of the ``score_edges`` loop, how much of a batch a cap touches, and what the sample does to the scores.  One
process, every arm interleaved pass by pass; the baseline of every ratio is the uncapped arm of the same run, which is the
code path without the capped kernel.

    python tools/capbench.py [--batches 4] [--repeats 12] [--loop-repeats 10] [--sources 4096] [--out profiles/capbench_collab.json]

    arms     no cap and cap 16 / 32 / 64 / 128, each with the batch's own column weights and with a frozen table
             (``frozen.freeze_columns`` on the first batch).
    pooling  ``predictor._pool`` on prepared batch states (intersection pass, weights, class order and schedule done, as phase A
             of a scoring loop leaves them), between two device events that end in a synchronise.
    loop     ``pipeline.score_edges`` over the same batches, ms per batch.
    touched  per cap, from the flag bytes: the share of candidates with more members than the cap, and the members pooled
             (sum of min(u, cap)) against all members.
    scores   against the uncapped scores of the same weights: max and RMS |dscore|, beside the standard deviation of the scores;
             ``recommend_links(k = 20)``: mean overlap with the uncapped lists over the sources that have candidates.
    ddi      one ddi-shaped arm (cn7, H = 64): pooling and loop with no cap (which takes the row-sum shortcut) and ``--ddi-cap``.

Every shape is warmed before it is timed.  The figures are those of a synthetic graph under an untrained model: recorded, not
gates, and no claim about a dataset."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = (None, 16, 32, 64, 128)


def event_ms(fn):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def spread(t):
    return dict(median=round(statistics.median(t), 4), min=round(min(t), 4), max=round(max(t), 4), passes=len(t))


def name(frozen, cap):
    return ("frozen" if frozen else "own") + ("/exact" if cap is None else f"/cap{cap}")


def member_counts(st):
    """u per candidate, from the flag bytes."""
    import torch
    total = int(st.off[-1])
    cs = torch.zeros(total + 1, dtype=torch.int64, device=st.flags.device)
    cs[1:] = (st.flags[:total] != 0).to(torch.int64).cumsum(0)
    return cs[st.off[1:]] - cs[st.off[:-1]]


def measure(wl, a, caps, frozen_arms, seed, dev):
    """Pooling, loop, touched share and score differences of one workload; arms = frozen_arms x caps."""
    import torch
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.pipeline import score_edges
    from ocn_amd.recommend import recommend_links
    from ocn_amd.utils import adjoverlap, fuse
    pred, h, adj, adj2, args = wl["pred"], wl["h"], wl["adj"], wl["adj2"], wl["args"]
    B, H = wl["cfg"]["batch"], h.shape[1]
    edges = torch.cat(wl["edges"], dim=1).t().contiguous()               # [batches * B, 2]: the split_edge layout
    arms = [(f, c) for f in frozen_arms for c in caps]
    out = {"batch": B, "H": H, "n": wl["n"], "nnz": wl["nnz"], "nnz2": wl["nnz2"], "max_deg": wl["max_deg"], "seed": seed,
           "arms": [name(*arm) for arm in arms]}
    fc = freeze_columns(pred, adj, adj2, edges[:B].contiguous(), args) if True in frozen_arms else None

    def setup(frozen, cap):
        pred.set_frozen_columns(fc if frozen else None, args if frozen else None)
        pred.set_cn_cap(cap, seed=seed) if cap is not None else pred.set_cn_cap(None)

    with torch.no_grad():
        # ---- the pooling alone, on prepared batch states
        states, u_all = [], []
        for e in wl["edges"]:
            e = e.contiguous()
            st = fuse(adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e), e, {}, adj=adj)
            setup(False, None)
            w = pred._weights(st, args)
            pred._class_order(st, h)
            st.prepare_schedule(H)
            states.append((st, {False: w, True: fc.weights if fc is not None else None}))
            u_all.append(member_counts(st))
        u = torch.cat(u_all)
        out["members_per_candidate"] = dict(mean=float(u.double().mean()), max=int(u.max()), p90=float(torch.quantile(u.double(), 0.9)))
        out["touched"] = {str(c): dict(share_of_candidates_over_cap=float((u > c).double().mean()),
                                       members_pooled_over_all=float(u.clamp(max=c).sum()) / max(float(u.sum()), 1.0))
                          for c in caps if c is not None}

        def pool(st, ws, arm):
            setup(*arm)
            return pred._pool(st, ws[arm[0]], h)
        for st, ws in states:                                            # warm: every state in every arm, twice
            for _ in range(2):
                for arm in arms:
                    pool(st, ws, arm)
        torch.cuda.synchronize()
        times = {arm: [] for arm in arms}
        for rep in range(a.repeats):
            k = rep % len(arms)
            for st, ws in states:
                for arm in arms[k:] + arms[:k]:                          # the arms change places from pass to pass
                    setup(*arm)
                    times[arm].append(event_ms(lambda: pred._pool(st, ws[arm[0]], h)))
        out["pooling_ms"] = {name(*arm): spread(t) for arm, t in times.items()}
        out["class_major_rows"] = states[0][0].cls is not None
        for arm in arms:
            print(f"pooling {name(*arm):14s}: median {out['pooling_ms'][name(*arm)]['median']:.4f} ms", flush=True)
        del states
        # ---- the score_edges loop
        def run(arm):
            setup(*arm)
            return score_edges(pred, h, adj, adj2, edges, B, args)
        scores = {}
        for arm in arms:
            for _ in range(2):
                scores[arm] = run(arm)
        torch.cuda.synchronize()
        loop = {arm: [] for arm in arms}
        for rep in range(a.loop_repeats):
            k = rep % len(arms)
            for arm in arms[k:] + arms[:k]:
                setup(*arm)
                loop[arm].append(event_ms(lambda: score_edges(pred, h, adj, adj2, edges, B, args)) / len(wl["edges"]))
        out["score_edges_ms_per_batch"] = {name(*arm): spread(t) for arm, t in loop.items()}
        for arm in arms:
            print(f"score_edges {name(*arm):14s}: median {out['score_edges_ms_per_batch'][name(*arm)]['median']:.4f} ms per batch", flush=True)
        # ---- what the sample does to the scores
        out["scores"] = {}
        sources = torch.randperm(wl["n"], generator=torch.Generator().manual_seed(1))[:a.sources].sort()[0].to(dev)
        k = 20
        for frozen in frozen_arms:
            ref = scores[(frozen, None)].double()
            setup(frozen, None)
            base = recommend_links(pred, h, adj, adj2, sources, k, B, args)[0] if a.sources else None
            out["scores"][name(frozen, None)] = dict(std=float(ref.std()), mean_abs=float(ref.abs().mean()))
            for cap in caps:
                if cap is None:
                    continue
                d = (scores[(frozen, cap)].double() - ref).abs()
                rec = dict(max_abs_dscore=float(d.max()), rms_dscore=float((d * d).mean().sqrt()))
                if base is not None:
                    setup(frozen, cap)
                    got = recommend_links(pred, h, adj, adj2, sources, k, B, args)[0]
                    some = (base >= 0).any(1)
                    g_, b_ = got[some], base[some]
                    hit = ((g_[:, :, None] == b_[:, None, :]) & (b_[:, None, :] >= 0)).any(2).sum(1).double()
                    rec.update(top20_mean_overlap=float((hit / (b_ >= 0).sum(1).double()).mean()),
                               top20_identical_lists=float((g_ == b_).all(1).double().mean()), sources_with_candidates=int(some.sum()))
                out["scores"][name(frozen, cap)] = rec
                print(f"scores {name(frozen, cap)}: {json.dumps(rec)}", flush=True)
    setup(False, None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=12, help="passes of the pooling timing (every pass pools every batch)")
    ap.add_argument("--loop-repeats", type=int, default=10, help="passes of the score_edges timing")
    ap.add_argument("--sources", type=int, default=4096, help="sources of the recommend_links comparison (0: none)")
    ap.add_argument("--seed", type=int, default=0, help="the sample's seed")
    ap.add_argument("--ddi-cap", type=int, default=64, help="the cap of the ddi-shaped cn7 arm (0: no such arm)")
    ap.add_argument("--ddi-batches", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 10 or a.loop_repeats < 10:
        ap.error("medians of at least ten passes")
    sys.path.insert(0, ROOT)
    import torch
    import bench
    dev = torch.device("cuda:0")
    ns = lambda **kw: SimpleNamespace(hiddim=None, batch=a.batch, scale=a.scale, full=False, innerprod=0.0, **kw)
    wl = bench.build_workload(ns(dataset=a.config, predictor="cn5", batches=a.batches), dev, 0, 1)
    out = {"workload": f"{a.config}-shaped synthetic graph (bench.py's), cn5, {a.batches} batches; times in ms between device events; "
                       "every ratio against the exact arm of this run"}
    out.update(measure(wl, a, CAPS, (False, True), a.seed, dev))
    del wl
    torch.cuda.empty_cache()
    if a.ddi_cap > 0:
        a.sources = 0
        wl = bench.build_workload(ns(dataset="ddi", predictor="cn7", batches=a.ddi_batches), dev, 0, 1)
        out["ddi_cn7"] = measure(wl, a, (None, a.ddi_cap), (False,), a.seed, dev)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
