"""Frozen column weights against batch-coupled scoring at the collab shape (gin, H = 256, B = 65 536, cn5 with a trained
checkpoint's ``innerprod`` = 0.37): one GPU process per arm, each under its own time limit, the arms alternated round by round
in one call.

    (a) unfrozen — the scoring loop of ``pipeline.score_edges`` as it was; with ``--baseline-lib PATH`` on a library built from
                   the commit before the frozen tables (the yardstick: "frozen serving costs no more than batch-coupled scoring")
    (b) chain    — frozen, ``OCN_FROZEN_FUSED=0``: flags -> the frozen table in place of the batch's weights -> the pooling
    (c) fused    — frozen, ``OCN_FROZEN_FUSED=1``: ``ocn_cn_pool_frozen``, intersection and weighted pooling in one pass

    python tools/frozenbench.py [--rounds 3] [--batches 8] [--repeats 5] [--out profiles/frozenbench.json]

Every child scores the same ``--batches`` batches ``--repeats`` times between two device events and reports the time of each
pass; (b) and (c) also time a small request, ``recommend_links`` for 16 sources with k = 100, the same way.  The table is frozen
on the first batch.  The parent prints and writes per arm the median and the range over all passes of all rounds.  A child that
ends abnormally ends the run: nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = {"unfrozen": None, "chain": "0", "fused": "1"}       # arm -> OCN_FROZEN_FUSED
TAG = "FROZENBENCH "


def timed(fn, repeats):
    """Milliseconds of each of ``repeats`` calls of ``fn``, between two device events on the current stream."""
    import torch
    out = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    return out


def child(a):
    sys.path.insert(0, ROOT)
    from ocn_amd import _lib
    if a.arm == "unfrozen" and os.environ.get("OCN_LIB_PATH"):
        _lib.SIGNATURES.pop("ocn_cn_pool_frozen", None)    # (a library from before the frozen tables does not export it; this arm never calls it)
    import torch
    import bench
    from ocn_amd import ops
    from ocn_amd.frozen import freeze_columns
    from ocn_amd.pipeline import score_edges
    from ocn_amd.recommend import recommend_links
    dev = torch.device("cuda:0")
    wl = bench.build_workload(SimpleNamespace(dataset=a.config, hiddim=None, predictor="cn5", batch=a.batch, scale=a.scale,
                                              full=False, batches=a.batches, innerprod=a.innerprod), dev, 0, 1)
    pred, h, adj, adj2, args = wl["pred"], wl["h"], wl["adj"], wl["adj2"], wl["args"]
    B = wl["cfg"]["batch"]
    edges = torch.cat(wl["edges"], dim=1).t().contiguous()              # [batches * B, 2]: the split_edge layout
    small = None
    if a.arm != "unfrozen":
        assert ops.frozen_fused_eval == (ARMS[a.arm] == "1")
        pred.set_frozen_columns(freeze_columns(pred, adj, adj2, edges[:B].contiguous(), args))
    with torch.no_grad():
        run = lambda: score_edges(pred, h, adj, adj2, edges, B, args)
        for _ in range(2):
            s = run()
        torch.cuda.synchronize()
        times = [t / a.batches for t in timed(run, a.repeats)]
        s = run()
        if a.arm != "unfrozen":
            sources = torch.randperm(wl["n"], generator=torch.Generator().manual_seed(1))[:16].to(dev)
            req = lambda: recommend_links(pred, h, adj, adj2, sources, 100, B, args)
            for _ in range(2):
                req()
            torch.cuda.synchronize()
            small = [round(t, 4) for t in timed(req, a.repeats)]
    print(TAG + json.dumps({"arm": a.arm, "ms_per_batch": [round(t, 4) for t in times], "ms_small_request": small, "batch": B,
                            "batches": a.batches, "n": wl["n"], "nnz": wl["nnz"], "nnz2": wl["nnz2"], "max_deg": wl["max_deg"],
                            "innerprod": a.innerprod, "score_sum": float(s.double().sum()),
                            "lib": os.path.relpath(os.environ["OCN_LIB_PATH"], ROOT) if os.environ.get("OCN_LIB_PATH") else "in-tree"}),
          flush=True)


def spread(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t), passes=t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=sorted(ARMS), help="(internal) run one arm in this process")
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--innerprod", type=float, default=0.37)
    ap.add_argument("--arms", default="unfrozen,chain,fused")
    ap.add_argument("--baseline-lib", default=None, help="libocn_hip.so built from the commit before the frozen tables, for arm unfrozen")
    ap.add_argument("--limit", type=int, default=240, help="seconds one child may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        return child(a)
    runs = {arm: [] for arm in a.arms.split(",")}
    small = {arm: [] for arm in runs}
    meta = {}
    for rnd in range(a.rounds):
        for arm in runs:
            env = dict(os.environ)
            env.pop("OCN_LIB_PATH", None)
            env.pop("OCN_FROZEN_FUSED", None)
            if ARMS[arm] is not None:
                env["OCN_FROZEN_FUSED"] = ARMS[arm]
            if arm == "unfrozen" and a.baseline_lib:
                env["OCN_LIB_PATH"] = os.path.abspath(a.baseline_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--config", a.config, "--scale", str(a.scale),
                   "--batches", str(a.batches), "--repeats", str(a.repeats), "--innerprod", str(a.innerprod)] \
                + (["--batch", str(a.batch)] if a.batch else [])
            try:
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(f"arm {arm} round {rnd}: over its {a.limit} s limit; stopping", flush=True)
                return 2
            line = [l for l in p.stdout.splitlines() if l.startswith(TAG)]
            if p.returncode != 0 or not line:
                print(f"arm {arm} round {rnd}: exit status {p.returncode}; stopping\n{p.stderr[-2000:]}", flush=True)
                return 2
            r = json.loads(line[-1][len(TAG):])
            runs[arm] += r.pop("ms_per_batch")
            small[arm] += r.pop("ms_small_request") or []
            meta[arm] = r
            print(f"round {rnd} {arm:8s}: median {statistics.median(runs[arm][-a.repeats:]):.4f} ms per batch"
                  + (f", small request {statistics.median(small[arm][-a.repeats:]):.4f} ms" if small[arm] else ""), flush=True)
    out = {"workload": f"{a.config}-shaped synthetic graph, cn5 with innerprod = {a.innerprod}, pipeline.score_edges over {a.batches} "
                       "batches, ms per batch between device events; small request: recommend_links for 16 sources, k = 100, ms",
           "rounds": a.rounds, "repeats": a.repeats,
           "arms": {arm: dict(**spread(t), small_request=spread(small[arm]) if small[arm] else None, **meta[arm])
                    for arm, t in runs.items()}}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
