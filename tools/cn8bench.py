"""cn8's two routes against cn7's scoring loop at the collab shape (B = 65 536, gin, H = 256): one GPU process per arm, each
under its own time limit, the arms alternated round by round in one call.

    (a) cn7   — the scoring loop of ``pipeline.score_edges`` with the cn7 predictor; with ``--baseline-lib PATH`` on a library
                built from the commit before cn8 (its kernels are the same sources: the arm shows that nothing moved)
    (b) unit  — cn8 through flags -> unit weights {1, 0, 1, 0} -> the pooling of cn5 / cn7 (``OCN_CN8_FUSED=0``)
    (c) fused — cn8 through ``ocn_cn8_pool``: intersection and pooling in one pass

    python tools/cn8bench.py [--rounds 3] [--batches 8] [--repeats 5] [--out profiles/cn8bench.json]

Every child scores the same ``--batches`` batches ``--repeats`` times and reports the time of each pass; the parent prints and
writes per arm the median and the range over all passes of all rounds.  A child that ends abnormally ends the run: nothing
more is started on the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = {"cn7": ("cn7", None), "unit": ("cn8", "0"), "fused": ("cn8", "1")}


def child(a):
    sys.path.insert(0, ROOT)
    from ocn_amd import _lib
    if a.arm == "cn7" and os.environ.get("OCN_LIB_PATH"):
        _lib.SIGNATURES.pop("ocn_cn8_pool", None)          # (a library from before cn8 does not export it; cn7 never calls it)
    import torch
    import bench
    from ocn_amd import ops
    from ocn_amd.pipeline import score_edges
    dev = torch.device("cuda:0")
    wl = bench.build_workload(SimpleNamespace(dataset=a.config, hiddim=None, predictor=ARMS[a.arm][0], batch=a.batch, scale=a.scale,
                                              full=False, batches=a.batches), dev, 0, 1)
    pred, h, adj, adj2, args = wl["pred"], wl["h"], wl["adj"], wl["adj2"], wl["args"]
    B = wl["cfg"]["batch"]
    edges = torch.cat(wl["edges"], dim=1).t().contiguous()              # [batches * B, 2]: the split_edge layout
    assert a.arm == "cn7" or ops.cn8_fused_eval == (ARMS[a.arm][1] == "1")
    with torch.no_grad():
        for _ in range(2):
            s = score_edges(pred, h, adj, adj2, edges, B, args)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            s = score_edges(pred, h, adj, adj2, edges, B, args)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / a.batches)
    print("CN8BENCH " + json.dumps({"arm": a.arm, "ms_per_batch": [round(1e3 * t, 4) for t in times], "batch": B, "batches": a.batches,
                                    "n": wl["n"], "nnz": wl["nnz"], "nnz2": wl["nnz2"], "max_deg": wl["max_deg"],
                                    "score_sum": float(s.double().sum()), "lib": os.environ.get("OCN_LIB_PATH", "in-tree")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=sorted(ARMS), help="(internal) run one arm in this process")
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--arms", default="cn7,unit,fused")
    ap.add_argument("--baseline-lib", default=None, help="libocn_hip.so built from the commit before cn8, for arm cn7")
    ap.add_argument("--limit", type=int, default=240, help="seconds one child may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        return child(a)
    runs = {arm: [] for arm in a.arms.split(",")}
    meta = {}
    for rnd in range(a.rounds):
        for arm in runs:
            env = dict(os.environ)
            env.pop("OCN_LIB_PATH", None)
            if ARMS[arm][1] is not None:
                env["OCN_CN8_FUSED"] = ARMS[arm][1]
            if arm == "cn7" and a.baseline_lib:
                env["OCN_LIB_PATH"] = os.path.abspath(a.baseline_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--config", a.config, "--scale", str(a.scale),
                   "--batches", str(a.batches), "--repeats", str(a.repeats)] + (["--batch", str(a.batch)] if a.batch else [])
            try:
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(f"arm {arm} round {rnd}: over its {a.limit} s limit; stopping", flush=True)
                return 2
            line = [l for l in p.stdout.splitlines() if l.startswith("CN8BENCH ")]
            if p.returncode != 0 or not line:
                print(f"arm {arm} round {rnd}: exit status {p.returncode}; stopping\n{p.stderr[-2000:]}", flush=True)
                return 2
            r = json.loads(line[-1][len("CN8BENCH "):])
            runs[arm] += r.pop("ms_per_batch")
            meta[arm] = r
            print(f"round {rnd} {arm:5s}: median {statistics.median(runs[arm][-a.repeats:]):.4f} ms per batch", flush=True)
    out = {"workload": f"{a.config}-shaped synthetic graph, pipeline.score_edges over {a.batches} batches, ms per batch",
           "rounds": a.rounds, "repeats": a.repeats,
           "arms": {arm: dict(median=statistics.median(t), min=min(t), max=max(t), passes=t, **meta[arm]) for arm, t in runs.items()}}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
