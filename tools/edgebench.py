"""Message saliency at the collab shape (the graph of bench.py, H = 256): one GPU process per arm, each under its own time
limit, the arms alternated round by round in one call.

    (a) kernels — on the collab adjacency with random g and x [N, 256], alternated call by call in one process:
                  ``ocn_sddmm_csr`` (the plain sum form, gin's); the same values in torch, ``(g[row] * x[col]).sum(1)`` (two
                  nnz x H temporaries); ``ocn_spmm_csr`` on the same operator (the forward the SDDMM differentiates).  The kernel's
                  and torch's outputs are compared in the run with fp64 dots, entry by entry, within (H + 2) u sum|g x| + 1e-37
                  (u = 2^-24): the bound of tests/test_sddmm_gpu.py
    (b) explain — the whole of ``explain_link_edges(top=20)`` on bench.py's encoder, predictor and one candidate batch, next to
                  one ``predictor(...)`` call on the same batch and one encoder pass

    python tools/edgebench.py [--rounds 2] [--repeats 5] [--out profiles/edgebench_collab.json]

Every child warms its calls up, then times ``--repeats`` calls of each between two device events.  The parent prints and writes
per figure the median and the range over all calls of all rounds.  A child that ends abnormally ends the run: nothing more is
started on the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("kernels", "explain")
TAG = "EDGEBENCH "
U = 2.0 ** -24


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
        out.append(round(t0.elapsed_time(t1), 4))
    return out


def worst_ratio(g, x, row, col, got, H, chunk=1 << 16):
    """max over the entries of |got - d_exact| / ((H + 2) u sum|g x| + 1e-37), dots in fp64."""
    worst = 0.0
    for lo in range(0, row.numel(), chunk):
        s = slice(lo, lo + chunk)
        pr = g[row[s]].double() * x[col[s]].double()
        ratio = (got[s].double() - pr.sum(1)).abs() / ((H + 2) * U * pr.abs().sum(1) + 1e-37)
        worst = max(worst, float(ratio.max()))
    return worst


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from ocn_amd import ops
    dev = torch.device("cuda:0")
    out = {"arm": a.arm}
    if a.arm == "kernels":
        from ocn_amd.sparse import SparseTensor
        from ocn_amd.synth import dataset_like
        H = a.hiddim
        ei, n, _ = dataset_like(a.config, seed=0, scale=a.scale)
        adj = SparseTensor.from_edge_index(ei.to(dev), sparse_sizes=(n, n), trust_data=True).to_symmetric()
        rowptr, col = adj._rowptr, adj._col
        nnz = int(col.numel())
        gen = torch.Generator().manual_seed(1)
        g, x = torch.randn(n, H, generator=gen).to(dev), torch.randn(n, H, generator=gen).to(dev)
        row = torch.repeat_interleave(torch.arange(n, device=dev), rowptr[1:] - rowptr[:-1])
        coll = col.long()
        buf = torch.empty(nnz, dtype=torch.float32, device=dev)
        sddmm = lambda: ops.sddmm_csr(rowptr, col, g, x, out=buf)        # (its output allocated once, as a predictor's scratch is)
        ref = lambda: (g[row] * x[coll]).sum(1)
        spmm = lambda: ops.spmm_csr(rowptr, col, x)
        out.update(n=n, nnz=nnz, H=H, max_deg=adj.max_rowcount())
        with torch.no_grad():
            for _ in range(3):
                sddmm(); ref(); spmm()
            torch.cuda.synchronize()
            ms = {"ms_sddmm": [], "ms_torch": [], "ms_spmm": []}
            for _ in range(a.repeats):                                    # alternated call by call
                ms["ms_sddmm"] += timed(sddmm, 1)
                ms["ms_torch"] += timed(ref, 1)
                ms["ms_spmm"] += timed(spmm, 1)
            out.update(ms)
            ratios = {"kernel": worst_ratio(g, x, row, coll, sddmm(), H), "torch": worst_ratio(g, x, row, coll, ref(), H)}
        out["worst_error_over_bound"] = ratios
        out["outputs_agree_within_bound"] = bool(ratios["kernel"] <= 1.0 and ratios["torch"] <= 1.0)
        # what the kernel has to move at least: g and x once, the column ids, the output
        out["compulsory_bytes"] = 2 * n * H * 4 + nnz * 8 + (n + 1) * 8
    else:
        import ocn_amd.model as M
        from ocn_amd.explain import explain_link_edges
        from ocn_amd.synth import SHAPES
        from ocn_amd.utils import adjoverlap
        wl = bench.build_workload(SimpleNamespace(dataset=a.config, hiddim=a.hiddim, predictor="cn5", batch=a.batch, scale=a.scale,
                                                  full=False, batches=1, innerprod=a.innerprod), dev, 0, 1)
        cfg, n, adj, adj2, pred, args = wl["cfg"], wl["n"], wl["adj"], wl["adj2"], wl["pred"], wl["args"]
        if cfg["ids"]:
            raise SystemExit("edgebench: a configuration with feature inputs")
        # bench.py's encoder and features again, from its seed (build_workload returns h only)
        H = cfg["H"]
        fin = SHAPES[a.config]["feat"] or H
        torch.manual_seed(0)
        x = torch.randn(n, fin, device=dev)
        enc = getattr(M, cfg["enc"])(fin, H, H, cfg["layers"], 0.05, cfg["ln"], cfg["res"], -1, cfg["conv"], cfg["jk"], 0.0,
                                     xdropout=0.7, taildropout=0.3).to(dev).eval()
        e = wl["edges"][0].contiguous()
        edges = e.t().contiguous()
        with torch.no_grad():
            same = bool(torch.equal(enc(x, adj), wl["h"]))
        run = lambda: explain_link_edges(enc, pred, x, adj, adj2, edges, 0, top=20, args=args)
        with torch.no_grad():
            score = lambda: pred(wl["h"], adj, adjoverlap(adj, adj, e), adjoverlap(adj, adj2, e), e)
            encode = lambda: enc(x, adj)
            for _ in range(2):
                ex = run(); score(); encode()
            torch.cuda.synchronize()
            out["ms_explain"] = timed(run, a.repeats)
            out["ms_predictor_call"] = timed(score, a.repeats)
            out["ms_encoder_pass"] = timed(encode, a.repeats)
        out.update(batch=int(e.shape[1]), H=H, n=n, nnz=wl["nnz"], conv_layers=int(ex.per_layer.shape[1]), innerprod=a.innerprod,
                   encoder_is_the_benchmarks=same, listed=int((ex.entries[:, 0] >= 0).sum()))
    print(TAG + json.dumps(out), flush=True)


def spread(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t), calls=t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=ARMS, help="(internal) run one arm in this process")
    ap.add_argument("--config", default="collab")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--hiddim", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--innerprod", type=float, default=0.37)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--limit", type=int, default=240, help="seconds one child may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.arm:
        return child(a)
    runs = {arm: {} for arm in a.arms.split(",")}
    meta = {}
    for rnd in range(a.rounds):
        for arm in runs:
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--config", a.config, "--scale", str(a.scale),
                   "--hiddim", str(a.hiddim), "--repeats", str(a.repeats), "--innerprod", str(a.innerprod)] \
                + (["--batch", str(a.batch)] if a.batch else [])
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(f"arm {arm} round {rnd}: over its {a.limit} s limit; stopping", flush=True)
                return 2
            line = [l for l in p.stdout.splitlines() if l.startswith(TAG)]
            if p.returncode != 0 or not line:
                print(f"arm {arm} round {rnd}: exit status {p.returncode}; stopping\n{p.stderr[-2000:]}", flush=True)
                return 2
            r = json.loads(line[-1][len(TAG):])
            for key in [k for k in r if k.startswith("ms_")]:
                runs[arm].setdefault(key, []).extend(r.pop(key))
            meta[arm] = r
            print(f"round {rnd} {arm:8s}: " + ", ".join(f"{key} median {statistics.median(t[-a.repeats:]):.4f}"
                                                          for key, t in runs[arm].items()), flush=True)
    out = {"workload": f"{a.config}-shaped synthetic graph of bench.py, H = {a.hiddim}; ms per call between device events after a "
                       "warm-up; kernels: ocn_sddmm_csr (plain sum form), the same values in torch ((g[row] * x[col]).sum(1)) and "
                       "ocn_spmm_csr on the same operator, alternated in one process; explain: explain_link_edges(top=20) on "
                       f"bench.py's encoder and cn5 predictor (innerprod = {a.innerprod}) with ONE candidate batch, beside one "
                       "predictor call and one encoder pass",
           "rounds": a.rounds, "repeats": a.repeats,
           "arms": {arm: dict(**{key: spread(t) for key, t in r.items()}, **meta[arm]) for arm, r in runs.items()}}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
